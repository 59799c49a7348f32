"""Reference of the occupation seam of a joint of tables that share one halo table: the
composition of `vjp_reference` per table, in NumPy.  A helper of the joint VJP tests, not a test
module.

With g (N) the cotangent of the concatenated prediction and table t owning its slice:
``g_occ = sum_t vjp_t(g[slice t])`` with g_ngal counted ONCE (ngal is one number: the tables share
their bins), and the scale -- the terms that cancel in an element -- the sum of the tables'
scales.  The likelihood form is that product with ``g = 2 P_sym (xi - data)`` over all N rows,
``P_sym = (precision + precision^T) / 2``: the off-diagonal blocks couple the tables.  No new
tolerance: an element is allowed 1e-10 (|ref| + scale), and ngal, xi and chi2 the formulas of
test_gpu_vjp.py.
"""

import numpy as np

import vjp_reference


def slices_of(tables):
    sizes = [len(table['tpcf_matrix']) for table in tables]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    return [slice(int(offsets[k]), int(offsets[k + 1])) for k in range(len(tables))]


def _setup(tables):
    return [vjp_reference.operands(table) for table in tables], [{} for _ in tables]


def vjp(tables, occupation, g, g_ngal=0.0, ops=None, caches=None):
    """ngal, xi (N), g_occupation (n_bins) and the scale (n_bins) of one draw; g is (N)."""
    if ops is None:
        ops, caches = _setup(tables)
    g = np.asarray(g, dtype=np.float64).ravel()
    parts = [vjp_reference.vjp(table, occupation, g[part], g_ngal if k == 0 else 0.0, ops[k],
                               caches[k])
             for k, (table, part) in enumerate(zip(tables, slices_of(tables)))]
    for part in parts[1:]:
        assert part[0] == parts[0][0]
    return (parts[0][0], np.concatenate([np.ravel(part[1]) for part in parts]),
            sum(part[2] for part in parts), sum(part[3] for part in parts))


def chi2_grad(tables, occupation, data, precision, ops=None, caches=None):
    """ngal, chi2, dchi2 / dn (n_bins), its scale (n_bins) and xi (N) of one draw.  In the scale
    |g_r| is replaced by 2 sum_s |P_sym,rs| (|xi_s| + |data_s|), as vjp_reference.chi2_grad."""
    if ops is None:
        ops, caches = _setup(tables)
    occupation = np.asarray(occupation, dtype=np.float64)
    terms = [vjp_reference._terms(table, occupation, ops[k], caches[k])
             for k, table in enumerate(tables)]
    n_h, ngal = terms[0][0], terms[0][1]
    xi = np.concatenate([np.ravel(term[2]) for term in terms])
    data = np.asarray(data, dtype=np.float64).ravel()
    precision = np.asarray(precision, dtype=np.float64)
    p_sym = 0.5 * (precision + precision.T)
    e = xi - data
    g = 2.0 * p_sym @ e
    g_abs = 2.0 * np.abs(p_sym) @ (np.abs(xi) + np.abs(data))
    dchi2, scale = np.zeros_like(n_h), np.zeros_like(n_h)
    for term, part in zip(terms, slices_of(tables)):
        assert term[1] == ngal
        _, _, _, jac, k = term
        dchi2 = dchi2 + n_h * (g[part] @ jac - k * (g[part] @ xi[part]) / ngal)
        scale = scale + n_h * (g_abs[part] @ np.abs(jac) +
                               k * (g_abs[part] @ np.abs(xi[part])) / ngal)
    return ngal, e @ precision @ e, dchi2, scale, xi


def vjp_batch(tables, occupation, g, g_ngal=None):
    """`vjp` draw by draw: ngal (n), xi (n, N), g_occupation and scale (n, n_bins)."""
    ops, caches = _setup(tables)
    with np.errstate(all='ignore'):
        results = [vjp(tables, occ, g[d], 0.0 if g_ngal is None else g_ngal[d], ops, caches)
                   for d, occ in enumerate(np.atleast_2d(occupation))]
    return tuple(np.array([r[i] for r in results]) for i in range(4))


def chi2_grad_batch(tables, occupation, data, precision):
    """`chi2_grad` draw by draw: ngal, chi2 (n), dchi2 and scale (n, n_bins), xi (n, N)."""
    ops, caches = _setup(tables)
    with np.errstate(all='ignore'):
        results = [chi2_grad(tables, occ, data, precision, ops, caches)
                   for occ in np.atleast_2d(occupation)]
    return tuple(np.array([r[i] for r in results]) for i in range(5))


def stacked(tables):
    """The one table of same-mode tables: their tpcf matrices concatenated along r."""
    assert len({table['attrs']['mode'] for table in tables}) == 1
    table = dict(tables[0])
    table['tpcf_matrix'] = np.concatenate(
        [np.asarray(t['tpcf_matrix'], dtype=np.float64) for t in tables], axis=0)
    table['tpcf_shape'] = (len(table['tpcf_matrix']), )
    return table
