"""Reference of a joint of tables that share one halo table: the per-table references
(`grad_reference.jacobian_batch`, `assembias_grad_reference.jacobian_batch`) concatenated in table
order, and chi2, its gradient and the Fisher matrix of the joint data vector in NumPy with P_sym
= (P + P^T) / 2.  A helper of the joint tests, not a test module.

Allowances are the existing ones with N = sum n_r for n_r, no new number: a derivative is allowed
RTOL |dxi| + RTOL scale with the scale of ITS table (a table's terms cancel among themselves), chi2
and dchi2 the formulas of test_gpu_grad.py (check_chi2_values), the Fisher matrix
`fisher_reference.allowance`.
"""

import numpy as np

import assembias_grad_reference
import fisher_reference
import grad_reference
from tabcorr_amd import synthetic

RTOL = 1e-10                         # the project's parity bar


def make_tables(n_prim, n_sec, parts, assembias=False):
    """The table dicts of a synthetic joint: `parts` = [(mode, tpcf_shape), ...], every table from
    synthetic_table(n_prim, n_sec, tpcf_shape, mode, seed=3) -- the same seed and bin counts give
    byte-identical gal_type tables --; an auto table behind the first auto one gets another matrix
    (synthetic_tpcf_matrix, seed=77 + its position).  `assembias`: the tables of
    assembias_grad_reference (a bin at the split sits at percentile 0.5 exactly)."""
    make = assembias_grad_reference.synthetic_table if assembias else synthetic.synthetic_table
    tables, seen = [], set()
    for position, (mode, shape) in enumerate(parts):
        table = make(n_prim, n_sec, tuple(shape), mode, seed=3)
        if mode in seen:
            table['tpcf_matrix'] = synthetic.synthetic_tpcf_matrix(
                len(table['gal_type']), int(np.prod(shape)), mode, seed=77 + position)
        seen.add(mode)
        tables.append(table)
    for table in tables[1:]:
        assert table['gal_type'].tobytes() == tables[0]['gal_type'].tobytes()
    return tables


def jacobian_batch(tables, theta, n_gauss_prim=10, modulate=False, assembias=False):
    """ngal (n), xi (n, N), dngal (n, Q), dxi (n, Q, N) and scale (n, Q, N): the per-k scale of
    every table, spread over its own r block."""
    module = assembias_grad_reference if assembias else grad_reference
    parts = [module.jacobian_batch(table, theta, n_gauss_prim, modulate) for table in tables]
    n = len(np.atleast_2d(theta))
    for part in parts[1:]:
        # one halo table: the tables' ngal and dngal are the same numbers
        assert np.array_equal(part[0], parts[0][0], equal_nan=True)
        assert np.array_equal(part[2], parts[0][2], equal_nan=True)
    xi = np.concatenate([part[1].reshape(n, -1) for part in parts], axis=1)
    dxi = np.concatenate([fisher_reference.flatten(part[3]) for part in parts], axis=2)
    scale = np.concatenate(
        [np.repeat(part[4][:, :, None], part[1].reshape(n, -1).shape[1], axis=2)
         for part in parts], axis=2)
    return parts[0][0], xi, parts[0][2], dxi, scale


def usable(reference):
    return grad_reference.usable(reference)


def check_derivatives(dngal, dxi, reference, what):
    """dngal (n, Q) and dxi (n, Q, N) against the reference of the first n draws."""
    n = len(dngal)
    _, _, dngal_ref, dxi_ref, scale = (a[:n] for a in reference)
    np.testing.assert_allclose(dngal, dngal_ref, rtol=RTOL,
                               atol=1e-14 * np.max(np.abs(dngal_ref)), err_msg=what)
    allowance = RTOL * np.abs(dxi_ref) + RTOL * scale
    error = np.abs(dxi - dxi_ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(error == 0.0, 0.0, error / allowance)
    print('%s: max |dxi - reference| / allowance = %.3g' % (what, np.max(ratio)))
    assert np.all(error <= allowance), (what, np.max(ratio))


def chi2_reference(reference, data, precision):
    """chi2 (n), dchi2 (n, Q) and their allowances (test_gpu_grad.py: check_chi2_values, with the
    per-row scale)."""
    _, xi, _, dxi, scale = reference
    p_sym = 0.5 * (precision + precision.T)
    e = xi - data
    v = 2.0 * e @ p_sym
    chi2 = np.einsum('nr,rs,ns->n', e, precision, e)
    dchi2 = np.einsum('nr,nkr->nk', v, dxi)
    chi2_allow = RTOL * np.abs(chi2) + RTOL * np.sum(np.abs(v) * np.abs(xi), axis=1)
    a_rk = RTOL * (np.abs(dxi) + scale)
    dchi2_allow = (RTOL * np.abs(dchi2) + np.einsum('nr,nkr->nk', np.abs(v), a_rk) +
                   2.0 * RTOL * np.einsum('nr,nkr->nk', np.abs(xi) @ np.abs(p_sym), np.abs(dxi)))
    return chi2, dchi2, chi2_allow, dchi2_allow


def check_chi2(chi2, dchi2, reference, data, precision, what):
    n = len(chi2)
    expect = chi2_reference(tuple(a[:n] for a in reference), data, precision)
    print('%s: max error / allowance = %.3g (chi2), %.3g (dchi2)' % (
        what, np.max(np.abs(chi2 - expect[0]) / expect[2]),
        np.max(np.abs(dchi2 - expect[1]) / np.maximum(expect[3], 1e-300))))
    assert np.all(np.abs(chi2 - expect[0]) <= expect[2]), what
    assert np.all(np.abs(dchi2 - expect[1]) <= expect[3]), what


def fisher_jacobian(reference):
    """dxi (n, Q, N) and its allowance a = 1e-10 (|dxi| + scale) for fisher_reference.check."""
    return reference[3], RTOL * (np.abs(reference[3]) + reference[4])


def coupled_data(xi, symmetric, in_units_of_xi=False):
    """A data vector near `xi` (one draw's joint vector) and a dense (N, N) precision matrix
    whose off-diagonal blocks couple the tables (derivative_kit.chi2_data).  in_units_of_xi: for
    tables whose scales differ by many orders of magnitude (w_p against DeltaSigma) the matrix is
    that of the data in units of |xi|, P = D^-1 P_0 D^-1 with D = diag(|xi|): every term of chi2
    is of order one, as with a real covariance."""
    from derivative_kit import chi2_data
    data, precision = chi2_data(xi, symmetric)
    if in_units_of_xi:
        inverse = 1.0 / np.abs(xi)
        precision = precision * inverse[:, None] * inverse[None, :]
    return data, precision
