"""Reference vector-Jacobian product of ``predict(occupation)`` with respect to the occupation
array, in NumPy from the oracle's own pieces.  A helper of the VJP tests, not a test module.

With ``w = n n_h``, ``ngal = sum_i w_i`` and the cotangents ``g_ngal`` (scalar), ``g_r`` (``n_r``):

mode auto   ``q_r = w^T S_r w`` (``S_r`` the full symmetric matrix, no pair prefactor),
            ``xi_r = q_r / ngal^2``, ``U_r = S_r w``,
            ``g_n,i = n_h,i [g_ngal + (2 / ngal^2) sum_r g_r U_ri - (2 / ngal) sum_r g_r xi_r]``
mode cross  ``xi_r = T_r . w / ngal``,
            ``g_n,i = n_h,i [g_ngal + (1 / ngal) sum_r g_r T_ri - (1 / ngal) sum_r g_r xi_r]``

``ngal`` and ``xi`` are ``oracle.predict``'s.  Next to every result comes, per element, the
absolute scale of the terms that cancel in it.  Everything is in the row order of ``gal_type``.
"""

import numpy as np

from oracle import tabcorr_oracle as oracle


def operands(table):
    """(S, None) in mode auto -- S (n_r, n_bins, n_bins) symmetric, from the packed matrix
    through ``oracle.pair_indices`` -- or (None, T) in mode cross, T (n_r, n_bins)."""
    matrix = np.asarray(table['tpcf_matrix'], dtype=np.float64)
    if table['attrs']['mode'] != 'auto':
        return None, matrix
    n_bins = len(table['gal_type'])
    i1, i2, _ = oracle.pair_indices(n_bins)
    dense = np.zeros((len(matrix), n_bins, n_bins))
    dense[:, i1, i2] = matrix
    dense[:, i2, i1] = matrix
    return dense, None


def _terms(table, occupation, ops, cache=None):
    """ngal, xi (flat) and J_ri with d xi_r / d n_i = n_h,i (J_ri - xi_r k / ngal), k = 2 (auto)
    or 1 (cross): J = 2 U / ngal^2 or T / ngal."""
    n_h = np.asarray(table['gal_type']['n_h'], dtype=np.float64)
    ngal, xi = oracle.predict(table, occupation, cache=cache)
    dense, cross = ops if ops is not None else operands(table)
    w = occupation * n_h
    if dense is not None:
        return n_h, ngal, xi, 2.0 * (dense @ w) / ngal**2, 2.0
    return n_h, ngal, xi, cross / ngal, 1.0


def vjp(table, occupation, g_xi, g_ngal=0.0, ops=None, cache=None):
    """ngal, xi, g_occupation (n_bins) and the scale (n_bins) of one draw.  `ops`: `operands`
    of the table, `cache`: the pair cache of `oracle.predict`, for a batch of calls."""
    n_h, ngal, xi, jac, k = _terms(table, np.asarray(occupation, dtype=np.float64), ops, cache)
    g = np.asarray(g_xi, dtype=np.float64).ravel()
    flat = xi.ravel()
    g_occupation = n_h * (g_ngal + g @ jac - k * (g @ flat) / ngal)
    scale = n_h * (abs(g_ngal) + np.abs(g) @ np.abs(jac) + k * (np.abs(g) @ np.abs(flat)) / ngal)
    return ngal, xi, g_occupation, scale


def chi2_grad(table, occupation, data, precision, ops=None, cache=None):
    """ngal, chi2, dchi2 / dn (n_bins), its scale (n_bins) and xi of one draw: the VJP with
    g = 2 P_sym (xi - data), P_sym = (precision + precision^T) / 2, and g_ngal = 0.  In the scale
    |g_r| is replaced by 2 sum_s |P_sym,rs| (|xi_s| + |data_s|)."""
    n_h, ngal, xi, jac, k = _terms(table, np.asarray(occupation, dtype=np.float64), ops, cache)
    data = np.asarray(data, dtype=np.float64).ravel()
    precision = np.asarray(precision, dtype=np.float64)
    p_sym = 0.5 * (precision + precision.T)
    flat = xi.ravel()
    e = flat - data
    g = 2.0 * p_sym @ e
    g_abs = 2.0 * np.abs(p_sym) @ (np.abs(flat) + np.abs(data))
    dchi2 = n_h * (g @ jac - k * (g @ flat) / ngal)
    scale = n_h * (g_abs @ np.abs(jac) + k * (g_abs @ np.abs(flat)) / ngal)
    return ngal, e @ precision @ e, dchi2, scale, xi


def vjp_batch(table, occupation, g_xi, g_ngal=None):
    """`vjp` draw by draw: ngal (n), xi (n, ) + tpcf_shape, g_occupation and scale (n, n_bins)."""
    ops, cache = operands(table), {}
    occupation = np.atleast_2d(occupation)
    with np.errstate(all='ignore'):
        results = [vjp(table, occ, g_xi[d], 0.0 if g_ngal is None else g_ngal[d], ops, cache)
                   for d, occ in enumerate(occupation)]
    return tuple(np.array([r[i] for r in results]) for i in range(4))


def chi2_grad_batch(table, occupation, data, precision):
    """`chi2_grad` draw by draw: ngal, chi2 (n), dchi2 and scale (n, n_bins), xi."""
    ops, cache = operands(table), {}
    with np.errstate(all='ignore'):
        results = [chi2_grad(table, occ, data, precision, ops, cache)
                   for occ in np.atleast_2d(occupation)]
    return tuple(np.array([r[i] for r in results]) for i in range(5))
