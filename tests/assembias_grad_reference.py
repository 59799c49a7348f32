"""Reference Jacobian of (ngal, xi) with respect to the seven parameters of Zheng07 decorated with
Heaviside assembly bias at the median split (`ZHENG07_KEYS + ASSEMBIAS_KEYS`), in NumPy from the
oracle's own pieces, built the way grad_reference.py is.  A helper of the assembly-bias gradient
tests, not a test module.

With c(A) the clip of a strength to [-1, 1], c'(A) = 1 for |A| <= 1 and 0 beyond, and s_b = +1 for
a bin whose sec_haloprop_percentile lies above 0.5, else -1, per quadrature node:
  centrals    N' = N + s_b c(A_cen) min(N, 1 - N), min(N, 1 - N) = erfc(|x|) / 2; with tau = +1
              where N <= 1 - N, else -1:
              dN'/dtheta_k = (1 + s_b c(A_cen) tau) dN/dtheta_k, dN'/dA_cen = s_b c'(A_cen) min(N, 1 - N)
  satellites  N' = (1 + s_b c(A_sat)) N (N after modulate_with_cenocc, with the PLAIN <N_cen>):
              dN'/dtheta_k = (1 + s_b c(A_sat)) dN/dtheta_k, dN'/dA_sat = s_b c'(A_sat) N
The values themselves come from `oracle.Zheng07(theta[:5], modulate, assembias=theta[5:])`.
"""

import math

import numpy as np

import grad_reference
import interp_grad_reference
from oracle import tabcorr_oracle as oracle

try:
    from scipy.special import erfc as _erfc
except ImportError:  # pragma: no cover
    _erfc = np.vectorize(math.erfc, otypes=[np.float64])

N_PARAMS = 7
STEP = 1e-4                          # the finite-difference step the draws keep clear of the nodes

# (A_cen, A_sat) of the first draws: none, inside the clip, exactly at it, beyond it (the column
# is exactly zero), and A_sat = -1 with A_cen inside (the satellites above the split vanish, their
# A_sat column does not)
STRENGTHS = np.array([[0.0, 0.0], [0.5, -0.5], [-0.5, 0.5], [1.0, 1.0], [-1.0, -1.0],
                      [1.7, -1.7], [-1.7, 1.7], [0.3, -1.0]])


def synthetic_table(n_prim, n_sec, tpcf_shape, mode, seed=3):
    """`synthetic.synthetic_table` whose middle secondary bin, where there is one, sits at
    percentile EXACTLY 0.5 (the synthetic one is the mean of two rounded edges, an ulp off): a bin
    at the split itself is below it."""
    from tabcorr_amd import synthetic
    table = synthetic.synthetic_table(n_prim, n_sec, tpcf_shape, mode, seed=seed)
    percentile = table['gal_type']['sec_haloprop_percentile']
    percentile[np.abs(percentile - 0.5) < 1e-9] = 0.5
    return table


def clip(a):
    return min(max(a, -1.0), 1.0)


def clip_slope(a):
    return 1.0 if abs(a) <= 1.0 else 0.0


def side(percentile):
    return np.where(np.asarray(percentile) > 0.5, 1.0, -1.0)


class Derivative:
    """d<N'>/dtheta_k of the decorated occupations at the nodes, k = 0 .. 6, with the callbacks'
    signature of ``tabcorr/tabcorr.py:556-563``."""

    def __init__(self, theta, k, modulate):
        self.t, self.k, self.modulate = np.asarray(theta, float), k, modulate
        self.plain = grad_reference.Derivative(self.t[:5], k, modulate)

    def mean_occupation_centrals(self, prim_haloprop, sec_haloprop_percentile=None):
        m = np.asarray(prim_haloprop, float)
        s = side(sec_haloprop_percentile)
        n = oracle.zheng07_centrals(m, self.t)
        if self.k == 5:
            # min(N, 1 - N) = erfc(|x|) / 2, from erfc: np.minimum(n, 1 - n) carries the absolute
            # rounding of n (1e-16), which is 1e-8 of it at |x| = 4, and a draw with a narrow
            # sigma_logM makes this column of such terms alone
            x = (np.log10(m) - self.t[0]) / self.t[1]
            return s * clip_slope(self.t[5]) * 0.5 * _erfc(np.abs(x))
        tau = np.where(n <= 1.0 - n, 1.0, -1.0)
        return (1.0 + s * clip(self.t[5]) * tau) * self.plain.centrals(m)

    def mean_occupation_satellites(self, prim_haloprop, sec_haloprop_percentile=None):
        m = np.asarray(prim_haloprop, float)
        s = side(sec_haloprop_percentile)
        if self.k == 5:
            return np.zeros_like(m)
        if self.k == 6:
            return s * clip_slope(self.t[6]) * oracle.zheng07_satellites(m, self.t, self.modulate)
        return (1.0 + s * clip(self.t[6])) * self.plain.mean_occupation_satellites(m)


def model(theta, modulate=False):
    return oracle.Zheng07(theta[:5], modulate, assembias=theta[5:])


def jacobian(table, theta, n_gauss_prim=10, modulate=False):
    """ngal, xi, dngal (7), dxi (7, ) + tpcf_shape and the per-(k) absolute scale of the terms of
    dxi that cancel, as `grad_reference.jacobian` has it."""
    theta = np.asarray(theta, float)
    occ = oracle.mean_occupation(table, model(theta, modulate), n_gauss_prim)
    n_h = table['gal_type']['n_h']
    w = occ * n_h
    ngal, xi = oracle.predict(table, occ)
    matrix = table['tpcf_matrix']
    auto = table['attrs']['mode'] == 'auto'
    if auto:
        i1, i2, prefactor = oracle.pair_indices(len(w))
    dngal = np.zeros(N_PARAMS)
    dxi = np.zeros((N_PARAMS, ) + xi.shape)
    scale = np.zeros(N_PARAMS)
    flat = xi.ravel()
    for k in range(N_PARAMS):
        dw = oracle.mean_occupation(table, Derivative(theta, k, modulate), n_gauss_prim) * n_h
        dngal[k] = dw.sum()
        if auto:
            dq = matrix @ (prefactor * (dw[i1] * w[i2] + w[i1] * dw[i2]))
            dxi[k] = (dq / ngal**2 - 2 * flat * dngal[k] / ngal).reshape(xi.shape)
            scale[k] = np.max(np.abs(dq) / ngal**2 + 2 * np.abs(flat * dngal[k]) / ngal)
        else:
            product = matrix @ dw
            dxi[k] = ((product - flat * dngal[k]) / ngal).reshape(xi.shape)
            scale[k] = np.max(np.abs(product) + np.abs(flat * dngal[k])) / ngal
    return ngal, xi, dngal, dxi, scale


def jacobian_batch(table, theta, n_gauss_prim=10, modulate=False):
    results = [jacobian(table, t, n_gauss_prim, modulate) for t in np.atleast_2d(theta)]
    return tuple(np.array([r[i] for r in results]) for i in range(5))


usable = grad_reference.usable


def rounding_of_centrals(compute, dxi, allowance):
    """How far the reference's own rounding carries into dxi, in units of `allowance`: `compute()`
    (which returns dxi again) runs with every `oracle.zheng07_centrals` value moved by half an
    ulp of 1 (1.1e-16, the rounding of 1 + erf) up or down.  <N_cen> far below logMmin is small
    against that absolute error -- 1e-8 of it at x = -4 -- and with modulate_with_cenocc it
    multiplies every satellite term: where the satellites' columns consist of such terms alone
    (one mass bin, one node, a narrow sigma_logM) the function itself, in NumPy as on the device,
    is known to fewer digits than the parity bar asks, and a comparison at that bar says nothing.
    The suites draw their batches so that this stays below a tenth of the allowance."""
    original = oracle.zheng07_centrals
    rng = np.random.default_rng(1)

    def moved(prim_haloprop, theta):
        n = original(prim_haloprop, theta)
        return n + 1.1e-16 * rng.choice([-1.0, 1.0], size=np.shape(n))

    oracle.zheng07_centrals = moved
    try:
        with np.errstate(all='ignore'):
            again = compute()
    finally:
        oracle.zheng07_centrals = original
    error = np.abs(again - dxi)
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.max(np.where(error == 0.0, 0.0, error / allowance)))


def well_conditioned(table, theta, expect, n_gauss_prim=10, modulate=False):
    """Whether `rounding_of_centrals` of a `jacobian_batch` result stays below a tenth of the
    allowance 1e-10 (|dxi| + scale)."""
    dxi, scale = expect[3], expect[4]
    allowance = 1e-10 * (np.abs(dxi) + scale.reshape(scale.shape + (1, ) * (dxi.ndim - 2)))
    return rounding_of_centrals(
        lambda: jacobian_batch(table, theta, n_gauss_prim, modulate)[3], dxi, allowance) <= 0.1


def clear_of_nodes(theta, nodes, column):
    """Moves every draw's `column` that lies inside the node range to the midpoint between its
    two neighbouring nodes (in place), as `grad_reference.centre_log_m0` does for logM0: the
    decorated <N_cen> has a kink where it crosses 1/2 at a node, i.e. where logMmin crosses one."""
    for t in theta:
        if nodes[0] < t[column] < nodes[-1]:
            j = np.searchsorted(nodes, t[column])
            t[column] = 0.5 * (nodes[j - 1] + nodes[j])
        # (outside the node range, or a table of one node: a value that fell next to the end
        # node steps off it)
        nearest = nodes[np.argmin(np.abs(nodes - t[column]))]
        if abs(t[column] - nearest) <= 4 * STEP:
            t[column] = nearest + 8 * STEP
    return theta


def stress_draws(table, n_draws, seed=5, n_gauss_prim=10):
    """(n_draws, 7): the rows of `grad_reference.stress_draws` (logM0 at node midpoints) with
    logMmin at node midpoints too -- more than 4 STEP from every node -- and the strengths of
    STRENGTHS in the first rows, uniform in (-1, 1) behind them."""
    plain = grad_reference.stress_draws(table, n_draws, seed=seed, n_gauss_prim=n_gauss_prim)
    nodes = grad_reference.nodes_of(table, n_gauss_prim)
    clear_of_nodes(plain, nodes, 0)
    assert np.min(np.abs(nodes[None, :] - plain[:, :1])) > 4 * STEP
    rng = np.random.default_rng(seed + 100)
    strengths = np.vstack([STRENGTHS, rng.uniform(-1.0, 1.0, size=(max(n_draws, 1), 2))])
    # (a batch of fewer draws than STRENGTHS has rows takes them in turn by its seed)
    if n_draws < len(STRENGTHS):
        strengths = np.roll(strengths[:len(STRENGTHS)], -(seed % len(STRENGTHS)), axis=0)
    return np.ascontiguousarray(np.hstack([plain, strengths[:n_draws]]))


def unclipped(theta):
    """The draws whose two strengths lie strictly inside (-1, 1): where the function is smooth in
    them."""
    return np.all(np.abs(np.atleast_2d(theta)[:, 5:]) < 1.0, axis=1)


# ---- interpolator: the spline-weighted sum of the table references -------------------------------

def interp_jacobian(tables, setup, points, theta, x, n_gauss_prim=10, modulate=False):
    """Of one draw (theta (7), x (D)), the dict of `interp_grad_reference.jacobian` with 7 + D
    columns."""
    per_table = [jacobian(table, theta, n_gauss_prim, modulate) for table in tables]
    ngal_t = np.array([r[0] for r in per_table])
    xi_t = np.array([r[1] for r in per_table])
    dngal_t = np.array([r[2] for r in per_table])
    dxi_t = np.array([r[3] for r in per_table])
    scale_t = np.array([r[4] for r in per_table])
    c, dc, abs_c, abs_dc = interp_grad_reference.table_weights(setup, points, x)
    ones = (1, ) * (xi_t.ndim - 1)
    return {
        'ngal': c @ ngal_t,
        'xi': np.tensordot(c, xi_t, 1),
        'dngal': np.concatenate([c @ dngal_t, dc @ ngal_t]),
        'dxi': np.concatenate([np.tensordot(c, dxi_t, 1), np.tensordot(dc, xi_t, 1)]),
        'ngal_scale': abs_c @ np.abs(ngal_t),
        'xi_scale': np.tensordot(abs_c, np.abs(xi_t), 1),
        'dngal_scale': np.concatenate([abs_c @ np.abs(dngal_t), abs_dc @ np.abs(ngal_t)]),
        'dxi_scale': np.concatenate([
            (abs_c @ scale_t).reshape((N_PARAMS, ) + ones) * np.ones(xi_t.shape[1:]),
            np.tensordot(abs_dc, np.abs(xi_t), 1)]),
    }


def interp_jacobian_batch(tables, setup, points, theta, x, n_gauss_prim=10, modulate=False):
    results = [interp_jacobian(tables, setup, points, t, xv, n_gauss_prim, modulate)
               for t, xv in zip(np.atleast_2d(theta), np.atleast_2d(x))]
    return {key: np.array([r[key] for r in results]) for key in results[0]}
