"""Reference Jacobian of (ngal, xi) with respect to the five Zheng07 parameters, in NumPy from
the oracle's own pieces.  A helper of the gradient tests, not a test module.

``oracle.mean_occupation`` is called with duck models whose callbacks return the per-node
derivatives, which keeps the identical quadrature (the bin average is linear in the node values);
``oracle.predict`` / ``oracle.pair_indices`` and the chain rule follow.
"""

import math

import numpy as np

from oracle import tabcorr_oracle as oracle
from tabcorr_amd import synthetic

LN10 = math.log(10.0)


class Derivative:
    """d<N>/dtheta_k of the Zheng07 occupations at the nodes, with the callbacks'
    signature of ``tabcorr/tabcorr.py:556-563``."""

    def __init__(self, theta, k, modulate):
        self.t, self.k, self.modulate = np.asarray(theta, float), k, modulate

    def centrals(self, m):
        t = self.t
        x = (np.log10(m) - t[0]) / t[1]
        g = np.exp(-x * x) / (t[1] * math.sqrt(math.pi))
        return {0: -g, 1: -x * g}.get(self.k, np.zeros_like(m))

    def mean_occupation_centrals(self, prim_haloprop, sec_haloprop_percentile=None):
        return self.centrals(np.asarray(prim_haloprop, float))

    def mean_occupation_satellites(self, prim_haloprop, sec_haloprop_percentile=None):
        t = self.t
        m = np.asarray(prim_haloprop, float)
        m0, m1 = 10**t[2], 10**t[3]
        out = np.zeros_like(m)
        use = m - m0 > 0
        s = (m[use] - m0) / m1
        n = s**t[4]
        out[use] = {2: -t[4] * s**(t[4] - 1) * m0 * LN10 / m1, 3: -t[4] * LN10 * n,
                    4: n * np.log(s)}.get(self.k, np.zeros_like(s))
        if self.modulate:
            out = (out * oracle.zheng07_centrals(m, t) +
                   oracle.zheng07_satellites(m, t, False) * self.centrals(m))
        return out


def jacobian(table, theta, n_gauss_prim=10, modulate=False):
    """ngal, xi, dngal (5), dxi (5, ) + tpcf_shape and the per-(k) absolute scale of the terms
    of dxi that cancel: max_r(|dq_k| / ngal^2 + 2 |xi_r dngal_k| / ngal) in mode auto,
    max_r(|T_r . dw_k| + |xi_r dngal_k|) / ngal in mode cross."""
    occ = oracle.mean_occupation(table, oracle.Zheng07(theta, modulate), n_gauss_prim)
    n_h = table['gal_type']['n_h']
    w = occ * n_h
    ngal, xi = oracle.predict(table, occ)
    matrix = table['tpcf_matrix']
    auto = table['attrs']['mode'] == 'auto'
    if auto:
        i1, i2, prefactor = oracle.pair_indices(len(w))
    dngal = np.zeros(5)
    dxi = np.zeros((5, ) + xi.shape)
    scale = np.zeros(5)
    flat = xi.ravel()
    for k in range(5):
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


def usable(reference):
    """Whether every draw of a `jacobian_batch` result has galaxies and all of it is finite."""
    return bool(np.all(reference[0] > 0.0) and all(np.all(np.isfinite(a)) for a in reference))


def nodes_of(table, n_gauss_prim=10):
    """Sorted log10 masses of every quadrature node of the table (tabcorr.py:543-549)."""
    gal_type = table['gal_type']
    x = (np.polynomial.legendre.leggauss(n_gauss_prim)[0] + 1) / 2
    low = gal_type['log_prim_haloprop_min'][:, None]
    width = (gal_type['log_prim_haloprop_max'] - gal_type['log_prim_haloprop_min'])[:, None]
    return np.unique((low + width * x).ravel())


def centre_log_m0(theta, nodes):
    """Moves every draw's logM0 that lies inside the node range to the midpoint between its two
    neighbouring nodes (in place): <N_sat> has a kink wherever M0 crosses a node."""
    for t in theta:
        if nodes[0] < t[2] < nodes[-1]:
            j = np.searchsorted(nodes, t[2])
            t[2] = 0.5 * (nodes[j - 1] + nodes[j])
    return theta


def stress_draws(table, n_draws, seed=5, n_gauss_prim=10):
    """Draws from the uniform prior box whose first rows stress the kernel's branches: a narrow
    sigma_logM, logM0 above the top bin edge (no satellites at all: their derivatives are exactly
    zero) and below the lowest one, alpha at both ends of the box; logM0 otherwise at node
    midpoints."""
    theta = synthetic.zheng07_draws(max(n_draws, 5), seed=seed)
    gal_type = table['gal_type']
    theta[0, 1] = 0.02
    theta[1, 2] = gal_type['log_prim_haloprop_max'].max() + 0.3
    theta[2, 2] = gal_type['log_prim_haloprop_min'].min() - 0.3
    theta[3, 4] = 0.7
    theta[4, 4] = 1.4
    # (a batch of fewer than five draws takes the stress rows in turn by its seed)
    theta = np.roll(theta, -(seed % 5), axis=0)[:n_draws] if n_draws < 5 else theta
    return centre_log_m0(theta, nodes_of(table, n_gauss_prim))
