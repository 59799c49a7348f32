"""Reference Jacobian of an interpolator's (ngal, xi) with respect to (theta, x): the five Zheng07
parameters and the D extra parameters, in NumPy from `grad_reference.jacobian` per table,
`oracle.interpolator_setup` and its spline matrices.  A helper of the interpolator gradient tests,
not a test module.

The interpolated result is linear in the per-table results: with c_t(x) the tensor-product weight
of table t, d/dtheta_k = sum_t c_t d(.)_t/dtheta_k and d/dx_d = sum_t (dc_t/dx_d) (.)_t, where
dc_t/dx_d differentiates the one cubic factor of axis d.
"""

import contextlib

import numpy as np

import grad_reference
from oracle import tabcorr_oracle as oracle

RTOL = 1e-10


def axis_terms(xp, a, x):
    """Weights and derivative weights of the nodes of one axis at x (segment as
    `oracle.spline_interpolate`, clamped), and the sums of the absolute values of their
    polynomial terms: the size of what cancels in the power-basis evaluation."""
    n = len(xp)
    segment = int(np.digitize(x, xp)) - 1
    if x == xp[-1]:
        segment = n - 2
    segment = min(max(segment, 0), n - 2)
    m = a[segment]                                           # (4, n)
    powers = x**np.arange(4)
    slopes = np.array([0.0, 1.0, 2.0 * x, 3.0 * x * x])
    return (m.T @ powers, m.T @ slopes, np.abs(m).T @ np.abs(powers),
            np.abs(m).T @ np.abs(slopes))


def table_weights(setup, points, x):
    """c_t (K) and dc_t/dx_d (D, K) of every table (rows of `points`) at x, and the same from
    the sums of absolute polynomial terms."""
    points = np.asarray(points, dtype=np.float64).reshape(len(points), -1)
    n_dim = points.shape[1]
    terms = [axis_terms(setup['xp'][d], setup['a'][d], x[d]) for d in range(n_dim)]
    nodes = [np.searchsorted(setup['xp'][d], points[:, d]) for d in range(n_dim)]

    def products(value, slope):
        c = np.prod([terms[d][value][nodes[d]] for d in range(n_dim)], axis=0)
        dc = np.array([np.prod([terms[e][slope if e == d else value][nodes[e]]
                                for e in range(n_dim)], axis=0) for d in range(n_dim)])
        return c, dc

    return products(0, 1) + products(2, 3)


@contextlib.contextmanager
def occupations_once_per_class(tables, setup):
    """While active, `oracle.mean_occupation` (through which `grad_reference.jacobian` gets the
    occupations and their derivatives) is evaluated once per class of identical halo tables and
    model, as the interpolator does (interpolator.py:181-184)."""
    class_of = {id(table): int(setup['unique_inverse'][k]) for k, table in enumerate(tables)}
    original = oracle.mean_occupation
    cache = {}

    def cached(table, model, n_gauss_prim=10):
        key = (class_of[id(table)], type(model).__name__, getattr(model, 'k', None), n_gauss_prim)
        if key not in cache:
            cache[key] = original(table, model, n_gauss_prim)
        return cache[key]

    oracle.mean_occupation = cached
    try:
        yield cache
    finally:
        oracle.mean_occupation = original


def jacobian(tables, setup, points, theta, x, n_gauss_prim=10, modulate=False):
    """Of one draw (theta (5), x (D)), as a dict: ngal, xi (tpcf_shape), dngal (5 + D), dxi
    (5 + D, ) + tpcf_shape, and per entry the absolute scale of the terms that cancel in it --
    ngal_scale, xi_scale: sum_t |c_t| |(ngal_t, xi_t)|; dngal_scale, dxi_scale: theta columns
    sum_t |c_t| (|dngal_{t,k}|, scale_{t,k} of `grad_reference.jacobian`), x columns
    sum_t |dc_t/dx_d| |(ngal_t, xi_{t,r})| -- with |c_t| and |dc_t| taken as the product of the
    sums of absolute polynomial terms."""
    with occupations_once_per_class(tables, setup) as cache:
        per_table = []
        for table in tables:
            per_table.append(grad_reference.jacobian(table, theta, n_gauss_prim, modulate))
        cache.clear()
    ngal_t = np.array([r[0] for r in per_table])             # (K)
    xi_t = np.array([r[1] for r in per_table])               # (K, ) + shape
    dngal_t = np.array([r[2] for r in per_table])            # (K, 5)
    dxi_t = np.array([r[3] for r in per_table])              # (K, 5) + shape
    scale_t = np.array([r[4] for r in per_table])            # (K, 5)
    c, dc, abs_c, abs_dc = table_weights(setup, points, x)
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
            (abs_c @ scale_t).reshape((5, ) + ones) * np.ones(xi_t.shape[1:]),
            np.tensordot(abs_dc, np.abs(xi_t), 1)]),
    }


def jacobian_batch(tables, setup, points, theta, x, n_gauss_prim=10, modulate=False):
    results = [jacobian(tables, setup, points, t, xv, n_gauss_prim, modulate)
               for t, xv in zip(np.atleast_2d(theta), np.atleast_2d(x))]
    return {key: np.array([r[key] for r in results]) for key in results[0]}


def usable(reference):
    """Whether all of a `jacobian_batch` result is finite: every table has galaxies in every
    draw (an interpolated ngal itself may have either sign outside the grid)."""
    return all(bool(np.all(np.isfinite(a))) for a in reference.values())


def first(reference, n):
    return {key: value[:n] for key, value in reference.items()}


def check(got, reference, what):
    """ngal, xi, dngal, dxi against the reference: |error| <= 1e-10 |reference| + 1e-10 scale,
    the gradient suite's allowance.  Prints the largest error in units of the allowance."""
    worst = 0.0
    for name, value in zip(('ngal', 'xi', 'dngal', 'dxi'), got):
        expect = reference[name]
        assert value.shape == expect.shape, (what, name, value.shape, expect.shape)
        allowance = RTOL * np.abs(expect) + RTOL * reference[name + '_scale']
        error = np.abs(value - expect)
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(error == 0.0, 0.0, error / allowance)
        worst = max(worst, float(np.max(ratio)))
        assert np.all(error <= allowance), (what, name, float(np.max(ratio)))
    print('%s: max |error| / allowance = %.3g' % (what, worst))
    return worst
