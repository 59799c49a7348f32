"""Interpolator gradients without a GPU: the reference Jacobian of the tests against central
differences of the oracle in every theta and x column, the host helper tc_spline_weights (the
text the gradient kernels run for the spline weights) and the argument checks of the Python
layer."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference  # noqa: E402
import interp_grad_reference as reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def central_differences(tables, setup, theta, x, h, modulate):
    """d(ngal, xi)/d(theta, x) by central differences of the oracle's interpolator."""
    n_dim = len(x)
    dngal = np.zeros(5 + n_dim)
    dxi = []
    for k in range(5 + n_dim):
        e = np.zeros(5 + n_dim)
        e[k] = h
        a = oracle.interpolator_predict_zheng07_batch(
            tables, setup, theta + e[:5], x + e[5:], modulate_with_cenocc=modulate)
        b = oracle.interpolator_predict_zheng07_batch(
            tables, setup, theta - e[:5], x - e[5:], modulate_with_cenocc=modulate)
        dngal[k] = (a[0][0] - b[0][0]) / (2 * h)
        dxi.append((a[1][0] - b[1][0]) / (2 * h))
    return dngal, np.array(dxi)


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('grid,mode', [((4, ), 'auto'), ((4, 5), 'auto'), ((4, 5), 'cross')],
                         ids=['auto-4', 'auto-4x5', 'cross-4x5'])
def test_reference_jacobian_matches_central_differences(grid, mode, modulate):
    """|J - FD(h/2)| <= |FD(h) - FD(h/2)| + 8 eps S / (h/2), elementwise, the pattern of
    test_grad_cpu.py: the error of a central difference quarters with h, so the first term bounds
    it (the worst ratio is the expected 1/3); the second is the rounding noise of the differenced
    values.  For one table that noise is a few eps of max |f|.  An interpolated value is a sum
    over tables of cubic polynomials in the power basis, whose terms cancel (an axis around
    x = 1 with knots 0.1 apart: terms a hundred times the weight), so its noise is a few eps of
    S = sum_t |c_t| |f_t| with the absolute polynomial terms (ngal_scale / the largest xi_scale
    of the reference, never below max |f|); with max |f| in its place the ngal columns of the
    2-D grids miss by the factor of that cancellation.  logM0 sits midway between its
    neighbouring nodes and every x more than 4 h from the knots, so that no node crosses M0 and
    no knot lies inside the stencil."""
    tables, keys, points = synthetic.synthetic_interpolator(grid, 4, 1, (5, ), mode, seed=7)
    # two classes of halo tables: every other table has its own n_h
    for k, table in enumerate(tables):
        if k % 2:
            table['gal_type'] = table['gal_type'].copy()
            table['gal_type']['n_h'] *= 1.0 + 0.1 * k
    setup = oracle.interpolator_setup(tables, points)
    nodes = np.unique(np.concatenate([grad_reference.nodes_of(t) for t in tables]))
    thetas = grad_reference.centre_log_m0(synthetic.zheng07_draws(6, seed=5), nodes)
    rng = np.random.default_rng(3)
    low, high = points.min(axis=0), points.max(axis=0)
    h = 1e-4
    worst = 0.0
    for t in thetas:
        x = rng.uniform(low, high)
        assert np.min(np.abs(nodes - t[2])) > 4 * h
        for d, xp in enumerate(setup['xp']):
            assert np.min(np.abs(xp - x[d])) > 4 * h
        j = reference.jacobian(tables, setup, points, t, x, modulate=modulate)
        coarse = central_differences(tables, setup, t, x, h, modulate)
        fine = central_differences(tables, setup, t, x, h / 2, modulate)
        for analytic, f1, f2, size in (
                (j['dngal'], coarse[0], fine[0], j['ngal_scale']),
                (j['dxi'], coarse[1], fine[1], np.max(j['xi_scale']))):
            bound = np.abs(f1 - f2) + 8 * EPS * size / (h / 2)
            worst = max(worst, np.max(np.abs(analytic - f2) / bound))
            assert np.all(np.abs(analytic - f2) <= bound)
    print('worst |J - FD(h/2)| / bound:', worst)


def spline_weights(lib, xp, a, x):
    from tabcorr_amd import _lib
    xp, a = _lib.contiguous(xp), _lib.contiguous(a)
    weight, dweight = np.full(len(xp), np.nan), np.full(len(xp), np.nan)
    segment = ctypes.c_int(-7)
    _lib.check(lib.tc_spline_weights(len(xp), _lib.as_double_p(xp), _lib.as_double_p(a), x,
                                     _lib.as_double_p(weight), _lib.as_double_p(dweight),
                                     ctypes.byref(segment)))
    return weight, dweight, segment.value


AXES = [np.array([-0.5, -0.1, 0.2, 0.5]), np.linspace(0.8, 1.2, 5),
        np.array([0.0, 0.05, 0.2, 0.25, 0.31, 0.4, 0.62])]


@pytest.mark.parametrize('xp', AXES, ids=['4', '5', '7-uneven'])
def test_spline_weights_reproduce_the_oracle_and_differentiate_polynomials(lib, xp):
    """With the oracle's matrix: sum_j weight_j y_j is `oracle.spline_interpolate`, the derivative
    weights sum to zero (the weights sum to one at every x) and differentiate data on a line, a
    parabola and a cubic -- which the not-a-knot spline reproduces -- to p'(x), all to rounding:
    64 eps of sum_j |y_j| x the absolute polynomial terms of weight_j (four terms per weight and
    n weights per sum: a few eps of that scale each; the matrix's own error stays inside it)."""
    a = oracle.spline_interpolation_matrix(xp)
    rng = np.random.default_rng(len(xp))
    y = rng.normal(size=len(xp))
    inside = rng.uniform(xp[0], xp[-1], size=20)
    outside = [xp[0] - 0.3, xp[-1] + 0.2]
    polynomials = [np.array([0.3, -1.2]), np.array([0.3, -1.2, 0.7]),
                   np.array([0.3, -1.2, 0.7, 2.1])]          # coefficients, lowest first
    for x in list(inside) + list(xp) + outside:
        weight, dweight, _ = spline_weights(lib, xp, a, float(x))
        expect = oracle.spline_interpolate(x, xp, a, y, extrapolate=True)
        _, _, terms, dterms = reference.axis_terms(xp, a, float(x))
        assert abs(weight @ y - expect) <= 64 * EPS * (terms @ np.abs(y))
        assert abs(np.sum(weight) - 1.0) <= 64 * EPS * np.sum(terms)
        assert abs(np.sum(dweight)) <= 64 * EPS * np.sum(dterms)
        for c in polynomials:
            values = np.polynomial.polynomial.polyval(xp, c)
            slope = np.polynomial.polynomial.polyval(x, np.polynomial.polynomial.polyder(c))
            assert abs(dweight @ values - slope) <= 64 * EPS * (dterms @ np.abs(values))
            assert abs(weight @ values - np.polynomial.polynomial.polyval(x, c)) <= \
                64 * EPS * (terms @ np.abs(values))


@pytest.mark.parametrize('xp', AXES, ids=['4', '5', '7-uneven'])
def test_spline_weights_segment_rule(lib, xp):
    """np.digitize(x, xp) - 1 with the last knot in the last segment, clamped on both sides."""
    a = oracle.spline_interpolation_matrix(xp)
    n = len(xp)
    cases = [(xp[0], 0), (xp[1], 1), (xp[n - 2], n - 2), (xp[-1], n - 2),
             (xp[0] - 1.0, 0), (xp[-1] + 1.0, n - 2), (0.5 * (xp[1] + xp[2]), 1),
             (np.nextafter(xp[1], -np.inf), 0), (np.nextafter(xp[-1], -np.inf), n - 2)]
    for x, segment in cases:
        weight, dweight, got = spline_weights(lib, xp, a, float(x))
        assert got == segment, (x, got, segment)
        # ... and the weights are that segment's polynomial
        powers = float(x)**np.arange(4)
        assert np.allclose(weight, a[segment].T @ powers, rtol=0, atol=64 * EPS * np.max(
            np.abs(a[segment]).T @ np.abs(powers)))
    # on a knot the weights pick that node: a property of the MATRIX (the oracle's numerical
    # inverse, good to the parity bar of 1e-10), not of the evaluation checked above
    for i in range(n):
        weight, _, _ = spline_weights(lib, xp, a, float(xp[i]))
        expect = np.zeros(n)
        expect[i] = 1.0
        segment = min(i, n - 2)
        terms = np.abs(a[segment]).T @ np.abs(float(xp[i])**np.arange(4))
        assert np.all(np.abs(weight - expect) <= 1e-10 * terms)


def make_interpolator(grid=(4, 5), tpcf_shape=(5, )):
    from tabcorr_amd import Interpolator, TabCorr
    tables, keys, points = synthetic.synthetic_interpolator(grid, 4, 1, tpcf_shape, 'auto', seed=7)
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
                for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)}), points


@pytest.mark.parametrize('tpcf_shape', [(5, ), (3, 4)])
def test_gradient_calls_reject_wrong_arguments_before_any_device_is_touched(tpcf_shape):
    interp, points = make_interpolator(tpcf_shape=tpcf_shape)
    n_r = int(np.prod(tpcf_shape))
    theta = synthetic.zheng07_draws(3, seed=2)
    x = np.tile(points.mean(axis=0), (3, 1))
    data, precision = np.zeros(tpcf_shape), np.eye(n_r)

    def both(theta, x, **kwargs):
        with pytest.raises(ValueError):
            interp.predict_batch_grad(theta, x, **kwargs)
        with pytest.raises(ValueError):
            interp.chi2_grad_batch(theta, x, data, precision, **kwargs)

    for columns in (7, 4):                       # the assembly-bias layout, a short one
        both(np.zeros((3, columns)), x)
    both(theta, x[:2])                           # one row of x missing
    both(theta, x[:, :1])                        # one column of x missing
    both(theta, np.hstack([x, x[:, :1]]))        # one column too many
    for d in range(2):                           # outside the grid, on either side
        for value in (points[:, d].min() - 0.01, points[:, d].max() + 0.01, np.nan):
            outside = x.copy()
            outside[1, d] = value
            both(theta, outside)
            with pytest.raises(ValueError, match='extrapolation'):
                interp.predict_batch_grad(theta, outside, extrapolate=False)
    for bad_data, bad_precision in ((np.zeros(n_r + 1), precision), (np.zeros(n_r - 1), precision),
                                    (np.zeros((n_r, 2)), precision), (data, np.eye(n_r + 1)),
                                    (data, np.ones((n_r, n_r + 1))), (data, np.ones(n_r * n_r))):
        with pytest.raises(ValueError, match='precision'):
            interp.chi2_grad_batch(theta, x, bad_data, bad_precision)
    assert interp._device is None
    assert all(halotab._device is None for halotab in interp.tabcorr_list)


def test_predict_grad_needs_a_plain_zheng07_model():
    """Anything but a plain Zheng07 model is a NotImplementedError of `predict_grad`, and a
    missing extra parameter a ValueError, before any device is touched."""
    from tabcorr_amd import Zheng07Model
    interp, points = make_interpolator()
    model = Zheng07Model(redshift=0.0)
    with pytest.raises(ValueError, match='log_eta'):
        interp.predict_grad(model, check_consistency=False)
    for d, key in enumerate(interp.keys):
        model.param_dict[key] = points[:, d].mean()
    biased = Zheng07Model(redshift=0.0, sec_haloprop_key='halo_nfw_conc')
    biased.param_dict.update(model.param_dict)
    with pytest.raises(NotImplementedError):
        interp.predict_grad(biased, check_consistency=False)
    assert interp._device is None


def test_c_entry_points_refuse_a_call_without_a_handle(lib):
    from tabcorr_amd import _lib
    empty = np.zeros(0)
    theta = synthetic.zheng07_draws(3, seed=2)
    p = _lib.as_double_p
    status = lib.tc_interp_predict_grad_zheng07_batch(
        None, p(theta), 5, p(empty), 3, 10, 0, p(empty), p(empty), p(empty), p(empty))
    assert status == _lib.TC_ERR_INVALID
    status = lib.tc_interp_chi2_grad_zheng07_batch(
        None, p(theta), 5, p(empty), 3, 10, 0, *[p(empty)] * 6)
    assert status == _lib.TC_ERR_INVALID
    assert lib.tc_interp_predict_grad_zheng07_batch_device(
        None, None, 5, None, 3, 10, 0, None, None, None, None) == _lib.TC_ERR_INVALID
    assert lib.tc_interp_chi2_grad_zheng07_batch_device(
        None, None, 5, None, 3, 10, 0, p(empty), p(empty), None, None, None,
        None) == _lib.TC_ERR_INVALID
