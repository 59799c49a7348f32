"""The occupation VJP without a GPU: the reference VJP of the tests against finite differences of
the oracle, the four new symbols of the C ABI, and the argument checks of the Python layer."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vjp_reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

EPS = np.finfo(np.float64).eps
NEW_SYMBOLS = ['tc_predict_occupation_vjp_batch', 'tc_predict_occupation_vjp_batch_device',
               'tc_chi2_occupation_grad_batch', 'tc_chi2_occupation_grad_batch_device']


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def central_differences(table, occupation, h):
    """d ngal / d n_i (n_bins) and d xi / d n_i (n_bins, n_r) by central differences of
    `oracle.predict` in single occupation entries."""
    dngal, dxi = [], []
    for i in range(len(occupation)):
        e = np.zeros(len(occupation))
        e[i] = h
        a = oracle.predict(table, occupation + e)
        b = oracle.predict(table, occupation - e)
        dngal.append((a[0] - b[0]) / (2 * h))
        dxi.append(((a[1] - b[1]) / (2 * h)).ravel())
    return np.array(dngal), np.array(dxi)


def occupations(table, n_draws, seed):
    """Zheng07 occupations and random positive ones with entries exactly zero, in turn."""
    rng = np.random.default_rng(seed)
    n_bins = len(table['gal_type'])
    out = []
    for d, theta in enumerate(synthetic.zheng07_draws(n_draws, seed=seed)):
        if d % 2 == 0:
            out.append(oracle.mean_occupation(table, oracle.Zheng07(theta)))
        else:
            occ = rng.uniform(0.1, 2.0, size=n_bins)
            occ[rng.choice(n_bins, size=2, replace=False)] = 0.0
            out.append(occ)
    return out


@pytest.mark.parametrize('shape', [(7, 1, (5, )), (3, 2, (3, 4))],
                         ids=['7x1-5', '3x2-3x4'])
@pytest.mark.parametrize('mode', ['auto', 'cross'])
def test_reference_vjp_matches_central_differences(mode, shape):
    """The rows of the Jacobian that the reference VJP gives for unit cotangents (one r at a
    time, then g_ngal = 1 alone) against central differences in single occupation entries:
    |J - FD(h/2)| <= |FD(h) - FD(h/2)| + 8 eps max|f| / (h/2), elementwise -- the error of a
    central difference quarters with h, so the right-hand side bounds it; no free tolerance.
    (ngal, xi) are rational in the occupations: there are no kinks to avoid."""
    table = synthetic.synthetic_table(shape[0], shape[1], shape[2], mode, seed=3)
    n_r = int(np.prod(shape[2]))
    n_h = table['gal_type']['n_h']
    h = 1e-3
    worst = 0.0
    for occupation in occupations(table, 4, seed=5):
        ngal, xi = oracle.predict(table, occupation)
        assert ngal > 0.0
        coarse = central_differences(table, occupation, h)
        fine = central_differences(table, occupation, h / 2)
        got_ngal, got_xi, row, _ = vjp_reference.vjp(table, occupation, np.zeros(shape[2]), 1.0)
        assert got_ngal == ngal and np.array_equal(got_xi, xi)
        # the bare n_h
        np.testing.assert_allclose(row, n_h, rtol=4 * EPS)
        jac = np.empty((len(occupation), n_r))
        for r in range(n_r):
            unit = np.zeros(n_r)
            unit[r] = 1.0
            jac[:, r] = vjp_reference.vjp(table, occupation, unit.reshape(shape[2]))[2]
        for analytic, f1, f2, value in ((row, coarse[0], fine[0], ngal),
                                        (jac, coarse[1], fine[1], xi)):
            bound = np.abs(f1 - f2) + 8 * EPS * np.max(np.abs(value)) / (h / 2)
            worst = max(worst, np.max(np.abs(analytic - f2) / bound))
            assert np.all(np.abs(analytic - f2) <= bound)
        # a random cotangent is the same linear combination of those rows
        rng = np.random.default_rng(7)
        g_xi, g_ngal = rng.normal(size=n_r), rng.normal()
        combined, scale = vjp_reference.vjp(table, occupation, g_xi.reshape(shape[2]), g_ngal)[2:]
        assert np.all(np.abs(combined - (g_ngal * row + jac @ g_xi)) <= 16 * EPS * scale)
    print('worst |J - FD(h/2)| / bound:', worst)


@pytest.mark.parametrize('mode', ['auto', 'cross'])
def test_reference_chi2_gradient_is_the_vjp_of_its_cotangent(mode):
    """chi2_grad = vjp with g = 2 P_sym (xi - data) and g_ngal = 0 (a non-symmetric precision
    pins the P_sym convention), and its chi2 is e^T P e."""
    table = synthetic.synthetic_table(3, 2, (3, 4), mode, seed=3)
    rng = np.random.default_rng(11)
    precision = np.eye(12) * 12 + rng.normal(size=(12, 12))
    for occupation in occupations(table, 2, seed=5):
        xi = oracle.predict(table, occupation)[1]
        data = xi * (1.0 + 0.05 * rng.normal(size=xi.shape))
        ngal, chi2, dchi2, scale, _ = vjp_reference.chi2_grad(table, occupation, data, precision)
        e = (xi - data).ravel()
        assert chi2 == e @ precision @ e
        g = (precision + precision.T) @ e
        expect = vjp_reference.vjp(table, occupation, g.reshape(xi.shape))
        assert ngal == expect[0]
        assert np.all(np.abs(dchi2 - expect[2]) <= 16 * EPS * scale)
        assert np.all(scale >= expect[3] * (1 - 16 * EPS))


def test_library_exports_the_four_vjp_symbols(lib):
    """Declared in the header, present in the ctypes table and exported by the library."""
    from tabcorr_amd import _lib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    declared = entry.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES['tc_predict_occupation_vjp_batch']) == 9
    assert len(_lib.SIGNATURES['tc_chi2_occupation_grad_batch']) == 9


def test_vjp_calls_reject_wrong_shapes_without_a_device():
    """The occupation columns, g_xi, g_ngal, data and precision: a ValueError of `predict_vjp` /
    `chi2_grad_occupation` before any device is touched, with tpcf_shape of one axis and two."""
    from tabcorr_amd import TabCorr
    for tpcf_shape in ((5, ), (3, 4)):
        table = synthetic.synthetic_table(7, 1, tpcf_shape, 'auto', seed=3)
        halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                      table['tpcf_shape'], table['attrs'])
        n_bins, n_r = len(table['gal_type']), int(np.prod(tpcf_shape))
        good = np.ones((3, n_bins))
        good_g = np.zeros((3, ) + tpcf_shape)
        good_data, good_precision = np.zeros(tpcf_shape), np.eye(n_r)
        for occupation in (np.ones((3, n_bins + 1)), np.ones((3, n_bins - 1)),
                           np.ones(n_bins + 1), np.ones((3, n_bins, 1))):
            with pytest.raises(ValueError, match='occupation'):
                halotab.predict_vjp(occupation, good_g)
            with pytest.raises(ValueError, match='occupation'):
                halotab.chi2_grad_occupation(occupation, good_data, good_precision)
        for g_xi in (np.zeros((2, ) + tpcf_shape), np.zeros((3, n_r + 1)), np.zeros(tpcf_shape),
                     np.zeros((3, ) + tpcf_shape + (1, )), np.zeros((3, n_r, n_r))):
            with pytest.raises(ValueError, match='g_xi'):
                halotab.predict_vjp(good, g_xi)
        # un-batched: g_xi has the bare tpcf_shape
        with pytest.raises(ValueError, match='g_xi'):
            halotab.predict_vjp(good[0], good_g)
        for g_ngal in (np.zeros(2), np.zeros((3, 1)), 1.0):
            with pytest.raises(ValueError, match='g_ngal'):
                halotab.predict_vjp(good, good_g, g_ngal)
        for data, precision in ((np.zeros(n_r + 1), good_precision),
                                (np.zeros(n_r - 1), good_precision),
                                (np.zeros((n_r, 2)), good_precision),
                                (good_data, np.eye(n_r + 1)),
                                (good_data, np.ones((n_r, n_r + 1))),
                                (good_data, np.ones(n_r * n_r)),
                                (good_data, np.ones((n_r, n_r, 1)))):
            with pytest.raises(ValueError, match='precision'):
                halotab.chi2_grad_occupation(good, data, precision)
        assert halotab._device is None


def test_vjp_entry_points_refuse_a_null_handle(lib):
    """All four C entry points refuse a call without a handle before they read anything else."""
    from tabcorr_amd import _lib
    empty = _lib.as_double_p(np.zeros(0))
    calls = [lib.tc_predict_occupation_vjp_batch(None, empty, 3, 0, None, empty, empty, empty,
                                                 empty),
             lib.tc_predict_occupation_vjp_batch_device(None, None, 3, 0, None, None, None, None,
                                                        None),
             lib.tc_chi2_occupation_grad_batch(None, empty, 3, 0, empty, empty, empty, empty,
                                               empty),
             lib.tc_chi2_occupation_grad_batch_device(None, None, 3, 0, empty, empty, None, None,
                                                      None)]
    for status in calls:
        assert status == _lib.TC_ERR_INVALID
        with pytest.raises(ValueError):
            _lib.check(status)
