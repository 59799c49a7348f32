"""Assembly-bias gradients without a GPU: the seven-column reference Jacobian of the tests against
finite differences of the oracle, the argument checks of the Python layer, the new symbols and
the decorated LDS budget of grad.h."""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assembias_grad_reference as reference  # noqa: E402
import grad_reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ['tc_predict_grad_assembias_batch', 'tc_predict_grad_assembias_batch_device',
           'tc_chi2_grad_assembias_batch', 'tc_chi2_grad_assembias_batch_device',
           'tc_interp_predict_grad_assembias_batch',
           'tc_interp_predict_grad_assembias_batch_device',
           'tc_interp_chi2_grad_assembias_batch', 'tc_interp_chi2_grad_assembias_batch_device']


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def central_differences(table, theta, h, modulate):
    dngal = np.zeros(7)
    dxi = []
    for k in range(7):
        e = np.zeros(7)
        e[k] = h
        a = oracle.predict(table, oracle.mean_occupation(table, reference.model(theta + e, modulate)))
        b = oracle.predict(table, oracle.mean_occupation(table, reference.model(theta - e, modulate)))
        dngal[k] = (a[0] - b[0]) / (2 * h)
        dxi.append((a[1] - b[1]) / (2 * h))
    return dngal, np.array(dxi)


@pytest.mark.parametrize('n_sec', [1, 2, 3])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('mode', ['auto', 'cross'])
def test_reference_jacobian_matches_central_differences(mode, modulate, n_sec):
    """|J - FD(h/2)| <= |FD(h) - FD(h/2)| + 8 eps max|f| / (h/2), elementwise, for all seven
    columns: the bound of test_grad_cpu.py, no free tolerance.  logM0 and logMmin sit midway
    between their neighbouring nodes, more than 4 h from both, so that no node crosses M0 or the
    point <N_cen> = 1/2 inside the stencil.  Draws with a strength at or beyond the clip are not
    differenced (the function has a kink at +-1): beyond it their column is asserted exactly
    zero.  Every draw has galaxies and a finite reference."""
    table = reference.synthetic_table(9, n_sec, (5, ), mode, seed=3)
    if n_sec != 2:
        assert np.sum(table['gal_type']['sec_haloprop_percentile'] == 0.5) == 18
    nodes = grad_reference.nodes_of(table)
    thetas = reference.stress_draws(table, 14, seed=5)
    smooth = reference.unclipped(thetas)
    assert smooth.sum() >= 8 and (~smooth).sum() >= 5
    h = reference.STEP
    worst = 0.0
    for t, differenced in zip(thetas, smooth):
        assert np.min(np.abs(nodes - t[2])) > 4 * h or not nodes[0] < t[2] < nodes[-1]
        assert np.min(np.abs(nodes - t[0])) > 4 * h
        ngal, xi, dngal, dxi, scale = reference.jacobian(table, t, modulate=modulate)
        assert ngal > 0.0 and all(np.all(np.isfinite(a)) for a in (xi, dngal, dxi, scale))
        for k in (5, 6):
            if abs(t[k]) > 1.0:
                assert dngal[k] == 0.0 and np.all(dxi[k] == 0.0)
        if not differenced:
            continue
        coarse = central_differences(table, t, h, modulate)
        fine = central_differences(table, t, h / 2, modulate)
        for analytic, f1, f2, value in ((dngal, coarse[0], fine[0], ngal),
                                        (dxi, coarse[1], fine[1], xi)):
            bound = np.abs(f1 - f2) + 8 * EPS * np.max(np.abs(value)) / (h / 2)
            worst = max(worst, np.max(np.abs(analytic - f2) / bound))
            assert np.all(np.abs(analytic - f2) <= bound)
    print('worst |J - FD(h/2)| / bound:', worst)


def test_reference_values_are_the_oracles_and_one_secondary_bin_is_below():
    """The reference's ngal and xi are `oracle.predict_zheng07(..., assembias=...)`; in a table
    with one secondary bin (percentile 0.5) every bin is below the split: a positive A_sat lowers
    every satellite bin."""
    table = synthetic.synthetic_table(9, 1, (5, ), 'auto', seed=3)
    theta = reference.stress_draws(table, 9, seed=5)
    for t in theta:
        ngal, xi, dngal, _, _ = reference.jacobian(table, t)
        expect = oracle.predict_zheng07(table, t[:5], assembias=t[5:])
        assert ngal == expect[0] and np.array_equal(xi, expect[1])
        assert dngal[6] <= 0.0


def test_gradient_calls_reject_a_wrong_theta_shape_before_any_device():
    from tabcorr_amd import Interpolator, TabCorr, Zheng07Model
    table = synthetic.synthetic_table(7, 2, (5, ), 'auto', seed=3)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                  table['tpcf_shape'], table['attrs'])
    data, precision = np.zeros(5), np.eye(5)
    for assembias, columns in ((True, 5), (True, 8), (False, 7)):
        theta = np.zeros((3, columns))
        with pytest.raises(ValueError, match='theta'):
            halotab.predict_batch_grad(theta, assembias=assembias)
        with pytest.raises(ValueError, match='theta'):
            halotab.chi2_grad_batch(theta, data, precision, assembias=assembias)
        with pytest.raises(ValueError, match='theta'):
            halotab.chi2_fisher_batch(theta, data, precision, assembias=assembias)
        with pytest.raises(ValueError, match='theta'):
            halotab.fisher_batch(theta, precision, assembias=assembias)
    # a plain model with assembias=True
    model = Zheng07Model(redshift=0.0)
    with pytest.raises(ValueError, match='decorated'):
        halotab.predict_grad(model, check_consistency=False, assembias=True)
    with pytest.raises(ValueError, match='decorated'):
        halotab.fisher(model, precision, check_consistency=False, assembias=True)
    assert halotab._device is None

    tables, keys, points = synthetic.synthetic_interpolator((4, ), 7, 2, (5, ), 'auto', seed=3)
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
                for t in tables]
    interpolator = Interpolator(halotabs, {keys[0]: points[:, 0]})
    x = np.zeros((3, 1))
    for assembias, columns in ((True, 5), (True, 8), (False, 7)):
        theta = np.zeros((3, columns))
        with pytest.raises(ValueError, match='theta'):
            interpolator.predict_batch_grad(theta, x, assembias=assembias)
        with pytest.raises(ValueError, match='theta'):
            interpolator.chi2_grad_batch(theta, x, data, precision, assembias=assembias)
        with pytest.raises(ValueError, match='theta'):
            interpolator.chi2_fisher_batch(theta, x, data, precision, assembias=assembias)
        with pytest.raises(ValueError, match='theta'):
            interpolator.fisher_batch(theta, x, precision, assembias=assembias)
    model.param_dict[keys[0]] = 0.0
    with pytest.raises(ValueError, match='decorated'):
        interpolator.predict_grad(model, check_consistency=False, assembias=True)
    with pytest.raises(ValueError, match='decorated'):
        interpolator.fisher(model, precision, check_consistency=False, assembias=True)
    assert interpolator._device is None and all(h._device is None for h in halotabs)


def test_seven_key_tuple():
    from tabcorr_amd import models
    assert models.ZHENG07_ASSEMBIAS_KEYS == models.ZHENG07_KEYS + models.ASSEMBIAS_KEYS
    assert len(models.ZHENG07_ASSEMBIAS_KEYS) == 7


def test_the_eight_entry_points_are_declared_listed_and_exported(lib):
    from tabcorr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tabcorr_amd.h')).read()
    declared = set(re.findall(r'^int (tc_\w+)\(', header, flags=re.M))
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    # the first argument is the handle: without one every entry refuses before reading the rest
    for name in ENTRIES:
        scalars = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint)
        status = getattr(lib, name)(*[0 if kind in scalars else None
                                      for kind in _lib.SIGNATURES[name]])
        assert status == _lib.TC_ERR_INVALID


# grad.h, restated in rows of 16 doubles.  Decorated: a central bin keeps 4 rows (w and the
# derivatives by logMmin, sigma_logM, A_cen), a satellite bin 7 (w, the five Zheng07 derivatives,
# the one by A_sat), one row of zeros, 8 totals, 8 n_r stash rows for the likelihood; mode cross 8
# slabs of 64 bins, 8 n_r products and the totals; an interpolator the weights and derivative
# weights of D axes of up to 32 nodes and 8 + D accumulators per r bin, its mode cross another
# 8 + D products per r bin for the class in flight.
def restated_rows(kernel, n_params, n_bins, n_central, n_r, n_dim, chi2):
    n_q = n_params + 1
    central, satellite = (3, 6) if n_params == 5 else (4, 7)
    auto_rows = central * n_central + satellite * (n_bins - n_central) + 1
    common = 2 * n_dim * 32 + (n_q + n_dim) * n_r
    return [auto_rows + n_q + (n_q * n_r if chi2 else 0),
            n_q * 64 + n_q * n_r + n_q,
            auto_rows + n_q + common,
            n_q * 64 + n_q + (n_q + n_dim) * n_r + common][kernel]


@pytest.mark.parametrize('n_params', [5, 7])
def test_lds_formulas(lib, n_params):
    from tabcorr_amd import _lib
    for n_bins, n_central, n_r, n_dim in ((4, 2, 1, 1), (36, 18, 5, 2), (100, 50, 19, 3),
                                          (201, 100, 40, 8), (7, 7, 3, 0)):
        for kernel in range(4):
            for chi2 in (0, 1):
                got = ctypes.c_int64(-1)
                _lib.check(lib.tc_debug_grad_lds(kernel, n_params, n_bins, n_central, n_r, n_dim,
                                                 chi2, ctypes.byref(got)))
                assert got.value == 16 * 8 * restated_rows(kernel, n_params, n_bins, n_central,
                                                           n_r, n_dim, chi2)
    bad = ctypes.c_int64(-1)
    assert lib.tc_debug_grad_lds(0, 6, 4, 2, 1, 0, 0, ctypes.byref(bad)) == _lib.TC_ERR_INVALID


def test_half_erfc_from_the_gaussian_on_host(lib):
    """min(N, 1 - N) = erfc(|x|) / 2 as the kernels form it for the A_cen column from |x| = 2.5
    on (fastmath.h: half_erfc_from_gauss, a degree-14 fit good to 4e-14, times the table-driven
    Gaussian, good to a few 1e-16 relative) against scipy's erfc: 1e-12 relative, a hundredth of
    the parity bar, down to where it underflows; and at |x| = 2.5, where the kernels switch to
    it, fmin(n, 1 - n) with its absolute 1e-16 is as good."""
    from scipy.special import erf, erfc
    from tabcorr_amd import _lib
    x = np.concatenate([np.linspace(2.5, 6.0, 20001), np.linspace(6.0, 26.0, 20001),
                        -np.linspace(2.5, 26.0, 1001), [2.5, 6.0, 1e3, np.inf]])
    out = np.empty_like(x)
    _lib.check(lib.tc_debug_fastmath(7, x.size, _lib.as_double_p(x), _lib.as_double_p(out)))
    expect = 0.5 * erfc(np.abs(x))
    normal = expect > 1e-300
    assert np.max(np.abs(out[normal] / expect[normal] - 1.0)) < 1e-12
    assert np.all(out[~normal] <= 1e-300) and np.all(out >= 0.0)
    n = 0.5 * (1.0 + erf(2.5))
    assert abs(min(n, 1.0 - n) / (0.5 * erfc(2.5)) - 1.0) < 1e-12
