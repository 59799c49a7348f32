"""Leauthaud11 gradients without a GPU: the eleven-column reference Jacobian of the tests against
finite differences of the oracle, the host build of the kernels' node arithmetic against the NumPy
derivatives, the new symbols, the family's LDS budget of grad.h, the argument checks of the
Python layer and `Leauthaud11Model.device_jacobian`."""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import leauthaud11_grad_reference as reference  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 1e-4

ENTRIES = ['tc_predict_grad_leauthaud11_batch', 'tc_predict_grad_leauthaud11_batch_device',
           'tc_chi2_grad_leauthaud11_batch', 'tc_chi2_grad_leauthaud11_batch_device']


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def central_differences(table, theta, h, modulate):
    dngal = np.zeros(11)
    dxi = []
    for k in range(11):
        e = np.zeros(14)
        e[k] = h
        a = reference.predict(table, theta + e, modulate=modulate)
        b = reference.predict(table, theta - e, modulate=modulate)
        dngal[k] = (a[0] - b[0]) / (2 * h)
        dxi.append((a[1] - b[1]) / (2 * h))
    return dngal, np.array(dxi)


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('mode', ['auto', 'cross'])
def test_reference_jacobian_matches_central_differences(mode, modulate):
    """|J - FD(h/2)| <= |FD(h) - FD(h/2)| + 8 eps max|f| / (h/2), elementwise, for all eleven
    columns of dngal and dxi: the bound of test_grad_cpu.py, no free tolerance.  Six draws of the
    box; the occupation is smooth, so no draw has to keep clear of anything.  Every draw has
    galaxies and a finite reference."""
    table = synthetic.synthetic_table(9, 1, (5, ), mode, seed=3)
    thetas = reference.leauthaud11_draws(6, 5)
    h = STEP
    worst = 0.0
    for t in thetas:
        ngal, xi, dngal, dxi, scale = reference.jacobian(table, t, modulate=modulate)
        assert ngal > 0.0 and all(np.all(np.isfinite(a)) for a in (xi, dngal, dxi, scale))
        coarse = central_differences(table, t, h, modulate)
        fine = central_differences(table, t, h / 2, modulate)
        for analytic, f1, f2, value in ((dngal, coarse[0], fine[0], ngal),
                                        (dxi, coarse[1], fine[1], xi)):
            bound = np.abs(f1 - f2) + 8 * EPS * np.max(np.abs(value)) / (h / 2)
            worst = max(worst, np.max(np.abs(analytic - f2) / bound))
            assert np.all(np.abs(analytic - f2) <= bound)
    print('worst |J - FD(h/2)| / bound:', worst)


def test_stress_draws_have_galaxies_and_a_finite_reference():
    table = synthetic.synthetic_table(9, 1, (5, ), 'auto', seed=3)
    theta = reference.stress_draws(8, seed=5)
    assert theta[0, 5] == 0.03 and theta[2, 10] == 0.0 and theta[5, 11] == 11.4
    assert theta[1, 9] == pytest.approx(0.97) and theta[3, 6] == 0.8 and theta[4, 6] == 1.2
    for modulate in (False, True):
        assert reference.usable(reference.jacobian_batch(table, theta, modulate=modulate))


def host_node_grad(lib, theta, modulate, mass):
    from tabcorr_amd import _lib
    n = len(mass)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    mass = np.ascontiguousarray(mass, dtype=np.float64)
    out = [np.empty(n), np.empty(n), np.empty((n, 11)), np.empty(n), np.empty((n, 11))]
    _lib.check(lib.tc_debug_leauthaud11_node_grad(
        _lib.as_double_p(theta), int(modulate), n, _lib.as_double_p(mass),
        *[_lib.as_double_p(a) for a in out]))
    return out


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
def test_host_node_routine_matches_the_numpy_derivatives(lib, modulate):
    """The host build of the kernels' node routine (the Newton root, N_cen, N_sat and all eleven
    derivatives of each) against the NumPy derivatives of the reference at 41 masses over
    10^10.5 .. 10^15.5, for the centre draw and the stress draws.  Allowance: 1e-12 of the
    column's largest magnitude, the bar test_half_erfc_from_the_gaussian_on_host sets for the host
    math."""
    mass = 10.0**np.linspace(10.5, 15.5, 41)
    draws = np.vstack([reference.CENTRE, reference.stress_draws(6, seed=5)])
    worst = 0.0
    for t in draws:
        log_mstar, n_cen, dn_cen, n_sat, dn_sat = host_node_grad(lib, t, modulate, mass)
        expect_cen, expect_dcen = reference.centrals(mass, t)
        expect_sat, expect_dsat = reference.satellites(mass, t, modulate)
        from oracle import tabcorr_oracle as oracle
        pairs = [(log_mstar, oracle.behroozi10_log_stellar_mass(np.log10(mass), t)),
                 (n_cen, expect_cen), (n_sat, expect_sat)]
        pairs += [(dn_cen[:, k], expect_dcen[k]) for k in range(11)]
        pairs += [(dn_sat[:, k], expect_dsat[k]) for k in range(11)]
        for got, expect in pairs:
            assert np.all(np.isfinite(expect))
            size = np.max(np.abs(expect))
            if size == 0.0:
                assert np.all(got == 0.0)
                continue
            worst = max(worst, np.max(np.abs(got - expect)) / (1e-12 * size))
            assert np.all(np.abs(got - expect) <= 1e-12 * size)
    print('worst host node error in units of 1e-12 of the column:', worst)


def test_the_four_entry_points_are_declared_listed_and_exported(lib):
    from tabcorr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tabcorr_amd.h')).read()
    declared = set(re.findall(r'^int (tc_\w+)\(', header, flags=re.M))
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    # the argument lists are those of the assembly-bias four
    for name in ENTRIES:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace('leauthaud11', 'assembias')]
    # the first argument is the handle: without one every entry refuses before reading the rest
    for name in ENTRIES:
        scalars = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint)
        status = getattr(lib, name)(*[0 if kind in scalars else None
                                      for kind in _lib.SIGNATURES[name]])
        assert status == _lib.TC_ERR_INVALID


# grad.h, restated in rows of 16 doubles.  Leauthaud11: a central bin keeps 7 rows (w and its six
# non-zero derivatives), a satellite bin 12, one row of zeros, 12 totals, 12 n_r stash rows for
# the likelihood; mode cross 12 slabs of 64 bins, 12 n_r products and the totals.
def restated_rows(kernel, n_bins, n_central, n_r, chi2):
    auto_rows = 7 * n_central + 12 * (n_bins - n_central) + 1
    return [auto_rows + 12 + (12 * n_r if chi2 else 0), 12 * (64 + n_r) + 12][kernel]


def test_lds_formulas(lib):
    from tabcorr_amd import _lib
    for n_bins, n_central, n_r, n_dim in ((4, 2, 1, 1), (36, 18, 5, 2), (100, 50, 19, 3),
                                          (201, 100, 40, 8), (7, 7, 3, 0)):
        for kernel in range(2):
            for chi2 in (0, 1):
                got = ctypes.c_int64(-1)
                _lib.check(lib.tc_debug_grad_lds(kernel, 11, n_bins, n_central, n_r, n_dim, chi2,
                                                 ctypes.byref(got)))
                assert got.value == 16 * 8 * restated_rows(kernel, n_bins, n_central, n_r, chi2)
    # the benchmark's 50 + 50 bins and 19 r bins: 123 KB, 152 KB with the likelihood, of 160 KB
    assert 16 * 8 * restated_rows(0, 100, 50, 19, 0) == 123264
    assert 16 * 8 * restated_rows(0, 100, 50, 19, 1) == 152448 <= 160 * 1024
    bad = ctypes.c_int64(-1)
    assert lib.tc_debug_grad_lds(0, 6, 4, 2, 1, 0, 0, ctypes.byref(bad)) == _lib.TC_ERR_INVALID
    # the interpolator kernels have no instance of the family
    for kernel in (2, 3):
        assert lib.tc_debug_grad_lds(kernel, 11, 4, 2, 1, 1, 0,
                                     ctypes.byref(bad)) == _lib.TC_ERR_INVALID


def test_gradient_calls_reject_wrong_arguments_before_any_device():
    from tabcorr_amd import TabCorr
    table = synthetic.synthetic_table(7, 2, (5, ), 'auto', seed=3)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                  table['tpcf_shape'], table['attrs'])
    data, precision = np.zeros(5), np.eye(5)
    family = 'leauthaud11'
    for columns in (5, 11, 13, 15):
        theta = np.zeros((3, columns))
        with pytest.raises(ValueError, match='theta'):
            halotab.predict_batch_grad(theta, family=family)
        with pytest.raises(ValueError, match='theta'):
            halotab.chi2_grad_batch(theta, data, precision, family=family)
        with pytest.raises(ValueError, match='theta'):
            halotab.chi2_fisher_batch(theta, data, precision, family=family)
        with pytest.raises(ValueError, match='theta'):
            halotab.fisher_batch(theta, precision, family=family)
    # fourteen columns are not a Zheng07 draw
    with pytest.raises(ValueError, match='theta'):
        halotab.predict_batch_grad(np.zeros((3, 14)))
    theta = reference.leauthaud11_draws(3, 5)
    for bad_data, bad_precision in ((np.zeros(4), precision), (data, np.eye(4)),
                                    (data, np.zeros((5, 4)))):
        with pytest.raises(ValueError, match='precision'):
            halotab.chi2_grad_batch(theta, bad_data, bad_precision, family=family)
        with pytest.raises(ValueError, match='precision'):
            halotab.chi2_fisher_batch(theta, bad_data, bad_precision, family=family)
        if bad_precision.shape != precision.shape:
            with pytest.raises(ValueError, match='precision'):
                halotab.fisher_batch(theta, bad_precision, family=family)
    # the family has no assembly bias
    with pytest.raises(ValueError, match='assembias'):
        halotab.predict_batch_grad(theta, assembias=True, family=family)
    with pytest.raises(ValueError, match='assembias'):
        halotab.chi2_grad_batch(theta, data, precision, assembias=True, family=family)
    with pytest.raises(ValueError, match='assembias'):
        halotab.chi2_fisher_batch(theta, data, precision, assembias=True, family=family)
    with pytest.raises(ValueError, match='assembias'):
        halotab.fisher_batch(theta, precision, assembias=True, family=family)
    with pytest.raises(ValueError, match='family'):
        halotab.predict_batch_grad(theta, family='zheng08')
    assert halotab._device is None


@pytest.mark.parametrize('redshift', [0.0, 0.5])
def test_device_jacobian_is_the_derivative_of_device_theta(redshift):
    """`Leauthaud11Model.device_jacobian()` (11, 16) against the exact derivative of
    `device_theta()`, which is linear in param_dict: a difference quotient with step 1 has no
    truncation error, and (a - 1) is formed as the model forms it."""
    from tabcorr_amd import Leauthaud11Model
    from tabcorr_amd.models import LEAUTHAUD11_GRAD_KEYS, LEAUTHAUD11_KEYS
    assert LEAUTHAUD11_GRAD_KEYS == ('logm0', 'logm1', 'beta', 'delta', 'gamma', 'scatter',
                                     'alphasat', 'bsat', 'betasat', 'bcut', 'betacut')
    assert len(LEAUTHAUD11_GRAD_KEYS) == 11 and len(LEAUTHAUD11_KEYS) == 16
    model = Leauthaud11Model(threshold=10.8, redshift=redshift)
    # exactly representable parameters: the difference quotient below is then exact
    for j, key in enumerate(LEAUTHAUD11_KEYS):
        model.param_dict[key] = float(j + 1)
    jacobian = model.device_jacobian()
    assert jacobian.shape == (11, 16)
    base = model.device_theta()
    a = 1.0 / (1.0 + redshift)
    for j, key in enumerate(LEAUTHAUD11_KEYS):
        model.param_dict[key] += 1.0
        moved = model.device_theta()
        model.param_dict[key] -= 1.0
        assert np.all(moved[11:] == base[11:])
        np.testing.assert_allclose(jacobian[:, j], (moved - base)[:11], rtol=0, atol=64 * EPS)
    # the theta columns the keys name: the relation's five, then the six that stand for themselves
    for k in range(5):
        assert jacobian[k, 2 * k] == 1.0 and jacobian[k, 2 * k + 1] == a - 1.0
    assert np.array_equal(jacobian[5:, 10:], np.eye(6))
    assert np.count_nonzero(jacobian) == (16 if redshift else 11)
