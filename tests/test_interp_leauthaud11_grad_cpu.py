"""The interpolator's Leauthaud11 gradients without a GPU: the reference Jacobian over (11, D) of
the tests against central differences of the oracle's interpolated Leauthaud11 prediction, the new
symbols, the LDS budget of the family behind its debug entry (the cross kernel's slab of 32 bins),
the shapes that must be served and refused, and the argument checks of the Python layer."""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interp_leauthaud11_grad_reference as reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from test_leauthaud11_grad_cpu import STEP  # noqa: E402

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = ROOT
LDS_LIMIT = 160 * 1024
AUTO, CROSS = 0, 1

ENTRIES = ['tc_interp_predict_grad_leauthaud11_batch',
           'tc_interp_predict_grad_leauthaud11_batch_device',
           'tc_interp_chi2_grad_leauthaud11_batch',
           'tc_interp_chi2_grad_leauthaud11_batch_device']


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def two_classes(tables):
    """Every other table's n_h times 1.2: two classes of halo tables, interleaved."""
    for k, table in enumerate(tables):
        if k % 2:
            table['gal_type'] = table['gal_type'].copy()
            table['gal_type']['n_h'] *= 1.2
    return tables


def central_differences(tables, setup, theta, x, h, modulate):
    """d(ngal, xi)/d(theta_0 .. theta_10, x) by central differences of the oracle's interpolator."""
    n_dim = len(x)
    dngal = np.zeros(11 + n_dim)
    dxi = []
    for k in range(11 + n_dim):
        e = np.zeros(14 + n_dim)
        e[k if k < 11 else k + 3] = h
        a = reference.predict(tables, setup, theta + e[:14], x + e[14:], modulate=modulate)
        b = reference.predict(tables, setup, theta - e[:14], x - e[14:], modulate=modulate)
        dngal[k] = (a[0] - b[0]) / (2 * h)
        dxi.append((a[1] - b[1]) / (2 * h))
    return dngal, np.array(dxi)


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_prim,mode', [(7, 'auto'), (18, 'cross')], ids=['auto-7', 'cross-18'])
def test_reference_jacobian_matches_central_differences(n_prim, mode, modulate):
    """|J - FD(h/2)| <= |FD(h) - FD(h/2)| + 8 eps max|f| / (h/2), elementwise, for the eleven theta
    columns and the x column of dngal and dxi: the step and the bound of
    test_leauthaud11_grad_cpu.py, no free tolerance.  The six stress draws; the occupation is
    smooth and a grid of four nodes is ONE cubic (not-a-knot), so no draw and no x has to keep
    clear of anything.  Every draw has galaxies in every table and a finite reference."""
    tables, keys, points = synthetic.synthetic_interpolator((4, ), n_prim, 1, (5, ), mode, seed=7)
    tables = two_classes(tables)
    setup = oracle.interpolator_setup(tables, points)
    assert len(np.unique(setup['unique_inverse'])) == 2
    thetas = reference.draws(6)
    rng = np.random.default_rng(3)
    low, high = points.min(axis=0), points.max(axis=0)
    h = STEP
    worst = 0.0
    for t in thetas:
        x = rng.uniform(low, high)
        j = reference.jacobian(tables, setup, points, t, x, modulate=modulate)
        assert np.all(j['ngal_tables'] > 0.0) and all(np.all(np.isfinite(a)) for a in j.values())
        coarse = central_differences(tables, setup, t, x, h, modulate)
        fine = central_differences(tables, setup, t, x, h / 2, modulate)
        for analytic, f1, f2, value in ((j['dngal'], coarse[0], fine[0], j['ngal']),
                                        (j['dxi'], coarse[1], fine[1], j['xi'])):
            bound = np.abs(f1 - f2) + 8 * EPS * np.max(np.abs(value)) / (h / 2)
            worst = max(worst, np.max(np.abs(analytic - f2) / bound))
            assert np.all(np.abs(analytic - f2) <= bound)
    print('worst |J - FD(h/2)| / bound:', worst)


def test_stress_draws_have_galaxies_in_every_table_of_the_fixture():
    """The draws of the GPU tests on the reference's own fixture: every one of the four tables has
    galaxies in every draw and the reference is finite, for both values of modulate."""
    from tabcorr_amd import Interpolator
    interp = Interpolator.read(os.path.join(REPO, 'tests', 'golden', 'ds_efficient.hdf5'))
    tables = [{'gal_type': h.gal_type.as_array(),
               'tpcf_matrix': np.asarray(h.tpcf_matrix, dtype=np.float64),
               'tpcf_shape': tuple(h.tpcf_shape), 'attrs': dict(h.attrs)}
              for h in interp.tabcorr_list]
    setup = oracle.interpolator_setup(tables, interp.points)
    theta = reference.draws(3)
    x = np.tile(interp.points.mean(axis=0), (3, 1))
    for modulate in (False, True):
        assert reference.has_galaxies(
            reference.jacobian_batch(tables, setup, interp.points, theta, x, modulate=modulate))
    assert interp._device is None


def test_the_four_entry_points_are_declared_listed_and_exported(lib):
    from tabcorr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'tabcorr_amd.h')).read()
    declared = set(re.findall(r'^int (tc_\w+)\(', header, flags=re.M))
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        # the argument lists are those of the assembly-bias four
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace('leauthaud11', 'assembias')]
    for form, stem in (('predict', 'predict_grad'), ('chi2', 'chi2_grad'), ('fisher', 'chi2_grad')):
        assert _lib.GRAD_ENTRIES['interp', 'leauthaud11', form] == \
            'tc_interp_%s_leauthaud11_batch' % stem
    assert 'tc_interp_chi2_grad_leauthaud11_batch' in _lib.GRAD_OPTIONAL_FISHER
    testing = open(os.path.join(ROOT, 'include', 'tabcorr_amd_testing.h')).read()
    assert 'tc_debug_interp_grad_lds_bytes' in re.findall(r'^int (tc_\w+)\(', testing, flags=re.M)
    assert 'tc_debug_interp_grad_lds_bytes' in _lib.SIGNATURES
    # the first argument is the handle: without one every entry refuses before reading the rest
    for name in ENTRIES:
        scalars = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint)
        status = getattr(lib, name)(*[0 if kind in scalars else None
                                      for kind in _lib.SIGNATURES[name]])
        assert status == _lib.TC_ERR_INVALID


# grad.h, restated in rows of 16 doubles.  Q = n_params + 1 quantities (w and its derivatives).
# Both kernels: 2 x 32 rows of weights per axis and Q + D accumulators per r bin.  Mode auto: the
# rows of one class (a central bin keeps 3 / 4 / 7 of them, a satellite bin 6 / 7 / 12, one row of
# zeros) and Q totals.  Mode cross: Q slabs -- 64 bins for 5 and 7 parameters, 32 for 11 --, Q
# totals and the Q + D weighted products per r bin of the class in flight.
CENTRAL_ROWS = {5: 3, 7: 4, 11: 7}
SATELLITE_ROWS = {5: 6, 7: 7, 11: 12}
CROSS_SLAB = {5: 64, 7: 64, 11: 32}


def restated_bytes(mode, n_params, n_bins, n_central, n_r, n_dim):
    q = n_params + 1
    common = 2 * 32 * n_dim + (q + n_dim) * n_r
    if mode == AUTO:
        rows = (CENTRAL_ROWS[n_params] * n_central +
                SATELLITE_ROWS[n_params] * (n_bins - n_central) + 1) + q + common
    else:
        rows = q * (CROSS_SLAB[n_params] + 1) + (q + n_dim) * n_r + common
    return rows * 16 * 8


def lds_bytes(lib, mode, n_params, n_bins, n_central, n_r, n_dim, chi2):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    _lib.check(lib.tc_debug_interp_grad_lds_bytes(mode, n_params, n_bins, n_central, n_r, n_dim,
                                                  chi2, ctypes.byref(got)))
    return got.value


def test_lds_debug_entry_against_the_restated_formula(lib):
    """For 5, 7 and 11 parameters; for 5 and 7 it is what tc_debug_grad_lds(2 | 3, ...) returns
    (those budgets are unchanged), which goes on refusing 11."""
    from tabcorr_amd import _lib
    for n_bins, n_central, n_r, n_dim in ((4, 2, 1, 1), (36, 18, 5, 2), (100, 50, 19, 3),
                                          (201, 100, 40, 8), (7, 7, 3, 4), (7, 7, 3, 5)):
        for mode in (AUTO, CROSS):
            for chi2 in (0, 1):
                for n_params in (5, 7, 11):
                    if n_params + 1 + n_dim > 16:
                        # one thread per (quantity, draw) of 256: eleven parameters, four axes
                        bad = ctypes.c_int64(-1)
                        assert lib.tc_debug_interp_grad_lds_bytes(
                            mode, n_params, n_bins, n_central, n_r, n_dim, chi2,
                            ctypes.byref(bad)) == _lib.TC_ERR_UNSUPPORTED
                        continue
                    got = lds_bytes(lib, mode, n_params, n_bins, n_central, n_r, n_dim, chi2)
                    assert got == restated_bytes(mode, n_params, n_bins, n_central, n_r, n_dim)
                    old = ctypes.c_int64(-1)
                    status = lib.tc_debug_grad_lds(2 + mode, n_params, n_bins, n_central, n_r,
                                                   n_dim, chi2, ctypes.byref(old))
                    if n_params == 11:
                        assert status == _lib.TC_ERR_INVALID
                    else:
                        assert status == _lib.TC_OK and old.value == got
    # the budgets of the two families that were there, in numbers: a slab of 64 bins
    assert lds_bytes(lib, CROSS, 5, 0, 0, 12, 2, 0) == (6 * 65 + 2 * 8 * 12 + 128) * 128 == 90880
    assert lds_bytes(lib, CROSS, 7, 0, 0, 12, 2, 1) == (8 * 65 + 2 * 10 * 12 + 128) * 128 == 113664
    assert lds_bytes(lib, AUTO, 5, 28, 14, 5, 2, 0) == (3 * 14 + 6 * 14 + 1 + 6 + 128 + 40) * 128
    bad = ctypes.c_int64(-1)
    for arguments in ((2, 11, 4, 2, 1, 1, 0), (AUTO, 6, 4, 2, 1, 1, 0), (AUTO, 11, 2, 4, 1, 1, 0),
                      (CROSS, 11, 4, 2, 1, -1, 0)):
        assert lib.tc_debug_interp_grad_lds_bytes(*arguments,
                                                  ctypes.byref(bad)) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_interp_grad_lds_bytes(AUTO, 11, 4, 2, 1, 1, 0, None) == _lib.TC_ERR_INVALID


def test_shapes_that_must_be_served_and_refused(lib):
    # the reference's database layout: three axes, 14 Delta Sigma bins, likelihood and Fisher
    assert lds_bytes(lib, CROSS, 11, 0, 0, 14, 3, 1) == \
        (12 * 33 + 2 * 15 * 14 + 2 * 3 * 32) * 128 == 1008 * 128 == 129024 <= LDS_LIMIT
    # ... which a slab of 64 bins would refuse: 12 x 32 rows more
    assert 129024 + 12 * 32 * 128 == 178176 > LDS_LIMIT
    # the reference's own fixture ds_efficient.hdf5: 1104 bins, n_r = 13, D = 1
    assert lds_bytes(lib, CROSS, 11, 1104, 552, 13, 1, 1) == \
        (12 * 33 + 2 * 13 * 13 + 64) * 128 == 102144 <= LDS_LIMIT
    # the limits of mode cross per number of axes
    for n_dim, n_r in ((1, 31), (2, 27), (3, 23)):
        assert lds_bytes(lib, CROSS, 11, 0, 0, n_r, n_dim, 1) <= LDS_LIMIT
        assert lds_bytes(lib, CROSS, 11, 0, 0, n_r + 1, n_dim, 1) > LDS_LIMIT
    # mode auto: 28 bins, n_r = 5, D = 2
    assert lds_bytes(lib, AUTO, 11, 28, 14, 5, 2, 0) == \
        (7 * 14 + 12 * 14 + 1 + 12 + 128 + 14 * 5) * 128 == 61056 <= LDS_LIMIT
    # refused for this family, served for Zheng07: mode auto, 128 bins, n_r = 5, D = 1, prediction
    assert lds_bytes(lib, AUTO, 11, 128, 64, 5, 1, 0) == 173824 > LDS_LIMIT
    assert lds_bytes(lib, AUTO, 5, 128, 64, 5, 1, 0) == \
        (3 * 64 + 6 * 64 + 1 + 6 + 64 + 7 * 5) * 128 == 87296 <= LDS_LIMIT


def make_interpolator(grid=(4, 5), tpcf_shape=(5, )):
    from tabcorr_amd import Interpolator, TabCorr
    tables, keys, points = synthetic.synthetic_interpolator(grid, 4, 1, tpcf_shape, 'auto', seed=7)
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
                for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)}), points


def untouched(interp):
    return interp._device is None and all(h._device is None for h in interp.tabcorr_list)


@pytest.mark.parametrize('tpcf_shape', [(5, ), (3, 4)])
def test_gradient_calls_reject_wrong_arguments_before_any_device_is_touched(tpcf_shape):
    interp, points = make_interpolator(tpcf_shape=tpcf_shape)
    n_r = int(np.prod(tpcf_shape))
    theta = reference.draws(3)
    x = np.tile(points.mean(axis=0), (3, 1))
    data, precision = np.zeros(tpcf_shape), np.eye(n_r)

    def every(error, match, theta, x, data=data, precision=precision, **kwargs):
        with pytest.raises(error, match=match):
            interp.predict_batch_grad(theta, x, **kwargs)
        with pytest.raises(error, match=match):
            interp.chi2_grad_batch(theta, x, data, precision, **kwargs)
        with pytest.raises(error, match=match):
            interp.chi2_fisher_batch(theta, x, data, precision, **kwargs)
        with pytest.raises(error, match=match):
            interp.fisher_batch(theta, x, precision, **kwargs)

    family = 'leauthaud11'
    for columns in (5, 7, 11, 13, 15):
        every(ValueError, 'theta', np.zeros((3, columns)), x, family=family)
    # fourteen columns are not a Zheng07 draw, decorated or not
    every(ValueError, 'theta', theta, x)
    every(ValueError, 'theta', theta, x, assembias=True)
    # the family has no assembly bias; an unknown family
    every(ValueError, 'assembias', theta, x, assembias=True, family=family)
    every(ValueError, 'family', theta, x, family='zheng08')
    every(ValueError, 'family', synthetic.zheng07_draws(3, seed=2), x, family='tinker13')
    # x: a row missing, a column missing, one too many, outside the grid
    every(ValueError, 'x must', theta, x[:2], family=family)
    every(ValueError, 'x must', theta, x[:, :1], family=family)
    every(ValueError, 'x must', theta, np.hstack([x, x[:, :1]]), family=family)
    for d in range(2):
        for value in (points[:, d].min() - 0.01, points[:, d].max() + 0.01, np.nan):
            outside = x.copy()
            outside[1, d] = value
            every(ValueError, 'extrapolation', theta, outside, family=family)
    for bad_data, bad_precision in ((np.zeros(n_r + 1), precision), (data, np.eye(n_r + 1)),
                                    (data, np.ones((n_r, n_r + 1)))):
        with pytest.raises(ValueError, match='precision'):
            interp.chi2_grad_batch(theta, x, bad_data, bad_precision, family=family)
        with pytest.raises(ValueError, match='precision'):
            interp.chi2_fisher_batch(theta, x, bad_data, bad_precision, family=family)
    with pytest.raises(ValueError, match='precision'):
        interp.fisher_batch(theta, x, np.eye(n_r + 1), family=family)
    assert untouched(interp)


def test_model_calls_need_the_extra_parameters_before_any_device_is_touched():
    """`predict_grad` and `fisher` of a Leauthaud11Model: a missing extra parameter is a
    ValueError that names it, a decorated call a ValueError, before any device is touched."""
    from tabcorr_amd import Leauthaud11Model
    interp, points = make_interpolator()
    model = Leauthaud11Model(threshold=10.5, redshift=0.3)
    precision = np.eye(5)
    with pytest.raises(ValueError, match='log_eta'):
        interp.predict_grad(model, check_consistency=False)
    with pytest.raises(ValueError, match='log_eta'):
        interp.fisher(model, precision, check_consistency=False)
    model.param_dict['log_eta'] = points[:, 0].mean()
    with pytest.raises(ValueError, match='alpha_s'):
        interp.predict_grad(model, check_consistency=False)
    with pytest.raises(ValueError, match='alpha_s'):
        interp.fisher(model, precision, check_consistency=False)
    model.param_dict['alpha_s'] = points[:, 1].max() + 0.5
    with pytest.raises(ValueError, match='extrapolation'):
        interp.predict_grad(model, check_consistency=False)
    with pytest.raises(ValueError, match='extrapolation'):
        interp.fisher(model, precision, check_consistency=False)
    model.param_dict['alpha_s'] = points[:, 1].mean()
    with pytest.raises(ValueError, match='assembias'):
        interp.predict_grad(model, check_consistency=False, assembias=True)
    with pytest.raises(ValueError, match='assembias'):
        interp.fisher(model, precision, check_consistency=False, assembias=True)
    with pytest.raises(ValueError, match='precision'):
        interp.fisher(model, np.eye(4), check_consistency=False)
    assert untouched(interp)
