"""Gradients of the Leauthaud11 family on the device (`family='leauthaud11'` of predict_batch_grad
/ chi2_grad_batch / chi2_fisher_batch / fisher_batch, predict_grad / fisher of a Leauthaud11Model,
the tc_*_grad_leauthaud11_* entry points) against the eleven-column reference Jacobian of
leauthaud11_grad_reference.py and the forward calls.  Needs an MI355X.

Allowance of a derivative, as in test_gpu_grad.py: 1e-10 |reference| (the project's parity bar)
plus 1e-10 of the size of the terms that cancel in it (the reference's `scale`); the likelihood
and the Fisher matrix carry it through their formulas (test_gpu_grad.check_chi2_values,
fisher_reference).  Every case prints its largest error in units of its allowance.  The
occupation is smooth: no draw has to keep clear of a node.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference  # noqa: E402
import leauthaud11_grad_reference as reference  # noqa: E402
import test_gpu_grad as table_suite  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    D, LDS_LIMIT, RTOL, check_still_serves, chi2_data, device_call, largest, same_bits)
from util import assert_rel, load_golden, table_from_golden  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILY = 'leauthaud11'
DRAW_COUNTS = [1, D, D + 1, 2 * D + 3]
N_MAX = max(DRAW_COUNTS)

_tables = {}
_references = {}


def make_tabcorr(table, **kwargs):
    from tabcorr_amd import TabCorr
    return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                               table['attrs'], **kwargs)


def get_table(n_prim, n_sec, tpcf_shape, mode):
    key = (n_prim, n_sec, tpcf_shape, mode)
    if key not in _tables:
        table = synthetic.synthetic_table(n_prim, n_sec, tpcf_shape, mode, seed=3)
        _tables[key] = (table, make_tabcorr(table))
    return _tables[key]


def get_reference(n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss, n_draws=N_MAX):
    """Draws (n_draws, 14), stress draws first, and their reference (ngal, xi, dngal, dxi, scale),
    computed once per combination and never modified: a batch of n draws is the first n of them.
    Every draw has galaxies and a finite reference."""
    key = (n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss, n_draws)
    if key not in _references:
        table, _ = get_table(n_prim, n_sec, tpcf_shape, mode)
        theta = reference.stress_draws(n_draws, seed=5)
        expect = reference.jacobian_batch(table, theta, n_gauss, modulate)
        assert reference.usable(expect), key
        for array in (theta, ) + expect:
            array.setflags(write=False)
        _references[key] = (theta, expect)
    return _references[key]


def check_gradient(halotab, theta, expect, n_gauss, modulate, tpcf_shape, what):
    n = len(theta)
    ngal, xi, dngal, dxi = halotab.predict_batch_grad(
        theta, n_gauss_prim=n_gauss, modulate_with_cenocc=modulate, family=FAMILY)
    assert ngal.shape == (n, ) and xi.shape == (n, ) + tpcf_shape
    assert dngal.shape == (n, 11) and dxi.shape == (n, 11) + tpcf_shape
    assert_rel(ngal, expect[0][:n], RTOL, what + ' ngal')
    assert_rel(xi, expect[1][:n], RTOL, what + ' xi')
    forward = halotab.predict_batch(theta, n_gauss_prim=n_gauss, modulate_with_cenocc=modulate,
                                    family=FAMILY)
    assert_rel(ngal, forward[0], RTOL, what + ' ngal against predict_batch')
    assert_rel(xi, forward[1], RTOL, what + ' xi against predict_batch')
    table_suite.check_derivatives(dngal, dxi, tuple(a[:n] for a in expect), what)
    return ngal, xi, dngal, dxi


def case_id(case):
    n_prim, n_sec, tpcf_shape, mode = case
    return '%s-%dx%dx%s' % (mode, n_prim, n_sec, 'x'.join(map(str, tpcf_shape)))


# (n_prim, n_sec, tpcf_shape, mode): mode auto with 18 bins and 36 (the family ignores the
# percentile), mode cross with 18 bins and with 80 (two slabs)
CASES = [(9, 1, (5, ), 'auto'), (9, 2, (5, ), 'auto'), (9, 1, (5, ), 'cross'),
         (20, 2, (5, ), 'cross')]


@pytest.mark.parametrize('n_gauss', [3, 10, 16])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_gradient_matches_reference_jacobian(case, n_draws, modulate, n_gauss):
    n_prim, n_sec, tpcf_shape, mode = case
    _, halotab = get_table(*case)
    theta, expect = get_reference(n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss)
    assert len(theta) == N_MAX and theta[0, 5] == 0.03
    check_gradient(halotab, theta[:n_draws], expect, n_gauss, modulate, tpcf_shape,
                   '%s n=%d modulate=%s ng=%d' % (case_id(case), n_draws, modulate, n_gauss))


# mode auto with 2 bins (half a step of four matrix columns), 4 (one step), 16 (one whole tile)
# and 34 (padding in the third tile); twelve r bins on two axes; one node per bin
EDGE_CASES = [(1, 1, (5, ), 'auto', 10), (1, 2, (5, ), 'auto', 10), (4, 2, (5, ), 'auto', 10),
              (17, 1, (5, ), 'auto', 10), (9, 1, (3, 4), 'auto', 10), (9, 1, (5, ), 'auto', 1),
              (9, 1, (3, 4), 'cross', 1)]


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('entry', EDGE_CASES, ids=lambda e: '%s-ng%d' % (case_id(e[:4]), e[4]))
def test_loop_edges(entry, modulate):
    case, n_gauss = entry[:4], entry[4]
    _, halotab = get_table(*case)
    theta, expect = get_reference(*case, modulate, n_gauss, n_draws=D + 1)
    check_gradient(halotab, theta, expect, n_gauss, modulate, case[2],
                   'edges %s modulate=%s ng=%d' % (case_id(case), modulate, n_gauss))


# ---- likelihood and Fisher matrix ---------------------------------------------------------------

def flat_reference(expect, n):
    """The first n draws with the r bins on one axis."""
    ngal, xi, dngal, dxi, scale = (a[:n] for a in expect)
    return ngal, xi.reshape(n, -1), dngal, dxi.reshape(n, 11, -1), scale


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', [1, D + 1, 2 * D + 3])
@pytest.mark.parametrize('case', [(9, 2, (5, ), 'auto'), (9, 1, (3, 4), 'auto'),
                                  (20, 2, (5, ), 'cross')], ids=case_id)
def test_likelihood_and_fisher(case, n_draws, modulate, symmetric):
    """chi2, dchi2 (allowances of test_gpu_grad.test_chi2_gradient) and fisher (11, 11)
    (fisher_reference) against the reference Jacobian; the non-symmetric precision pins the
    P_sym convention.  fisher is symmetric to the bit, fisher_batch gives its bits with zero data,
    and the other four results of the Fisher call are those of the gradient call bit for bit."""
    n_prim, n_sec, tpcf_shape, mode = case
    _, halotab = get_table(*case)
    theta, expect = get_reference(n_prim, n_sec, tpcf_shape, mode, modulate, 10)
    data, precision = chi2_data(expect[1][3].ravel(), symmetric)
    theta = theta[:n_draws]
    what = '%s n=%d modulate=%s symmetric=%s' % (case_id(case), n_draws, modulate, symmetric)
    got = halotab.chi2_fisher_batch(theta, data.reshape(tpcf_shape), precision,
                                    modulate_with_cenocc=modulate, family=FAMILY)
    assert [g.shape for g in got] == [(n_draws, ), (n_draws, ), (n_draws, 11), (n_draws, 11),
                                      (n_draws, 11, 11)]
    flat = flat_reference(expect, n_draws)
    table_suite.check_chi2_values(got[1], got[3], flat, data, precision, 'chi2 ' + what)
    assert_rel(got[0], flat[0], RTOL)
    assert_rel(got[2], flat[2], RTOL)
    dxi, a = fisher_reference.table_jacobian(expect)
    fisher_reference.check(got[4], dxi, a, precision, 'fisher ' + what)
    assert np.array_equal(got[4], got[4].transpose(0, 2, 1))
    gradient = halotab.chi2_grad_batch(theta, data.reshape(tpcf_shape), precision,
                                       modulate_with_cenocc=modulate, family=FAMILY)
    assert len(gradient) == 4 and same_bits(got[:4], gradient)
    zero = halotab.chi2_fisher_batch(theta, np.zeros(tpcf_shape), precision,
                                     modulate_with_cenocc=modulate, family=FAMILY)
    forecast = halotab.fisher_batch(theta, precision, modulate_with_cenocc=modulate,
                                    family=FAMILY)
    assert same_bits(forecast, (zero[0], zero[2], zero[4]))
    # (a draw's matrix does not depend on the data)
    assert same_bits(forecast, (got[0], got[2], got[4]))
    # the value agrees with the forward entry point to parity
    assert_rel(got[1], halotab.chi2_batch(theta, data, precision, modulate_with_cenocc=modulate,
                                          family=FAMILY)[1], RTOL)


# ---- batch invariance, the entry points -----------------------------------------------------------

def device_grad(halotab, theta, flags=0):
    device = halotab.to_device()
    n, n_r = len(theta), device.n_r
    return device_call(device, 'tc_predict_grad_leauthaud11_batch_device',
                       [theta, 14, n, 10, flags], [n, (n, n_r), (n, 11), (n, 11, n_r)])


def device_chi2_grad(halotab, theta, data, precision, flags=0):
    from tabcorr_amd import _lib
    device = halotab.to_device()
    n = len(theta)
    data = _lib.contiguous(np.ravel(data))
    precision = _lib.contiguous(precision)
    arguments = [theta, 14, n, 10, flags, _lib.as_double_p(data), _lib.as_double_p(precision)]
    return device_call(device, 'tc_chi2_grad_leauthaud11_batch_device', arguments,
                       [n, n, (n, 11), (n, 11), (n, 11, 11)])


@pytest.mark.parametrize('case', [(9, 2, (5, ), 'auto'), (9, 1, (3, 4), 'auto'),
                                  (20, 2, (5, ), 'cross')], ids=case_id)
def test_batch_invariance_and_device_entries(case):
    """The kernels have one form and every lane solves its own Newton iteration: a draw's bits
    are the same alone, as draw 16 of 17 and in 35, and through the host-array and the
    device-pointer entry points -- for the prediction, the likelihood and the Fisher matrix, and
    with modulate_with_cenocc through the device flags."""
    from tabcorr_amd import _lib
    n_prim, n_sec, tpcf_shape, mode = case
    _, halotab = get_table(*case)
    theta, expect = get_reference(n_prim, n_sec, tpcf_shape, mode, False, 10)
    data, precision = chi2_data(expect[1][3].ravel(), False)
    full = halotab.predict_batch_grad(theta, family=FAMILY)
    full_chi2 = halotab.chi2_fisher_batch(theta, data.reshape(tpcf_shape), precision,
                                          family=FAMILY)
    assert all(np.all(np.isfinite(a)) for a in full + full_chi2)

    def predict(draws):
        return halotab.predict_batch_grad(draws, family=FAMILY)

    def likelihood(draws):
        return halotab.chi2_fisher_batch(draws, data.reshape(tpcf_shape), precision,
                                         family=FAMILY)

    for call, everything in ((predict, full), (likelihood, full_chi2)):
        for rows in (slice(0, 1), slice(D, D + 1), slice(0, D + 1), slice(3, 3 + D)):
            assert same_bits(call(theta[rows]), [b[rows] for b in everything])
    for n in (1, D + 1, N_MAX):
        assert same_bits(device_grad(halotab, theta[:n]), [b[:n] for b in full], reshape=True)
        assert same_bits(device_chi2_grad(halotab, theta[:n], data, precision),
                         [b[:n] for b in full_chi2])
    host = halotab.predict_batch_grad(theta[:D + 1], modulate_with_cenocc=True, family=FAMILY)
    assert same_bits(device_grad(halotab, theta[:D + 1], _lib.FLAG_MODULATE_WITH_CENOCC), host,
                     reshape=True)
    assert not np.array_equal(host[1], full[1][:D + 1])


def test_device_entry_without_a_fisher_matrix():
    """The trailing `fisher` of the likelihood entry may be NULL: the four other results are the
    same bits."""
    import ctypes
    from tabcorr_amd import _lib
    case = (9, 2, (5, ), 'auto')
    _, halotab = get_table(*case)
    theta, expect = get_reference(*case, False, 10)
    data, precision = chi2_data(expect[1][3].ravel(), False)
    n = D + 1
    full = device_chi2_grad(halotab, theta[:n], data, precision)
    device = halotab.to_device()
    lib = device.lib
    draws = np.ascontiguousarray(theta[:n])
    outputs = [np.empty(shape) for shape in (n, n, (n, 11), (n, 11))]
    pointers = []
    try:
        for array in [draws] + outputs:
            ptr = ctypes.c_void_p()
            _lib.check(lib.tc_device_malloc(ctypes.byref(ptr), max(array.nbytes, 8)))
            pointers.append(ptr)
        with device.lock:
            _lib.check(lib.tc_memcpy_h2d(pointers[0], draws.ctypes.data_as(ctypes.c_void_p),
                                         draws.nbytes))
            _lib.check(lib.tc_chi2_grad_leauthaud11_batch_device(
                device.handle, pointers[0], 14, n, 10, 0, _lib.as_double_p(_lib.contiguous(data)),
                _lib.as_double_p(_lib.contiguous(precision)), *pointers[1:], None))
            _lib.check(lib.tc_table_synchronize(device.handle))
            for array, ptr in zip(outputs, pointers[1:]):
                _lib.check(lib.tc_memcpy_d2h(array.ctypes.data_as(ctypes.c_void_p), ptr,
                                             array.nbytes))
    finally:
        for ptr in pointers:
            lib.tc_device_free(ptr)
    assert same_bits(outputs, full[:4])


# ---- the real table ---------------------------------------------------------------------------------

@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
def test_real_table(modulate):
    """The table of the leauthaud11_bolplanck_wp fixture (60 bins, 19 r bins) and its 12 draws:
    the values against the fixture, recorded from the reference, the derivatives against the
    reference Jacobian."""
    data = load_golden('leauthaud11_bolplanck_wp')
    table = table_from_golden(data)
    halotab = make_tabcorr(table)
    theta = np.ascontiguousarray(data['theta'])
    assert theta.shape == (12, 14)
    expect = reference.jacobian_batch(table, theta, 10, modulate)
    assert reference.usable(expect)
    suffix = '' if modulate else '_nomodulate'
    got = check_gradient(halotab, theta, expect, 10, modulate, tuple(table['tpcf_shape']),
                         'bolplanck wp modulate=%s' % modulate)
    assert_rel(got[0], data['ngal' + suffix], RTOL)
    assert_rel(got[1], data['xi' + suffix], RTOL)


# ---- limits -----------------------------------------------------------------------------------------
# The family's budget of grad_auto_kernel (csrc/grad.h), in rows of D doubles: seven rows per
# central bin, twelve per satellite bin, one row of zeros, twelve rows of totals, and twelve per r
# bin for the likelihood.

def auto_lds_bytes(n_bins, n_central, n_r=0):
    return (7 * n_central + 12 * (n_bins - n_central) + 1 + 12 + 12 * n_r) * D * 8


def test_lds_limit_auto():
    """One secondary bin, three r bins: the table with the most bins that the gradient serves
    matches the reference; one more primary bin is refused naming LDS, and the handle then goes on
    serving predict_batch."""
    n_prim = largest(lambda n: auto_lds_bytes(2 * n, n) <= LDS_LIMIT)
    case = (n_prim, 1, (3, ), 'auto')
    _, halotab = get_table(*case)
    theta, expect = get_reference(*case, False, 10, n_draws=D + 1)
    check_gradient(halotab, theta, expect, 10, False, (3, ),
                   'LDS limit auto %d bins' % (2 * n_prim))
    table = synthetic.synthetic_table(n_prim + 1, 1, (3, ), 'auto', seed=3)
    halotab = make_tabcorr(table)
    draws = reference.stress_draws(5, seed=5)
    with pytest.raises(NotImplementedError, match='LDS'):
        halotab.predict_batch_grad(draws, family=FAMILY)
    check_still_serves(halotab, table)


def test_lds_limit_of_the_likelihood_alone():
    """A table that serves predict_batch_grad but, with the twelve stash rows per r bin, not the
    likelihood: chi2_grad_batch and chi2_fisher_batch alone refuse it."""
    n_prim, n_r = 60, 19
    assert auto_lds_bytes(2 * n_prim, n_prim) <= LDS_LIMIT < auto_lds_bytes(2 * n_prim, n_prim, n_r)
    table = synthetic.synthetic_table(n_prim, 1, (n_r, ), 'auto', seed=3)
    halotab = make_tabcorr(table)
    draws = reference.stress_draws(6, seed=5)
    expect = reference.jacobian_batch(table, draws, 10, False)
    assert reference.usable(expect)
    check_gradient(halotab, draws, expect, 10, False, (n_r, ), 'likelihood limit')
    with pytest.raises(NotImplementedError, match='LDS'):
        halotab.chi2_grad_batch(draws, np.zeros(n_r), np.eye(n_r), family=FAMILY)
    with pytest.raises(NotImplementedError, match='LDS'):
        halotab.chi2_fisher_batch(draws, np.zeros(n_r), np.eye(n_r), family=FAMILY)
    check_still_serves(halotab, table)
    check_gradient(halotab, draws, expect, 10, False, (n_r, ), 'after the refusals')


def test_unsupported_requests_leave_the_handle_usable():
    from tabcorr_amd import _lib
    case = (9, 2, (5, ), 'auto')
    table, halotab = get_table(*case)
    theta, expect = get_reference(*case, False, 10)
    single = make_tabcorr(table, compute_dtype='float32')
    with pytest.raises(NotImplementedError, match='float64'):
        single.predict_batch_grad(theta[:5], family=FAMILY)
    check_still_serves(single, table, 1e-5)     # (the float32 path's stated tolerance)

    device = halotab.to_device()
    n, n_r = 5, device.n_r
    draws = np.ascontiguousarray(theta[:n])
    outputs = [np.empty(n), np.empty(n * n_r), np.empty(n * 11), np.empty(n * 11 * n_r)]
    for flags in (_lib.FLAG_SEPARATE_GAL_TYPE, _lib.FLAG_ASSEMBIAS, _lib.FLAG_LEAUTHAUD11,
                  _lib.FLAG_MODULATE_WITH_CENOCC | _lib.FLAG_SEPARATE_GAL_TYPE):
        with device.lock:
            status = device.lib.tc_predict_grad_leauthaud11_batch(
                device.handle, _lib.as_double_p(draws), 14, n, 10, flags,
                *[_lib.as_double_p(a) for a in outputs])
        assert status == _lib.TC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            _lib.check(status)
        with device.lock:
            status = device.lib.tc_chi2_grad_leauthaud11_batch(
                device.handle, _lib.as_double_p(draws), 14, n, 10, flags,
                _lib.as_double_p(np.zeros(n_r)), _lib.as_double_p(np.eye(n_r)),
                _lib.as_double_p(outputs[0]), _lib.as_double_p(np.empty(n)),
                _lib.as_double_p(outputs[2]), _lib.as_double_p(np.empty(n * 11)), None)
        assert status == _lib.TC_ERR_UNSUPPORTED
        check_still_serves(halotab, table)
    # eleven columns are not the family's draws
    with device.lock:
        status = device.lib.tc_predict_grad_leauthaud11_batch(
            device.handle, _lib.as_double_p(np.ascontiguousarray(draws[:, :11])), 11, n, 10, 0,
            *[_lib.as_double_p(a) for a in outputs])
    assert status == _lib.TC_ERR_INVALID
    # the Zheng07 entry points go on refusing the family's flag
    with device.lock:
        status = device.lib.tc_predict_grad_zheng07_batch(
            device.handle, _lib.as_double_p(np.ascontiguousarray(draws[:, :5])), 5, n, 10,
            _lib.FLAG_LEAUTHAUD11, *[_lib.as_double_p(a) for a in outputs])
    assert status == _lib.TC_ERR_UNSUPPORTED
    check_gradient(halotab, theta, expect, 10, False, (5, ), 'after the refused calls')


@pytest.mark.parametrize('column', [5, 6], ids=['scatter', 'alphasat'])
@pytest.mark.parametrize('case', [(9, 2, (5, ), 'auto'), (20, 2, (5, ), 'cross')], ids=case_id)
def test_nan_draw(case, column):
    """A NaN in scatter or alphasat makes that draw's ngal, xi, dxi, chi2, dchi2 and Fisher matrix
    NaN -- and those columns of dngal that its bins feed --, and leaves every other draw's bits
    alone."""
    n_prim, n_sec, tpcf_shape, mode = case
    _, halotab = get_table(*case)
    theta, expect = get_reference(n_prim, n_sec, tpcf_shape, mode, False, 10)
    data, precision = chi2_data(expect[1][3].ravel(), True)
    clean = halotab.predict_batch_grad(theta, family=FAMILY)
    clean_chi2 = halotab.chi2_fisher_batch(theta, data, precision, family=FAMILY)
    row = 7
    draws = np.array(theta)
    draws[row, column] = np.nan
    got = halotab.predict_batch_grad(draws, family=FAMILY)
    got_chi2 = halotab.chi2_fisher_batch(draws, data, precision, family=FAMILY)
    others = np.arange(len(theta)) != row
    assert same_bits([a[others] for a in got + got_chi2],
                     [a[others] for a in clean + clean_chi2])
    assert np.isnan(got[0][row]) and np.all(np.isnan(got[1][row]))
    assert np.all(np.isnan(got[3][row]))
    assert np.isnan(got[2][row, column])
    assert np.isnan(got_chi2[1][row]) and np.all(np.isnan(got_chi2[3][row]))
    assert np.all(np.isnan(got_chi2[4][row]))


# ---- model objects ----------------------------------------------------------------------------------

def test_model_object_calls():
    """predict_grad(model) and fisher(model, P) of a Leauthaud11Model at z = 0.3, keyed by the
    sixteen LEAUTHAUD11_KEYS: the smhm_*_0 and the non-relation entries are the bits of the batch
    of the model's device_theta, the smhm_*_a entries (a - 1) times them, the Fisher matrix
    J^T F J."""
    from tabcorr_amd import Leauthaud11Model
    from tabcorr_amd.models import LEAUTHAUD11_KEYS
    case = (9, 2, (5, ), 'auto')
    table, _ = get_table(*case)
    attrs = dict(table['attrs'], redshift=0.3)
    halotab = make_tabcorr(dict(table, attrs=attrs))
    _, expect = get_reference(*case, True, 10)
    _, precision = chi2_data(expect[1][3].ravel(), False)
    model = Leauthaud11Model(threshold=10.6, redshift=0.3)
    assert model.modulate_with_cenocc
    theta = model.device_theta()[np.newaxis]
    a = 1.0 / 1.3
    batch = halotab.predict_batch_grad(theta, modulate_with_cenocc=True, family=FAMILY)
    one = halotab.predict_grad(model)
    assert isinstance(one[0], float) and one[0] == batch[0][0]
    assert np.array_equal(one[1], batch[1][0])
    assert list(one[2]) == list(LEAUTHAUD11_KEYS) == list(one[3])
    for k, name in enumerate(('m0', 'm1', 'beta', 'delta', 'gamma')):
        assert one[2]['smhm_%s_0' % name] == batch[2][0, k]
        assert np.array_equal(one[3]['smhm_%s_0' % name], batch[3][0, k])
        assert one[2]['smhm_%s_a' % name] == (a - 1.0) * batch[2][0, k]
        assert np.array_equal(one[3]['smhm_%s_a' % name], (a - 1.0) * batch[3][0, k])
    for k, key in enumerate(LEAUTHAUD11_KEYS[10:], start=5):
        assert one[2][key] == batch[2][0, k] and np.array_equal(one[3][key], batch[3][0, k])
    forecast = halotab.fisher_batch(theta, precision, modulate_with_cenocc=True, family=FAMILY)
    ngal, dngal, fisher = halotab.fisher(model, precision)
    assert ngal == forecast[0][0] and fisher.shape == (16, 16)
    assert [dngal[key] for key in LEAUTHAUD11_KEYS] == [one[2][key] for key in LEAUTHAUD11_KEYS]
    jacobian = model.device_jacobian()
    assert_rel(fisher, jacobian.T @ forecast[2][0] @ jacobian, RTOL)
    # the model's own setting decides, not a keyword
    plain = Leauthaud11Model(threshold=10.6, redshift=0.3, modulate_with_cenocc=False)
    assert halotab.predict_grad(plain)[0] == halotab.predict_batch_grad(
        theta, family=FAMILY)[0][0]
