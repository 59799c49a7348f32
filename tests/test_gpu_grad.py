"""Analytic gradients on the device (TabCorr.predict_batch_grad / chi2_grad_batch /
predict_grad, the tc_*_grad_* entry points) against the reference Jacobian of grad_reference.py
and the oracle's values.  Needs an MI355X.

Tolerance of a derivative: rtol = 1e-10 (the project's parity bar) plus, per (draw, k), 1e-10 x
the size of the terms that cancel in it (grad_reference.jacobian: scale) -- the same bar applied
to those terms.  Every case prints its largest error in units of that allowance.
"""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from util import assert_rel, load_golden, table_from_golden  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-10
D = 16                               # draws per workgroup of the gradient kernels (grad.h)
DRAW_COUNTS = [1, D - 1, D, D + 1, 2 * D + 3]
N_MAX = max(DRAW_COUNTS)

_tables = {}
_references = {}


def get_table(shape, mode):
    """(table dict, TabCorr) of a synthetic (n_prim, n_sec, n_r) table, made once."""
    key = (shape, mode)
    if key not in _tables:
        from tabcorr_amd import TabCorr
        table = synthetic.synthetic_table(shape[0], shape[1], (shape[2], ), mode, seed=3)
        _tables[key] = (table, TabCorr.from_arrays(
            table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'], table['attrs']))
    return _tables[key]


def get_reference(shape, mode, modulate, n_gauss):
    """Draws and their reference (ngal, xi, dngal, dxi, scale), computed once per combination and
    never modified: a batch of n draws is the first n of them."""
    key = (shape, mode, modulate, n_gauss)
    if key not in _references:
        table, _ = get_table(shape, mode)
        theta = grad_reference.stress_draws(table, N_MAX, seed=5, n_gauss_prim=n_gauss)
        reference = grad_reference.jacobian_batch(table, theta, n_gauss, modulate)
        values = oracle.predict_zheng07_batch(table, theta, n_gauss_prim=n_gauss,
                                              modulate_with_cenocc=modulate)
        for array in (theta, ) + reference + values:
            array.setflags(write=False)
        _references[key] = (theta, reference, values)
    return _references[key]


def check_derivatives(got_dngal, got_dxi, reference, what):
    _, _, dngal, dxi, scale = reference
    assert_rel(got_dngal, dngal, RTOL, what + ' dngal')
    extra = (1, ) * (dxi.ndim - 2)
    allowance = RTOL * np.abs(dxi) + RTOL * scale.reshape(scale.shape + extra)
    error = np.abs(got_dxi - dxi)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(error == 0.0, 0.0, error / allowance)
    print('%s: max |dxi - reference| / allowance = %.3g' % (what, np.max(ratio)))
    assert np.all(error <= allowance), (what, np.max(ratio))


AUTO_SHAPES = [(7, 1, 5), (9, 2, 5), (50, 1, 19), (52, 2, 21)]
CROSS_SHAPES = [(9, 2, 5), (276, 2, 13)]
CASES = ([(shape, 'auto') for shape in AUTO_SHAPES] +
         [(shape, 'cross') for shape in CROSS_SHAPES])


@pytest.mark.parametrize('n_gauss', [10, 3])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('shape,mode', CASES,
                         ids=['%s-%dx%dx%d' % ((m, ) + s) for s, m in CASES])
def test_gradient_matches_reference_jacobian(shape, mode, n_draws, modulate, n_gauss):
    _, halotab = get_table(shape, mode)
    theta, reference, values = get_reference(shape, mode, modulate, n_gauss)
    ngal, xi, dngal, dxi = halotab.predict_batch_grad(
        theta[:n_draws], n_gauss_prim=n_gauss, modulate_with_cenocc=modulate)
    assert dngal.shape == (n_draws, 5) and dxi.shape == (n_draws, 5, shape[2])
    what = '%s %s n=%d modulate=%s ng=%d' % (mode, shape, n_draws, modulate, n_gauss)
    assert_rel(ngal, values[0][:n_draws], RTOL, what + ' ngal')
    assert_rel(xi, values[1][:n_draws], RTOL, what + ' xi')
    assert_rel(ngal, reference[0][:n_draws], RTOL, what + ' ngal')
    check_derivatives(dngal, dxi, tuple(a[:n_draws] for a in reference), what)
    # logM0 above the top bin edge: no satellites, exactly zero derivatives
    empty = np.nonzero(theta[:n_draws, 2] >
                       get_table(shape, mode)[0]['gal_type']['log_prim_haloprop_max'].max())[0]
    for i in empty:
        assert np.all(reference[2][i, 2:] == 0.0)
        assert np.all(dngal[i, 2:] == 0.0) and np.all(dxi[i, 2:] == 0.0)


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('shape,mode', [((9, 2, 5), 'auto'), ((50, 1, 19), 'auto'),
                                        ((52, 2, 21), 'auto'), ((9, 2, 5), 'cross')])
def test_chi2_gradient(shape, mode, symmetric):
    """chi2 = e^T P e and dchi2_k = 2 e^T P_sym dxi_k; the non-symmetric precision pins the
    P_sym convention.  Allowance, from the allowances of xi (1e-10 |xi|) and dxi (a_rk = 1e-10
    (|dxi_rk| + scale_k)) carried through the two formulas with v = 2 P_sym e:
    chi2: rtol + 1e-10 sum_r |v_r| |xi_r|; dchi2_k: rtol + sum_r |v_r| a_rk +
    2e-10 sum_r (|P_sym| |xi|)_r |dxi_rk|."""
    _, halotab = get_table(shape, mode)
    theta, reference, _ = get_reference(shape, mode, False, 10)
    n_r = shape[2]
    rng = np.random.default_rng(11)
    a = rng.normal(size=(n_r, n_r))
    precision = a @ a.T + n_r * np.eye(n_r)
    if not symmetric:
        precision = precision + rng.normal(size=(n_r, n_r))
    ngal_ref, xi, dngal_ref, dxi, scale = reference
    data = xi[3] * (1.0 + 0.05 * rng.normal(size=n_r))
    ngal, chi2, dngal, dchi2 = halotab.chi2_grad_batch(theta, data, precision)
    p_sym = 0.5 * (precision + precision.T)
    e = xi - data
    v = 2.0 * e @ p_sym
    chi2_ref = np.einsum('nr,rs,ns->n', e, precision, e)
    dchi2_ref = np.einsum('nr,nkr->nk', v, dxi)
    assert_rel(ngal, ngal_ref, RTOL)
    assert_rel(dngal, dngal_ref, RTOL)
    chi2_allow = RTOL * np.abs(chi2_ref) + RTOL * np.sum(np.abs(v) * np.abs(xi), axis=1)
    a_rk = RTOL * (np.abs(dxi) + scale[:, :, None])
    dchi2_allow = (RTOL * np.abs(dchi2_ref) + np.einsum('nr,nkr->nk', np.abs(v), a_rk) +
                   2.0 * RTOL * np.einsum('nr,nkr->nk', np.abs(xi) @ np.abs(p_sym), np.abs(dxi)))
    print('chi2 %s %s: max error / allowance = %.3g (chi2), %.3g (dchi2)' % (
        mode, shape, np.max(np.abs(chi2 - chi2_ref) / chi2_allow),
        np.max(np.abs(dchi2 - dchi2_ref) / np.maximum(dchi2_allow, 1e-300))))
    assert np.all(np.abs(chi2 - chi2_ref) <= chi2_allow)
    assert np.all(np.abs(dchi2 - dchi2_ref) <= dchi2_allow)
    # the value agrees with the forward entry point to parity
    assert_rel(chi2, halotab.chi2_batch(theta, data, precision)[1], RTOL)


def device_call(halotab, theta, n_gauss=10, flags=0):
    """tc_predict_grad_zheng07_batch_device on freshly allocated device arrays."""
    from tabcorr_amd import _lib
    device = halotab.to_device()
    lib = device.lib
    n, n_r = len(theta), device.n_r
    outputs = [np.empty(n), np.empty((n, n_r)), np.empty((n, 5)), np.empty((n, 5, n_r))]
    theta = np.ascontiguousarray(theta)
    pointers = []
    for array in [theta] + outputs:
        ptr = ctypes.c_void_p()
        _lib.check(lib.tc_device_malloc(ctypes.byref(ptr), array.nbytes))
        pointers.append(ptr)
    try:
        with device.lock:
            _lib.check(lib.tc_memcpy_h2d(pointers[0], theta.ctypes.data_as(ctypes.c_void_p),
                                         theta.nbytes))
            _lib.check(lib.tc_predict_grad_zheng07_batch_device(
                device.handle, pointers[0], 5, n, n_gauss, flags, *pointers[1:]))
            _lib.check(lib.tc_table_synchronize(device.handle))
            for array, ptr in zip(outputs, pointers[1:]):
                _lib.check(lib.tc_memcpy_d2h(array.ctypes.data_as(ctypes.c_void_p), ptr,
                                             array.nbytes))
    finally:
        for ptr in pointers:
            lib.tc_device_free(ptr)
    return outputs


@pytest.mark.parametrize('shape,mode', [((50, 1, 19), 'auto'), ((7, 1, 5), 'auto'),
                                        ((276, 2, 13), 'cross')])
def test_batch_invariance(shape, mode):
    """A draw's 6 (1 + R) outputs are bit-equal in batches of 1, D + 1 and 2 D + 3 draws and
    between the host-array and the device-pointer entry points."""
    _, halotab = get_table(shape, mode)
    theta, _, _ = get_reference(shape, mode, False, 10)
    full = halotab.predict_batch_grad(theta)
    for n in (1, D + 1):
        part = halotab.predict_batch_grad(theta[:n])
        for a, b in zip(part, full):
            assert np.array_equal(a, b[:n], equal_nan=True)
    # the last draw alone, and in the middle of another batch
    alone = halotab.predict_batch_grad(theta[-1:])
    for a, b in zip(alone, full):
        assert np.array_equal(a[0], b[-1], equal_nan=True)
    for n in (1, D + 1, N_MAX):
        for a, b in zip(device_call(halotab, theta[:n]), full):
            assert np.array_equal(a.reshape(b[:n].shape), b[:n], equal_nan=True)


@pytest.mark.parametrize('name', ['bolplanck_wp', 'bolplanck_ds'])
def test_real_table(name):
    from tabcorr_amd import TabCorr, Zheng07Model
    from tabcorr_amd.models import ZHENG07_KEYS
    data = load_golden(name)
    table = table_from_golden(data)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                  table['tpcf_shape'], table['attrs'])
    nodes = grad_reference.nodes_of(table)
    theta = np.resize(np.array(data['theta'], dtype=np.float64), (N_MAX, 5)).copy()
    theta[len(data['theta']):] += 0.01
    theta = grad_reference.centre_log_m0(theta, nodes)
    reference = grad_reference.jacobian_batch(table, theta)
    ngal, xi, dngal, dxi = halotab.predict_batch_grad(theta)
    values = oracle.predict_zheng07_batch(table, theta)
    assert_rel(ngal, values[0], RTOL)
    assert_rel(xi, values[1], RTOL)
    check_derivatives(dngal, dxi, reference, name)
    if name == 'bolplanck_wp':
        model = Zheng07Model(redshift=0.0)
        for key, value in zip(ZHENG07_KEYS, theta[0]):
            model.param_dict[key] = value
        one = halotab.predict_grad(model)
        assert isinstance(one[0], float) and one[1].shape == tuple(table['tpcf_shape'])
        assert list(one[2]) == list(ZHENG07_KEYS) and list(one[3]) == list(ZHENG07_KEYS)
        assert one[0] == ngal[0] and np.array_equal(one[1], xi[0])
        for k, key in enumerate(ZHENG07_KEYS):
            assert one[2][key] == dngal[0, k]
            assert np.array_equal(one[3][key], dxi[0, k])


def test_unsupported_requests_leave_the_handle_usable():
    from tabcorr_amd import TabCorr, _lib
    table = synthetic.synthetic_table(9, 2, (5, ), 'auto', seed=3)
    theta = synthetic.zheng07_draws(5, seed=2)
    expect = oracle.predict_zheng07_batch(table, theta)

    def still_works(halotab, rtol):
        ngal, xi = halotab.predict_batch(theta)
        assert_rel(ngal, expect[0], rtol)
        assert_rel(xi, expect[1], rtol)

    single = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                 table['attrs'], compute_dtype='float32')
    with pytest.raises(NotImplementedError, match='float64'):
        single.predict_batch_grad(theta)
    still_works(single, 1e-5)         # the float32 path's stated tolerance

    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                  table['attrs'])
    device = halotab.to_device()
    n, n_r = len(theta), device.n_r
    outputs = [np.empty(n * 2), np.empty(n * 3 * n_r), np.empty(n * 10), np.empty(n * 15 * n_r)]
    for flags, columns in ((_lib.FLAG_SEPARATE_GAL_TYPE, 5), (_lib.FLAG_ASSEMBIAS, 7)):
        wide = np.ascontiguousarray(np.hstack([theta, np.zeros((n, 2))])[:, :columns])
        with device.lock:
            status = device.lib.tc_predict_grad_zheng07_batch(
                device.handle, _lib.as_double_p(wide), columns, n, 10, flags,
                *[_lib.as_double_p(a) for a in outputs])
        assert status == _lib.TC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            _lib.check(status)
        still_works(halotab, RTOL)
    # and the gradient call itself still serves the handle
    reference = grad_reference.jacobian_batch(
        table, grad_reference.centre_log_m0(theta.copy(), grad_reference.nodes_of(table)))
    got = halotab.predict_batch_grad(
        grad_reference.centre_log_m0(theta.copy(), grad_reference.nodes_of(table)))
    check_derivatives(got[2], got[3], reference, 'after the refused calls')
