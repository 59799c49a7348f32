"""Analytic gradients without a GPU: the reference Jacobian of the tests against finite
differences of the oracle, the new table-driven functions, the dense operand layout of the
gradient kernel and the argument checks of the Python layer."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def central_differences(table, theta, h, modulate):
    dngal = np.zeros(5)
    dxi = []
    for k in range(5):
        e = np.zeros(5)
        e[k] = h
        a = oracle.predict_zheng07(table, theta + e, modulate_with_cenocc=modulate)
        b = oracle.predict_zheng07(table, theta - e, modulate_with_cenocc=modulate)
        dngal[k] = (a[0] - b[0]) / (2 * h)
        dxi.append((a[1] - b[1]) / (2 * h))
    return dngal, np.array(dxi)


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('mode', ['auto', 'cross'])
def test_reference_jacobian_matches_central_differences(mode, modulate):
    """|J - FD(h/2)| <= |FD(h) - FD(h/2)| + 8 eps max|f| / (h/2), elementwise: the error of a
    central difference quarters with h, so the right-hand side bounds it (the worst ratio is the
    expected 1/3) -- no free tolerance.  logM0 sits midway between its neighbouring nodes, more
    than 4 h from both, so that no node crosses M0 inside the stencil."""
    table = synthetic.synthetic_table(9, 2, (5, ), mode, seed=3)
    nodes = grad_reference.nodes_of(table)
    thetas = grad_reference.centre_log_m0(synthetic.zheng07_draws(12, seed=5), nodes)
    h = 1e-4
    worst = 0.0
    for t in thetas:
        assert np.min(np.abs(nodes - t[2])) > 4 * h
        ngal, xi, dngal, dxi, _ = grad_reference.jacobian(table, t, modulate=modulate)
        coarse = central_differences(table, t, h, modulate)
        fine = central_differences(table, t, h / 2, modulate)
        for analytic, f1, f2, value in ((dngal, coarse[0], fine[0], ngal),
                                        (dxi, coarse[1], fine[1], xi)):
            bound = np.abs(f1 - f2) + 8 * EPS * np.max(np.abs(value)) / (h / 2)
            worst = max(worst, np.max(np.abs(analytic - f2) / bound))
            assert np.all(np.abs(analytic - f2) <= bound)
    print('worst |J - FD(h/2)| / bound:', worst)


def test_natural_log_accuracy_on_host(lib):
    """log_fast (ln from the table-driven log2) against numpy, as
    test_fastmath_accuracy_on_host checks its neighbours: the absolute error of log2 is a few
    1e-16 max(1, |log2 y|), which ln 2 scales."""
    from tabcorr_amd import _lib
    rng = np.random.default_rng(5)
    y = np.concatenate([10**rng.uniform(-290, 290, 100000), rng.uniform(0.5, 2.0, 100000),
                        1.0 + np.arange(257) / 256.0, [1.0, 2.0, 0.5, 1e-300]])
    out = np.empty_like(y)
    _lib.check(lib.tc_debug_fastmath(6, y.size, _lib.as_double_p(y), _lib.as_double_p(out)))
    expect = np.log(y)
    assert np.max(np.abs(out - expect) / np.maximum(1.0, np.abs(expect))) < 4e-16


@pytest.mark.parametrize('n_bins', [2, 4, 14, 16, 32, 36, 64, 100])
def test_dense_operand_layout_round_trips(lib, n_bins):
    """The matrix-operand layout the host builds for the gradient kernel, read back lane by lane,
    is the symmetric expansion of the packed matrix (and its padding is zero).  2 and 4 bins are
    a single step of four columns, 16, 32 and 64 whole tiles of 16 rows without padding."""
    from tabcorr_amd import _lib
    n_r = 3
    rng = np.random.default_rng(n_bins)
    packed = np.ascontiguousarray(rng.normal(size=(n_r, n_bins * (n_bins + 1) // 2)))
    dense = np.full((n_r, n_bins, n_bins), np.nan)
    _lib.check(lib.tc_debug_grad_operand(n_bins, n_r, _lib.as_double_p(packed),
                                         _lib.as_double_p(dense)))
    i1, i2, _ = oracle.pair_indices(n_bins)
    expect = np.zeros_like(dense)
    expect[:, i1, i2] = packed
    expect[:, i2, i1] = packed
    assert np.array_equal(dense, expect)
    assert np.array_equal(dense, dense.transpose(0, 2, 1))


def test_gradient_calls_reject_a_wrong_theta_shape():
    """theta with 7 columns (the assembly-bias layout) or 4 is a ValueError before any device
    is touched."""
    from tabcorr_amd import TabCorr
    table = synthetic.synthetic_table(7, 1, (5, ), 'auto', seed=3)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                  table['tpcf_shape'], table['attrs'])
    for columns in (7, 4):
        with pytest.raises(ValueError):
            halotab.predict_batch_grad(np.zeros((3, columns)))
        with pytest.raises(ValueError):
            halotab.chi2_grad_batch(np.zeros((3, columns)), np.zeros(5), np.eye(5))


def test_chi2_gradient_calls_reject_wrong_data_and_precision_shapes(lib):
    """A data vector or a precision matrix that does not fit the table's n_r is a ValueError of
    `chi2_grad_batch` before any device is touched (the C entry points take bare pointers: the
    shapes are the Python layer's to check), with tpcf_shape of one axis and of two.  Both C
    entry points refuse a call without a handle before they read any other argument."""
    from tabcorr_amd import TabCorr, _lib
    theta = synthetic.zheng07_draws(3, seed=2)
    for tpcf_shape in ((5, ), (3, 4)):
        table = synthetic.synthetic_table(7, 1, tpcf_shape, 'auto', seed=3)
        halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                      table['tpcf_shape'], table['attrs'])
        n_r = int(np.prod(tpcf_shape))
        good_data, good_precision = np.zeros(tpcf_shape), np.eye(n_r)
        for data, precision in ((np.zeros(n_r + 1), good_precision),
                                (np.zeros(n_r - 1), good_precision),
                                (np.zeros((n_r, 2)), good_precision),
                                (good_data, np.eye(n_r + 1)),
                                (good_data, np.ones((n_r, n_r + 1))),
                                (good_data, np.ones(n_r * n_r)),
                                (good_data, np.ones((n_r, n_r, 1)))):
            with pytest.raises(ValueError, match='precision'):
                halotab.chi2_grad_batch(theta, data, precision)
        assert halotab._device is None
    empty = np.zeros(0)
    status = lib.tc_chi2_grad_zheng07_batch(
        None, _lib.as_double_p(theta), 5, 3, 10, 0, *[_lib.as_double_p(empty)] * 6)
    assert status == _lib.TC_ERR_INVALID
    with pytest.raises(ValueError):
        _lib.check(status)
    status = lib.tc_chi2_grad_zheng07_batch_device(
        None, None, 5, 3, 10, 0, _lib.as_double_p(empty), _lib.as_double_p(empty),
        None, None, None, None)
    assert status == _lib.TC_ERR_INVALID
