"""The joint likelihood of several tables without a GPU: the joint reference of the tests against
central differences of the oracle's chi2, the LDS budget of the joint kernel and the argument
checks of `JointLikelihood`, which fire before any device is touched."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference  # noqa: E402
import joint_reference  # noqa: E402
from derivative_kit import chi2_data  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

EPS = np.finfo(np.float64).eps
PARTS = [('auto', (3, )), ('cross', (5, ))]


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def make_halotabs(tables, **kwargs):
    from tabcorr_amd import TabCorr
    return [TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                table['attrs'], **kwargs) for table in tables]


def oracle_chi2(tables, theta, data, precision, modulate):
    xi = np.concatenate([np.ravel(oracle.predict_zheng07(
        table, theta, modulate_with_cenocc=modulate)[1]) for table in tables])
    return (xi - data) @ precision @ (xi - data)


def central_differences(tables, theta, data, precision, h, modulate):
    out = np.zeros(5)
    for k in range(5):
        e = np.zeros(5)
        e[k] = h
        out[k] = (oracle_chi2(tables, theta + e, data, precision, modulate) -
                  oracle_chi2(tables, theta - e, data, precision, modulate)) / (2 * h)
    return out


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
def test_joint_reference_matches_central_differences_of_chi2(modulate, symmetric):
    """|dchi2 - FD(h/2)| <= |FD(h) - FD(h/2)| + 8 eps max|f| / (h/2) with f the oracle's chi2 of
    the concatenated prediction against a precision matrix that couples the tables (the bound of
    test_grad_cpu.py: no free tolerance); the values of the reference are the oracle's."""
    tables = joint_reference.make_tables(9, 2, PARTS)
    nodes = grad_reference.nodes_of(tables[0])
    thetas = grad_reference.centre_log_m0(synthetic.zheng07_draws(12, seed=5), nodes)
    reference = joint_reference.jacobian_batch(tables, thetas, modulate=modulate)
    assert reference[1].shape == (12, 8) and reference[3].shape == (12, 5, 8)
    data, precision = chi2_data(reference[1][3], symmetric)
    assert np.any(precision[:3, 3:] != 0.0)
    chi2, dchi2, _, _ = joint_reference.chi2_reference(reference, data, precision)
    h = 1e-4
    worst = 0.0
    for i, t in enumerate(thetas):
        assert np.min(np.abs(nodes - t[2])) > 4 * h
        value = oracle_chi2(tables, t, data, precision, modulate)
        assert abs(chi2[i] - value) <= 1e-12 * abs(value) + 1e-12 * np.max(np.abs(chi2))
        coarse = central_differences(tables, t, data, precision, h, modulate)
        fine = central_differences(tables, t, data, precision, h / 2, modulate)
        bound = np.abs(coarse - fine) + 8 * EPS * abs(value) / (h / 2)
        worst = max(worst, np.max(np.abs(dchi2[i] - fine) / bound))
        assert np.all(np.abs(dchi2[i] - fine) <= bound), (i, dchi2[i], fine, bound)
    print('worst |dchi2 - FD(h/2)| / bound:', worst)


def grad_auto_lds_bytes(n_bins, n_central, n_r, chi2, n_params):
    """grad.h: grad_auto_lds_bytes."""
    per_central, per_satellite = {5: (3, 6), 7: (4, 7)}[n_params]
    rows = per_central * n_central + per_satellite * (n_bins - n_central) + 1
    return (rows + (n_params + 1) + ((n_params + 1) * n_r if chi2 else 0)) * 16 * 8


@pytest.mark.parametrize('n_params', [5, 7])
def test_joint_lds_budget_is_that_of_the_auto_kernel_with_all_rows(lib, n_params):
    from tabcorr_amd import _lib
    for n_bins, n_central, n_r_total in [(18, 9, 8), (36, 18, 8), (60, 30, 38), (200, 100, 50),
                                         (5, 0, 1), (5, 5, 1)]:
        for chi2 in (0, 1):
            got = ctypes.c_int64(-1)
            _lib.check(lib.tc_debug_joint_lds_bytes(n_bins, n_central, n_r_total, chi2, n_params,
                                                    ctypes.byref(got)))
            assert got.value == grad_auto_lds_bytes(n_bins, n_central, n_r_total, chi2, n_params)
            same = ctypes.c_int64(-1)
            _lib.check(lib.tc_debug_grad_lds(0, n_params, n_bins, n_central, n_r_total, 0, chi2,
                                             ctypes.byref(same)))
            assert same.value == got.value
    assert lib.tc_debug_joint_lds_bytes(18, 9, 8, 1, 11, ctypes.byref(got)) == _lib.TC_ERR_INVALID


def test_constructor_refuses_what_is_no_joint_before_any_device():
    from tabcorr_amd import JointLikelihood
    tables = joint_reference.make_tables(9, 2, PARTS)
    auto, cross = make_halotabs(tables)
    joint = JointLikelihood([auto, cross])
    assert joint.n_r_total == 8 and joint.slices == [slice(0, 3), slice(3, 8)]
    assert JointLikelihood([cross, auto]).slices == [slice(0, 5), slice(5, 8)]
    # another halo table: more bins, and the same bins with one n_h moved
    other = make_halotabs([synthetic.synthetic_table(9, 1, (5, ), 'cross', seed=3)])[0]
    with pytest.raises(ValueError, match='Table 1 .*gal_type'):
        JointLikelihood([auto, other])
    moved = dict(tables[1])
    moved['gal_type'] = tables[1]['gal_type'].copy()
    moved['gal_type']['n_h'][4] *= 1.0 + 1e-15
    with pytest.raises(ValueError, match='Table 2 .*gal_type'):
        JointLikelihood([auto, cross] + make_halotabs([moved]))
    with pytest.raises(ValueError, match='Table 2 .*twice'):
        JointLikelihood([auto, cross, auto])
    with pytest.raises(ValueError, match='1 to 16 tables'):
        JointLikelihood(make_halotabs(tables * 9)[:17])
    with pytest.raises(ValueError, match='1 to 16 tables'):
        JointLikelihood([])
    assert len(JointLikelihood(make_halotabs(tables * 8)).slices) == 16
    with pytest.raises(ValueError, match='Table 1 .*float64'):
        JointLikelihood([auto] + make_halotabs(tables[1:], compute_dtype='float32'))
    for halotab in (auto, cross, other):
        assert halotab._device is None


def test_calls_refuse_wrong_shapes_before_any_device():
    from tabcorr_amd import JointLikelihood
    halotabs = make_halotabs(joint_reference.make_tables(9, 2, PARTS))
    joint = JointLikelihood(halotabs)
    theta = synthetic.zheng07_draws(3, seed=2)
    good_data, good_precision = np.zeros(8), np.eye(8)
    for data, precision in ((np.zeros(7), good_precision), (np.zeros(9), good_precision),
                            (np.zeros((8, 2)), good_precision),
                            ([np.zeros(3), np.zeros(4)], good_precision),
                            ([np.zeros(5), np.zeros(3)], good_precision),
                            (good_data, np.eye(5)), (good_data, np.ones((8, 9))),
                            (good_data, np.ones(64)), (good_data, np.ones((8, 8, 1)))):
        for call in (joint.chi2_grad_batch, joint.chi2_fisher_batch):
            with pytest.raises(ValueError, match='data'):
                call(theta, data, precision)
    with pytest.raises(ValueError, match='precision'):
        joint.fisher_batch(theta, np.eye(3))
    for columns in (4, 7):
        with pytest.raises(ValueError, match='theta'):
            joint.predict_batch_grad(np.zeros((3, columns)))
        with pytest.raises(ValueError, match='theta'):
            joint.chi2_grad_batch(np.zeros((3, columns)), good_data, good_precision)
    with pytest.raises(ValueError, match='theta'):
        joint.predict_batch_grad(theta, assembias=True)
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.predict_batch_grad(np.zeros((3, 14)), family='leauthaud11')
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.chi2_fisher_batch(np.zeros((3, 14)), good_data, good_precision,
                                family='leauthaud11')
    assert joint._device is None and all(halotab._device is None for halotab in halotabs)


def test_un_batched_forms_refuse_models_the_device_does_not_serve():
    from tabcorr_amd import JointLikelihood, Leauthaud11Model, Zheng07Model
    joint = JointLikelihood(make_halotabs(joint_reference.make_tables(9, 2, PARTS)))
    with pytest.raises(NotImplementedError):
        joint.predict_grad(Leauthaud11Model(), check_consistency=False)
    with pytest.raises(NotImplementedError):
        joint.chi2_fisher(object(), np.zeros(8), np.eye(8), check_consistency=False)
    with pytest.raises(ValueError, match='assembias'):
        joint.predict_grad(Zheng07Model(), check_consistency=False, assembias=True)
    assert joint._device is None


def test_c_entry_points_refuse_a_call_without_a_handle(lib):
    from tabcorr_amd import _lib
    empty = np.zeros(0)
    p = _lib.as_double_p(empty)
    assert lib.tc_joint_predict_grad_batch(None, p, 5, 3, 10, 0, p, p, p, p) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_chi2_grad_batch(None, p, 5, 3, 10, 0, p, p, p, p, p, p,
                                        None) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_synchronize(None) == _lib.TC_ERR_INVALID
    handle = ctypes.c_void_p()
    assert lib.tc_joint_create(None, 2, ctypes.byref(handle)) == _lib.TC_ERR_INVALID
    tables = (ctypes.c_void_p * 17)()
    assert lib.tc_joint_create(tables, 17, ctypes.byref(handle)) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_create(tables, 0, ctypes.byref(handle)) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_create(tables, 2, ctypes.byref(handle)) == _lib.TC_ERR_INVALID
    assert b'table 0 is NULL' in lib.tc_last_error()
    assert lib.tc_joint_destroy(None) == _lib.TC_OK
