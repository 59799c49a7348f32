"""The joint of interpolators without a GPU: the joint reference of the tests against central
differences of the oracle's chi2 in (theta, x), the LDS budgets of the joint kernel's two forms and
the argument checks of `JointInterpolator`, which fire before any device is touched."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference  # noqa: E402
import joint_interp_reference as reference  # noqa: E402
import joint_reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

EPS = np.finfo(np.float64).eps
PARTS = [('auto', (3, )), ('cross', (5, ))]
D = 16
SLAB = 64
MAX_AXIS = 32


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def make_interpolator(member, **kwargs):
    from tabcorr_amd import Interpolator, TabCorr
    tables, keys, points = member
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'],
                                    **kwargs) for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)})


def oracle_chi2(members, setups, theta, x, data, precision, modulate):
    xi = np.concatenate([np.ravel(oracle.interpolator_predict_zheng07_batch(
        tables, setup, theta, x, modulate_with_cenocc=modulate)[1][0])
        for (tables, _, _), setup in zip(members, setups)])
    return (xi - data) @ precision @ (xi - data)


def central_differences(members, setups, theta, x, data, precision, h, modulate):
    n_cols = 5 + len(x)
    out = np.zeros(n_cols)
    for k in range(n_cols):
        e = np.zeros(n_cols)
        e[k] = h
        out[k] = (oracle_chi2(members, setups, theta + e[:5], x + e[5:], data, precision,
                              modulate) -
                  oracle_chi2(members, setups, theta - e[:5], x - e[5:], data, precision,
                              modulate)) / (2 * h)
    return out


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
def test_joint_reference_matches_central_differences_of_chi2(modulate, symmetric):
    """|dchi2 - FD(h/2)| <= |FD(h) - FD(h/2)| + 8 eps max|f| / (h/2) in all 5 + D columns, with f
    the oracle's chi2 of the members' concatenated interpolated predictions against a precision
    matrix that couples them -- the step and the bar of
    test_joint_cpu.py::test_joint_reference_matches_central_differences_of_chi2 -- on a grid (4, )
    of [auto (3, ), cross (5, )] with 18 bins, two classes of halo tables."""
    members = reference.make_members((4, ), 9, 1, PARTS, classes='two')
    assert len(members[0][0][0]['gal_type']) == 18
    setups = [oracle.interpolator_setup(tables, points) for tables, _, points in members]
    nodes = np.unique(np.concatenate([grad_reference.nodes_of(t) for t in members[0][0]]))
    thetas = grad_reference.centre_log_m0(synthetic.zheng07_draws(8, seed=5), nodes)
    points = members[0][2]
    rng = np.random.default_rng(3)
    xs = rng.uniform(points.min(axis=0), points.max(axis=0), size=(len(thetas), 1))
    expect = reference.jacobian_batch(members, thetas, xs, modulate=modulate)
    assert expect['xi'].shape == (8, 8) and expect['dxi'].shape == (8, 6, 8)
    data, precision = joint_reference.coupled_data(expect['xi'][3], symmetric)
    assert np.any(precision[:3, 3:] != 0.0)
    chi2, dchi2, _, _ = reference.chi2_reference(expect, data, precision)
    h = 1e-4
    worst = 0.0
    for i, (t, x) in enumerate(zip(thetas, xs)):
        assert np.min(np.abs(nodes - t[2])) > 4 * h
        assert np.min(np.abs(setups[0]['xp'][0] - x[0])) > 4 * h
        value = oracle_chi2(members, setups, t, x, data, precision, modulate)
        assert abs(chi2[i] - value) <= 1e-12 * abs(value) + 1e-12 * np.max(np.abs(chi2))
        coarse = central_differences(members, setups, t, x, data, precision, h, modulate)
        fine = central_differences(members, setups, t, x, data, precision, h / 2, modulate)
        bound = np.abs(coarse - fine) + 8 * EPS * abs(value) / (h / 2)
        worst = max(worst, np.max(np.abs(dchi2[i] - fine) / bound))
        assert np.all(np.abs(dchi2[i] - fine) <= bound), (i, dchi2[i], fine, bound)
    print('worst |dchi2 - FD(h/2)| / bound:', worst)


# ---- the LDS budgets (csrc/joint_interp.h), restated in rows of D doubles ----------------------

def rows_form_bytes(n_bins, n_central, n_r_total, n_r_cross, n_dim, n_params):
    """grad_interp_auto_lds_bytes with N result rows -- one class's rows of w and dw, the totals,
    the weights of every axis, (n_params + 1 + n_dim) accumulators per row -- plus the per-class
    products of the cross members' rows."""
    per_central, per_satellite = {5: (3, 6), 7: (4, 7)}[n_params]
    rows = per_central * n_central + per_satellite * (n_bins - n_central) + 1
    n_q = n_params + 1 + n_dim
    return (rows + (n_params + 1) + 2 * n_dim * MAX_AXIS + n_q * n_r_total +
            n_q * n_r_cross) * D * 8


def slab_form_bytes(n_r_total, n_dim, n_params):
    """grad_interp_cross_lds_bytes with N result rows: one slab and the totals, the class's
    products, the weights and the accumulators."""
    n_q = n_params + 1 + n_dim
    return ((n_params + 1) * (SLAB + 1) + n_q * n_r_total + 2 * n_dim * MAX_AXIS +
            n_q * n_r_total) * D * 8


@pytest.mark.parametrize('n_params', [5, 7])
def test_lds_budgets_of_both_forms(lib, n_params):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    for n_bins, n_central, n_r_total, n_r_cross, n_dim in [
            (18, 9, 8, 5, 1), (36, 18, 8, 5, 2), (32, 16, 8, 5, 1), (36, 18, 11, 2, 1),
            (36, 18, 8, 0, 1), (100, 50, 38, 19, 2), (5, 0, 1, 0, 1), (5, 5, 2, 1, 8)]:
        _lib.check(lib.tc_debug_joint_interp_lds_bytes(1, n_bins, n_central, n_r_total, n_r_cross,
                                                       n_dim, n_params, ctypes.byref(got)))
        assert got.value == rows_form_bytes(n_bins, n_central, n_r_total, n_r_cross, n_dim,
                                            n_params)
        if n_r_cross == 0:
            # no cross member: the budget of the interpolator's own mode-auto kernel with N rows
            same = ctypes.c_int64(-1)
            _lib.check(lib.tc_debug_grad_lds(2, n_params, n_bins, n_central, n_r_total, n_dim, 0,
                                             ctypes.byref(same)))
            assert same.value == got.value
    # the reference's AbacusSummit case among the slab shapes: 1104 bins, N = 26, D = 1
    for n_bins, n_r_total, n_dim in [(1104, 26, 1), (36, 8, 1), (160, 8, 2), (36, 1, 8)]:
        _lib.check(lib.tc_debug_joint_interp_lds_bytes(0, n_bins, n_bins // 2, n_r_total,
                                                       n_r_total, n_dim, n_params,
                                                       ctypes.byref(got)))
        assert got.value == slab_form_bytes(n_r_total, n_dim, n_params)
        same = ctypes.c_int64(-1)
        _lib.check(lib.tc_debug_grad_lds(3, n_params, n_bins, n_bins // 2, n_r_total, n_dim, 0,
                                         ctypes.byref(same)))
        assert same.value == got.value
    assert slab_form_bytes(26, 1, 5) <= 160 * 1024
    for arguments in [(1, 18, 9, 8, 5, 1, 11), (0, 18, 9, 8, 8, 1, 11), (2, 18, 9, 8, 5, 1, 5),
                      (1, 18, 9, 8, 8, 1, 5), (0, 18, 9, 8, 5, 1, 5), (1, 18, 9, 8, 5, 9, 5)]:
        assert lib.tc_debug_joint_interp_lds_bytes(
            *arguments, ctypes.byref(got)) == _lib.TC_ERR_INVALID


# ---- the constructor -----------------------------------------------------------------------------

def test_constructor_refuses_what_is_no_joint_before_any_device():
    from tabcorr_amd import Interpolator, JointInterpolator
    members = reference.make_members((4, ), 9, 1, PARTS, classes='two')
    auto, cross = [make_interpolator(member) for member in members]
    joint = JointInterpolator([auto, cross])
    assert joint.n_r_total == 8 and joint.slices == [slice(0, 3), slice(3, 8)]
    assert joint.keys == list(auto.keys)
    assert JointInterpolator([cross, auto]).slices == [slice(0, 5), slice(5, 8)]
    assert JointInterpolator([cross]).n_r_total == 5

    # a member whose list is a permutation of member 0's is accepted: tables go by grid node
    order = np.array([2, 0, 3, 1])
    shuffled = make_interpolator(reference.permuted(members[1], order))
    assert JointInterpolator([auto, shuffled]).slices == joint.slices

    # the keys in another order (a grid of two axes)
    two = reference.make_members((4, 4), 9, 1, PARTS)
    first = make_interpolator(two[0])
    tables, keys, points = two[1]
    swapped = make_interpolator((tables, keys[::-1], points[:, ::-1]))
    with pytest.raises(ValueError, match='Member 1 .*keys'):
        JointInterpolator([first, swapped])

    # one abscissa moved by one ulp
    tables, keys, points = members[1]
    moved = points.copy()
    moved[moved[:, 0] == np.max(moved[:, 0]), 0] = np.nextafter(np.max(moved[:, 0]), np.inf)
    with pytest.raises(ValueError, match='Member 1 .*abscissae'):
        JointInterpolator([auto, make_interpolator((tables, keys, moved))])

    # n_h of one table at one node moved by 1e-15 relative
    tables = [dict(table) for table in members[1][0]]
    tables[2]['gal_type'] = tables[2]['gal_type'].copy()
    tables[2]['gal_type']['n_h'][4] *= 1.0 + 1e-15
    with pytest.raises(ValueError, match='Member 1.*table 2 .*gal_type'):
        JointInterpolator([auto, make_interpolator((tables, keys, points))])
    # ... found through the permutation too: list position 1 is grid node 0
    tables = [dict(table) for table in reference.permuted(members[1], order)[0]]
    tables[1]['gal_type'] = tables[1]['gal_type'].copy()
    tables[1]['gal_type']['n_h'][4] *= 1.0 + 1e-15
    with pytest.raises(ValueError, match='Member 1.*table 1 .*gal_type'):
        JointInterpolator([auto, make_interpolator((tables, keys, points[order]))])

    with pytest.raises(ValueError, match='Member 1.*float64'):
        JointInterpolator([auto, make_interpolator(members[1], compute_dtype='float32')])
    with pytest.raises(ValueError, match='Member 2 .*twice'):
        JointInterpolator([auto, cross, auto])
    with pytest.raises(ValueError, match='1 to 16 interpolators'):
        JointInterpolator([])
    many = [make_interpolator(members[k % 2]) for k in range(17)]
    with pytest.raises(ValueError, match='1 to 16 interpolators'):
        JointInterpolator(many)
    assert len(JointInterpolator(many[:16]).slices) == 16
    with pytest.raises(ValueError, match='Member 1 .*Interpolator'):
        JointInterpolator([auto, auto.tabcorr_list[0]])
    for interp in [auto, cross, shuffled, first, swapped] + many:
        assert isinstance(interp, Interpolator) and interp._device is None
        assert all(halotab._device is None for halotab in interp.tabcorr_list)


def make_joint():
    from tabcorr_amd import JointInterpolator
    members = reference.make_members((4, ), 9, 1, PARTS)
    interpolators = [make_interpolator(member) for member in members]
    return JointInterpolator(interpolators), interpolators, members[0][2]


def test_calls_refuse_wrong_shapes_before_any_device():
    joint, interpolators, points = make_joint()
    theta = synthetic.zheng07_draws(3, seed=2)
    x = np.tile(points.mean(axis=0), (3, 1))
    good_data, good_precision = np.zeros(8), np.eye(8)
    for data, precision in ((np.zeros(7), good_precision), (np.zeros(9), good_precision),
                            (np.zeros((8, 2)), good_precision),
                            ([np.zeros(3), np.zeros(4)], good_precision),
                            ([np.zeros(5), np.zeros(3)], good_precision),
                            (good_data, np.eye(5)), (good_data, np.ones((8, 9))),
                            (good_data, np.ones(64)), (good_data, np.ones((8, 8, 1)))):
        for call in (joint.chi2_grad_batch, joint.chi2_fisher_batch):
            with pytest.raises(ValueError, match='data'):
                call(theta, x, data, precision)
    with pytest.raises(ValueError, match='precision'):
        joint.fisher_batch(theta, x, np.eye(3))
    for columns in (4, 7):
        with pytest.raises(ValueError, match='theta'):
            joint.predict_batch_grad(np.zeros((3, columns)), x)
        with pytest.raises(ValueError, match='theta'):
            joint.chi2_grad_batch(np.zeros((3, columns)), x, good_data, good_precision)
    with pytest.raises(ValueError, match='theta'):
        joint.predict_batch_grad(theta, x, assembias=True)
    for bad_x in (x[:2], np.hstack([x, x]), np.zeros((3, 0))):
        with pytest.raises(ValueError, match='x must have shape'):
            joint.predict_batch_grad(theta, bad_x)
        with pytest.raises(ValueError, match='x must have shape'):
            joint.chi2_fisher_batch(theta, bad_x, good_data, good_precision)
    for value in (points.min() - 0.01, points.max() + 0.01, np.nan):
        outside = x.copy()
        outside[1, 0] = value
        with pytest.raises(ValueError, match='extrapolation'):
            joint.predict_batch_grad(theta, outside)
        with pytest.raises(ValueError, match='extrapolation'):
            joint.fisher_batch(theta, outside, good_precision)
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.predict_batch_grad(np.zeros((3, 14)), x, family='leauthaud11')
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.chi2_fisher_batch(np.zeros((3, 14)), x, good_data, good_precision,
                                family='leauthaud11')
    assert joint._device is None
    for interp in interpolators:
        assert interp._device is None
        assert all(halotab._device is None for halotab in interp.tabcorr_list)


def test_un_batched_forms_refuse_models_the_device_does_not_serve():
    from tabcorr_amd import Leauthaud11Model, Zheng07Model
    joint, _, points = make_joint()
    model = Zheng07Model(redshift=0.0)
    with pytest.raises(ValueError, match=joint.keys[0]):
        joint.predict_grad(model, check_consistency=False)
    other = Leauthaud11Model()
    other.param_dict[joint.keys[0]] = points.mean()
    with pytest.raises(NotImplementedError):
        joint.predict_grad(other, check_consistency=False)
    model.param_dict[joint.keys[0]] = points.mean()
    with pytest.raises(ValueError, match='assembias'):
        joint.chi2_fisher(model, np.zeros(8), np.eye(8), check_consistency=False, assembias=True)
    model.param_dict[joint.keys[0]] = points.max() + 1.0
    with pytest.raises(ValueError, match='extrapolation'):
        joint.predict_grad(model, check_consistency=False)
    assert joint._device is None


def test_c_entry_points_refuse_a_call_without_a_handle(lib):
    from tabcorr_amd import _lib
    empty = np.zeros(0)
    p = _lib.as_double_p(empty)
    assert lib.tc_joint_interp_predict_grad_batch(None, p, 5, p, 3, 10, 0, p, p, p,
                                                  p) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_interp_chi2_grad_batch(None, p, 5, p, 3, 10, 0, p, p, p, p, p, p,
                                               None) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_interp_predict_grad_batch_device(
        None, None, 5, None, 3, 10, 0, None, None, None, None) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_interp_chi2_grad_batch_device(
        None, None, 5, None, 3, 10, 0, p, p, None, None, None, None, None) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_interp_synchronize(None) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_interp_info(None, None, None, None, None) == _lib.TC_ERR_INVALID
    handle = ctypes.c_void_p()
    assert lib.tc_joint_interp_create(None, 2, ctypes.byref(handle)) == _lib.TC_ERR_INVALID
    members = (ctypes.c_void_p * 17)()
    for count in (17, 0):
        assert lib.tc_joint_interp_create(members, count,
                                          ctypes.byref(handle)) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_interp_create(members, 2, ctypes.byref(handle)) == _lib.TC_ERR_INVALID
    assert b'member 0 is NULL' in lib.tc_last_error()
    assert lib.tc_joint_interp_destroy(None) == _lib.TC_OK
