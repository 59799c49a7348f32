"""The joint of interpolators on the device (`JointInterpolator`, the tc_joint_interp_* entry
points, grad_joint_interp_kernel) against the reference of joint_interp_reference.py, the members'
own `Interpolator` calls and the oracle.  Needs an MI355X.

Allowances are the suite's own, no new number: 1e-10 relative plus 1e-10 of the scale of the terms
that cancel (interp_grad_reference), carried through chi2 and the Fisher matrix by the formulas of
joint_reference and fisher_reference.  Every case prints its largest error in units of its
allowance.  Shapes are the smallest at which each path can go wrong; draw counts 1, 17 and 35: a
partial workgroup and several workgroups.
"""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assembias_grad_reference  # noqa: E402
import grad_reference  # noqa: E402
import joint_interp_reference as reference  # noqa: E402
import joint_reference  # noqa: E402
import test_gpu_interp_grad as interp_suite  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import D, LDS_LIMIT, RTOL, device_call, largest, same_bits  # noqa: E402
from util import assert_rel  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAW_COUNTS = [1, D + 1, 2 * D + 3]
N_MAX = max(DRAW_COUNTS)

AUTO_CROSS = (('auto', (3, )), ('cross', (5, )))
CROSS_CROSS = (('cross', (5, )), ('cross', (3, )))
# name -> (parts, grid, n_prim, n_sec, classes): the rows form with 18 bins (a second row tile of
# two rows), 36 bins on a 2-D grid with two classes of halo tables, 32 bins with the cross member
# first, and 9 auto rows over 4 waves with a cross member between them; the slab form with 36 bins
# and with 160 bins on a 2-D grid: three slabs, the last one partial
SHAPES = {
    'rows-18': (AUTO_CROSS, (4, ), 9, 1, 'one'),
    'rows-36-4x4': (AUTO_CROSS, (4, 4), 9, 2, 'two'),
    'rows-32-cross-first': ((('cross', (5, )), ('auto', (3, ))), (4, ), 16, 1, 'one'),
    'rows-36-three': ((('auto', (3, )), ('cross', (2, )), ('auto', (6, ))), (4, ), 18, 1, 'two'),
    'slabs-36': (CROSS_CROSS, (4, ), 18, 1, 'two'),
    'slabs-160-4x4': (CROSS_CROSS, (4, 4), 40, 2, 'two'),
    # two secondary bins for the decorated model
    'rows-36-sec': (AUTO_CROSS, (4, ), 9, 2, 'two'),
    'slabs-36-sec': (CROSS_CROSS, (4, ), 9, 2, 'two'),
}

_cases = {}


def make_interpolator(member, **kwargs):
    from tabcorr_amd import Interpolator, TabCorr
    tables, keys, points = member
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'],
                                    **kwargs) for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)})


def get_case(name, modulate=False, assembias=False, x_kind='inside'):
    """Members, their interpolators, the joint, draws (theta, x) and their reference, made once per
    combination and never modified: a batch of n draws is the first n of them.  The seed of the
    draws is the first one from 5 on with which every draw has only finite reference results,
    chosen from the reference alone (test_gpu_interp_grad.get_case; decorated: the condition of
    test_gpu_assembias_grad.get_interp_case on the rounding of the central columns with it)."""
    from tabcorr_amd import JointInterpolator
    key = (name, modulate, assembias, x_kind)
    if key not in _cases:
        parts, grid, n_prim, n_sec, classes = SHAPES[name]
        members = reference.make_members(grid, n_prim, n_sec, parts, classes, assembias=assembias)
        tables, _, points = members[0]
        setup = oracle.interpolator_setup(tables, points)
        nodes = np.unique(np.concatenate([grad_reference.nodes_of(t) for t in tables]))
        for seed in range(5, 25):
            if assembias:
                theta = assembias_grad_reference.stress_draws(tables[0], N_MAX, seed=seed)
            else:
                theta = grad_reference.centre_log_m0(
                    grad_reference.stress_draws(tables[0], N_MAX, seed=seed), nodes)
            x = interp_suite.make_x(points, setup, N_MAX, x_kind, seed)

            def compute(shared=True):
                with np.errstate(all='ignore'):
                    return reference.jacobian_batch(members, theta, x, 10, modulate, assembias,
                                                    shared)

            expect = compute()
            if not reference.usable(expect):
                continue
            allowance = RTOL * (np.abs(expect['dxi']) + expect['dxi_scale'])
            if not assembias or assembias_grad_reference.rounding_of_centrals(
                    lambda: compute(False)['dxi'], expect['dxi'], allowance) <= 0.1:
                break
        else:
            raise AssertionError('no seed gives usable draws for %s' % (key, ))
        for array in [theta, x] + list(expect.values()):
            array.setflags(write=False)
        interpolators = [make_interpolator(member) for member in members]
        _cases[key] = {
            'members': members, 'interpolators': interpolators,
            'joint': JointInterpolator(interpolators), 'theta': theta, 'x': x,
            'reference': expect,
            'options': {'modulate_with_cenocc': modulate, 'assembias': assembias,
                        'extrapolate': x_kind == 'outside'}}
    return _cases[key]


def operands(case, symmetric):
    """A data vector near draw 3's joint vector and a dense precision matrix whose off-diagonal
    blocks couple the members."""
    joint = case['joint']
    data, precision = joint_reference.coupled_data(case['reference']['xi'][3], symmetric)
    first = joint.slices[0]
    assert len(joint.slices) == 1 or np.any(precision[first, first.stop:] != 0.0)
    return data, precision


def check_case(case, n, what):
    """Prediction, chi2 (symmetric and non-symmetric coupled precision) and Fisher matrix of the
    first n draws against the reference; ngal and xi against the members' forward calls."""
    joint, options = case['joint'], case['options']
    theta, x = case['theta'][:n], case['x'][:n]
    n_cols = theta.shape[1] + x.shape[1]
    expect = reference.first(case['reference'], n)
    got = joint.predict_batch_grad(theta, x, **options)
    assert got[0].shape == (n, ) and got[2].shape == (n, n_cols)
    for part, interp in zip(got[1], case['interpolators']):
        assert part.shape == (n, ) + tuple(interp.tabcorr_list[0].tpcf_shape)
    for part, interp in zip(got[3], case['interpolators']):
        assert part.shape == (n, n_cols) + tuple(interp.tabcorr_list[0].tpcf_shape)
    reference.check_prediction(reference.flat(got, joint.n_r_total), expect, what)
    for xi, interp in zip(got[1], case['interpolators']):
        ngal, forward = interp.predict_batch(theta, x, **options)
        assert_rel(got[0], ngal, RTOL, what + ' ngal against predict_batch')
        assert_rel(xi, forward, RTOL, what + ' xi against predict_batch')
    for symmetric in (True, False):
        data, precision = operands(case, symmetric)
        label = '%s %s' % (what, 'spd' if symmetric else 'nonsymmetric')
        full = joint.chi2_fisher_batch(theta, x, data, precision, **options)
        assert full[4].shape == (n, n_cols, n_cols)
        reference.check_chi2(full, expect, data, precision, 'chi2 ' + label)
        reference.check_fisher(full[4], expect, precision, 'fisher ' + label)
        gradient = joint.chi2_grad_batch(theta, x, [data[part] for part in joint.slices],
                                         precision, **options)
        assert len(gradient) == 4 and same_bits(full[:4], gradient)
        forecast = joint.fisher_batch(theta, x, precision, **options)
        assert same_bits(forecast, (full[0], full[2], full[4]))
    return got


MAIN = ['rows-18', 'rows-36-4x4', 'rows-32-cross-first', 'rows-36-three', 'slabs-36',
        'slabs-160-4x4']


@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('name', MAIN)
def test_joint_matches_reference(name, n_draws):
    check_case(get_case(name), n_draws, '%s n=%d' % (name, n_draws))


@pytest.mark.parametrize('name', ['rows-18', 'slabs-36'])
def test_modulate_with_cenocc(name):
    check_case(get_case(name, modulate=True), D + 1, '%s modulate' % name)


@pytest.mark.parametrize('name', ['rows-36-sec', 'slabs-36-sec'])
def test_assembias(name):
    """The decorated model: 7 + D columns."""
    case = get_case(name, modulate=(name == 'rows-36-sec'), assembias=True)
    got = check_case(case, D + 1, '%s assembias' % name)
    assert got[2].shape[1] == 8


@pytest.mark.parametrize('x_kind', ['node', 'knot', 'last', 'outside'])
def test_positions_of_x(x_kind):
    """On a grid node, on an interior knot, on the last knot, outside the grid on both sides with
    extrapolate=True."""
    case = get_case('rows-36-4x4', x_kind=x_kind)
    check_case(case, N_MAX, 'rows-36-4x4 x=%s' % x_kind)
    if x_kind == 'outside':
        with pytest.raises(ValueError, match='extrapolation'):
            case['joint'].predict_batch_grad(case['theta'], case['x'])


# ---- bits ----------------------------------------------------------------------------------------

def all_forms(handle, case, n, data, precision):
    """Prediction, chi2 and chi2 with Fisher of the first n draws through `handle` (a joint or an
    interpolator), flattened to plain arrays."""
    theta, x, options = case['theta'][:n], case['x'][:n], case['options']
    predicted = handle.predict_batch_grad(theta, x, **options)
    if isinstance(predicted[1], list):
        predicted = reference.flat(predicted, handle.n_r_total)
    else:
        predicted = (predicted[0], predicted[1].reshape(n, -1), predicted[2],
                     predicted[3].reshape(n, predicted[2].shape[1], -1))
    return (predicted, handle.chi2_grad_batch(theta, x, data, precision, **options),
            handle.chi2_fisher_batch(theta, x, data, precision, **options))


@pytest.mark.parametrize('name,member', [('rows-18', 0), ('slabs-36', 0), ('rows-36-sec', 0)],
                         ids=['auto', 'cross', 'auto-assembias'])
def test_joint_of_one_member_returns_that_members_bits(name, member):
    """Prediction, chi2 and Fisher: the pieces and their order are the interpolator kernels'."""
    from tabcorr_amd import JointInterpolator
    case = get_case(name, assembias=name.endswith('sec'), modulate=name.endswith('sec'))
    interp = case['interpolators'][member]
    part = case['joint'].slices[member]
    data, precision = joint_reference.coupled_data(case['reference']['xi'][3][part], False)
    alone = JointInterpolator([interp])
    for n in DRAW_COUNTS:
        mine = all_forms(alone, case, n, data, precision)
        theirs = all_forms(interp, case, n, data, precision)
        for a, b in zip(mine, theirs):
            assert same_bits(a, b), (name, n)


@pytest.mark.parametrize('name', ['rows-18', 'rows-36-three', 'rows-36-4x4', 'slabs-36',
                                  'slabs-160-4x4'])
def test_member_rows_carry_the_members_own_bits(name):
    """Prediction form: the rows of an auto member in any joint and of every member of an all-cross
    joint are those of the member's own predict_batch_grad (the lists agree node for node);
    ngal and dngal are member 0's."""
    case = get_case(name)
    joint, n = case['joint'], N_MAX
    got = joint.predict_batch_grad(case['theta'], case['x'])
    all_cross = name.startswith('slabs')
    checked = 0
    for m, interp in enumerate(case['interpolators']):
        own = interp.predict_batch_grad(case['theta'], case['x'])
        if m == 0:
            assert same_bits((got[0], got[2]), (own[0], own[2]))
        if all_cross or interp.tabcorr_list[0].attrs['mode'] == 'auto':
            assert same_bits((got[1][m], got[3][m]), (own[1], own[3])), (name, m)
            checked += 1
        else:
            assert_rel(got[1][m], own[1], RTOL)
    assert checked >= 1 and n == len(got[0])


@pytest.mark.parametrize('name', ['rows-36-4x4', 'slabs-36'])
def test_a_permuted_member_changes_nothing(name):
    """A member whose list is a fixed permutation of member 0's: the walk is member 0's either
    way, the results are the unpermuted joint's bit for bit, in every form."""
    from tabcorr_amd import JointInterpolator
    case = get_case(name)
    members = case['members']
    order = np.random.default_rng(9).permutation(len(members[0][0]))
    assert np.any(order != np.arange(len(order)))
    shuffled = make_interpolator(reference.permuted(members[1], order))
    joint = JointInterpolator([case['interpolators'][0], shuffled])
    data, precision = operands(case, False)
    n = D + 1
    for a, b in zip(all_forms(joint, case, n, data, precision),
                    all_forms(case['joint'], case, n, data, precision)):
        assert same_bits(a, b)


def device_entries(joint, theta, x, data, precision, flags=0):
    """The `_device` entries: prediction, and chi2 with the Fisher matrix."""
    from tabcorr_amd import _lib
    device = joint.to_device()
    n, n_r, n_cols = len(theta), joint.n_r_total, theta.shape[1] + x.shape[1]
    arguments = [theta, theta.shape[1], x, n, 10, flags]
    predicted = device_call(device, 'tc_joint_interp_predict_grad_batch_device', arguments,
                            [n, (n, n_r), (n, n_cols), (n, n_cols, n_r)],
                            'tc_joint_interp_synchronize')
    data, precision = _lib.contiguous(data), _lib.contiguous(precision)
    likelihood = device_call(device, 'tc_joint_interp_chi2_grad_batch_device',
                             arguments + [_lib.as_double_p(data), _lib.as_double_p(precision)],
                             [n, n, (n, n_cols), (n, n_cols), (n, n_cols, n_cols)],
                             'tc_joint_interp_synchronize')
    return predicted, likelihood


@pytest.mark.parametrize('name', ['rows-36-three', 'slabs-160-4x4'])
def test_batch_invariance_and_device_entries(name):
    """A draw's results are bit-equal in batches of 1, 17 and 35 draws, alone or among others, and
    between the host-array and the device-pointer entry points; three device-pointer calls in a
    row also use member 0's lanes in turn."""
    case = get_case(name)
    joint, theta, x = case['joint'], case['theta'], case['x']
    data, precision = operands(case, False)
    full = all_forms(joint, case, N_MAX, data, precision)
    assert all(np.all(np.isfinite(a)) for form in full for a in form)
    for n in DRAW_COUNTS:
        part = all_forms(joint, case, n, data, precision)
        for a, b in zip(part, full):
            assert same_bits(a, [c[:n] for c in b]), (name, n)
        predicted, likelihood = device_entries(joint, theta[:n], x[:n], data, precision)
        assert same_bits(predicted, part[0]) and same_bits(likelihood, part[2])
    # every draw of the largest batch alone (column 0 of its workgroup)
    for k in range(N_MAX):
        alone = joint.chi2_fisher_batch(theta[k:k + 1], x[k:k + 1], data, precision)
        assert same_bits(alone, [c[k:k + 1] for c in full[2]]), (name, k)
        alone = reference.flat(joint.predict_batch_grad(theta[k:k + 1], x[k:k + 1]),
                               joint.n_r_total)
        assert same_bits(alone, [c[k:k + 1] for c in full[0]]), (name, k)


@pytest.mark.parametrize('name', ['rows-18', 'slabs-36'])
def test_block_diagonal_precision_is_the_sum_of_the_members(name):
    """Without coupling chi2 and dchi2 are the sums of the members' own chi2_grad_batch results:
    each side lies within its allowance (joint_reference.chi2_reference) of the same reference."""
    case = get_case(name)
    joint, theta, x = case['joint'], case['theta'], case['x']
    expect = case['reference']
    data, dense = operands(case, False)
    precision = np.zeros_like(dense)
    for part in joint.slices:
        precision[part, part] = dense[part, part]
    got = joint.chi2_fisher_batch(theta, x, data, precision)
    _, _, chi2_allow, dchi2_allow = reference.chi2_reference(expect, data, precision)
    chi2, dchi2 = np.zeros(N_MAX), np.zeros_like(got[3])
    for part, interp in zip(joint.slices, case['interpolators']):
        own = interp.chi2_grad_batch(theta, x, data[part], precision[part, part])
        chi2 += own[1]
        dchi2 += own[3]
        block = dict(expect)
        for name_ in ('xi', 'dxi', 'dxi_scale'):
            block[name_] = expect[name_][..., part]
        allow = reference.chi2_reference(block, data[part], precision[part, part])
        chi2_allow = chi2_allow + allow[2]
        dchi2_allow = dchi2_allow + allow[3]
    print('%s: max |joint - sum| / allowance = %.3g (chi2), %.3g (dchi2)' % (
        name, np.max(np.abs(got[1] - chi2) / chi2_allow),
        np.max(np.abs(got[3] - dchi2) / np.maximum(dchi2_allow, 1e-300))))
    assert np.all(np.abs(got[1] - chi2) <= chi2_allow)
    assert np.all(np.abs(got[3] - dchi2) <= dchi2_allow)
    assert np.array_equal(got[4], got[4].transpose(0, 2, 1))


def test_reference_fixture_in_the_slab_form():
    """The reference's AbacusSummit interpolator (4 tables of 1104 bins, mode cross) joined with a
    second member made of the same tables (the first five r rows, times 3): 17 draws in the slab
    form, every member's rows bit for bit those of its own predict_batch_grad."""
    from tabcorr_amd import Interpolator, JointInterpolator, TabCorr
    first = Interpolator.read(os.path.join(REPO, 'tests', 'golden', 'ds_efficient.hdf5'))
    assert len(first.tabcorr_list) == 4 and len(first.tabcorr_list[0].gal_type) == 1104
    assert first.tabcorr_list[0].attrs['mode'] == 'cross'
    halotabs = [TabCorr.from_arrays(t.gal_type, 3.0 * np.asarray(t.tpcf_matrix)[:5], (5, ),
                                    t.attrs) for t in first.tabcorr_list]
    second = Interpolator(halotabs, {key: first.points[:, d] for d, key in enumerate(first.keys)})
    joint = JointInterpolator([first, second])
    n_r = len(first.tabcorr_list[0].tpcf_matrix)
    assert joint.n_r_total == n_r + 5
    n = D + 1
    rng = np.random.default_rng(5)
    theta = synthetic.zheng07_draws(n, seed=9)
    theta[:, 0] = rng.uniform(12.5, 13.3, n)
    theta[:, 3] = rng.uniform(13.6, 14.4, n)
    x = np.stack([rng.uniform(xp[0], xp[-1], n) for xp in first.xp], axis=-1)
    got = joint.predict_batch_grad(theta, x)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[2]))
    for m, interp in enumerate((first, second)):
        own = interp.predict_batch_grad(theta, x)
        assert np.all(np.isfinite(own[1])) and np.all(np.isfinite(own[3]))
        assert same_bits((got[1][m], got[3][m]), (own[1], own[3])), m
        if m == 0:
            assert same_bits((got[0], got[2]), (own[0], own[2]))
    ngal, xi = first.predict_batch(theta, x)
    assert_rel(got[0], ngal, RTOL)
    assert_rel(got[1][0], xi, RTOL, floor=1e-12)


# ---- refusals ------------------------------------------------------------------------------------

def debug_bytes(form, n_bins, n_central, n_r_total, n_r_cross, n_dim, n_params=5):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    _lib.check(_lib.load().tc_debug_joint_interp_lds_bytes(
        form, n_bins, n_central, n_r_total, n_r_cross, n_dim, n_params, ctypes.byref(got)))
    return got.value


def check_still_serves(joint, members, theta, x):
    """The joint's prediction and each member's predict_batch match the oracle."""
    got = joint.predict_batch_grad(theta, x)
    for m, ((tables, _, points), interp) in enumerate(zip(members, joint.interpolators)):
        setup = oracle.interpolator_setup(tables, points)
        expect = oracle.interpolator_predict_zheng07_batch(tables, setup, theta, x)
        ngal, xi = interp.predict_batch(theta, x)
        assert_rel(ngal, expect[0], RTOL)
        assert_rel(xi, expect[1], RTOL)
        assert_rel(got[0], expect[0], RTOL)
        assert_rel(got[1][m], expect[1], RTOL)


def test_lds_limit_agrees_with_the_debug_symbol():
    """Rows form, a grid (4, ) over 18 bins, [auto (R, ), cross (5, )]: the largest R whose budget
    the debug symbol puts within 160 KiB is served in every form, R + 1 is refused by every form
    with NotImplementedError naming LDS, and everything goes on serving."""
    from tabcorr_amd import JointInterpolator
    n_rows = largest(lambda r: debug_bytes(1, 18, 9, r + 5, 5, 1) <= LDS_LIMIT)
    assert debug_bytes(1, 18, 9, n_rows + 6, 5, 1) > LDS_LIMIT
    theta = synthetic.zheng07_draws(5, seed=2)

    def build(rows):
        members = reference.make_members((4, ), 9, 1, [('auto', (rows, )), ('cross', (5, ))])
        interpolators = [make_interpolator(member) for member in members]
        return JointInterpolator(interpolators), members

    joint, members = build(n_rows)
    x = interp_suite.make_x(members[0][2], None, 5, 'inside', 2)
    n = joint.n_r_total
    assert n == n_rows + 5
    check_still_serves(joint, members, theta, x)
    own = joint.interpolators[0].predict_batch_grad(theta, x)
    got = joint.predict_batch_grad(theta, x)
    assert same_bits((got[1][0], got[3][0]), (own[1], own[3]))
    full = joint.chi2_fisher_batch(theta, x, np.zeros(n), np.eye(n))
    assert all(np.all(np.isfinite(a)) for a in full)

    refused, refused_members = build(n_rows + 1)
    n = refused.n_r_total
    with pytest.raises(NotImplementedError, match='LDS'):
        refused.predict_batch_grad(theta, x)
    with pytest.raises(NotImplementedError, match='LDS'):
        refused.chi2_grad_batch(theta, x, np.zeros(n), np.eye(n))
    with pytest.raises(NotImplementedError, match='LDS'):
        refused.fisher_batch(theta, x, np.eye(n))
    for (tables, _, points), interp in zip(refused_members, refused.interpolators):
        setup = oracle.interpolator_setup(tables, points)
        expect = oracle.interpolator_predict_zheng07_batch(tables, setup, theta, x)
        ngal, xi = interp.predict_batch(theta, x)
        assert_rel(ngal, expect[0], RTOL)
        assert_rel(xi, expect[1], RTOL)
    check_still_serves(joint, members, theta, x)


def test_refused_requests_leave_everything_usable():
    case = get_case('rows-18')
    joint, theta, x = case['joint'], case['theta'][:5], case['x'][:5]
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.predict_batch_grad(np.zeros((5, 14)), x, family='leauthaud11')
    outside = x.copy()
    outside[2, 0] = case['members'][0][2].max() + 0.1
    with pytest.raises(ValueError, match='extrapolation'):
        joint.predict_batch_grad(theta, outside)
    with pytest.raises(ValueError, match='extrapolation'):
        joint.chi2_fisher_batch(theta, outside, np.zeros(8), np.eye(8))
    check_still_serves(joint, case['members'], theta, x)


# ---- model objects -------------------------------------------------------------------------------

@pytest.mark.parametrize('assembias', [False, True], ids=['plain', 'decorated'])
def test_model_object_calls(assembias):
    """predict_grad and chi2_fisher of a model object are row 3 of the batched calls, keyed by the
    model's keys followed by the grid's."""
    from tabcorr_amd import Zheng07Model
    from tabcorr_amd.models import ZHENG07_ASSEMBIAS_KEYS, ZHENG07_KEYS
    case = get_case('rows-36-sec', modulate=True, assembias=assembias)
    joint, row = case['joint'], 3
    theta, x = case['theta'][row:row + 1], case['x'][row:row + 1]
    model_keys = tuple(ZHENG07_ASSEMBIAS_KEYS if assembias else ZHENG07_KEYS)
    keys = model_keys + tuple(joint.keys)
    if assembias:
        import test_gpu_assembias_grad as assembias_suite
        model = assembias_suite.decorated_model(theta[0], True, {joint.keys[0]: x[0, 0]})
    else:
        model = Zheng07Model(redshift=0.0, modulate_with_cenocc=True)
        for key, value in zip(keys, np.concatenate([theta[0], x[0]])):
            model.param_dict[key] = value
    batch = joint.predict_batch_grad(theta, x, **case['options'])
    one = joint.predict_grad(model, assembias=assembias)
    assert isinstance(one[0], float) and one[0] == batch[0][0]
    assert tuple(one[2]) == keys and tuple(one[3]) == keys
    for m in range(2):
        assert np.array_equal(one[1][m], batch[1][m][0])
    for k, key in enumerate(keys):
        assert one[2][key] == batch[2][0, k]
        for m in range(2):
            assert np.array_equal(one[3][key][m], batch[3][m][0, k])
    data, precision = operands(case, False)
    batch = joint.chi2_fisher_batch(theta, x, data, precision, **case['options'])
    one = joint.chi2_fisher(model, data, precision, assembias=assembias)
    assert one[0] == batch[0][0] and one[1] == batch[1][0]
    assert tuple(one[2]) == keys and tuple(one[3]) == keys
    for k, key in enumerate(keys):
        assert one[2][key] == batch[2][0, k] and one[3][key] == batch[3][0, k]
    assert np.array_equal(one[4], batch[4][0])
