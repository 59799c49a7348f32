"""The forward calls of a joint of interpolators on the device (JointInterpolator.predict_batch /
chi2_batch, the tc_joint_interp_predict_batch / tc_joint_interp_chi2_batch entry points,
joint_interp_forward_kernel) against the references the joint already has:
`joint_interp_reference.jacobian_batch` for ngal and xi with the allowance RTOL |value| + RTOL scale,
`joint_interp_reference.chi2_reference` for chi2 and its allowance, `util.assert_rel(..., 1e-10)`
per member block against the members' own `Interpolator.predict_batch`.  No new tolerance.  Needs
an MI355X.

Every case prints its largest error in units of its allowance.  Plain draws:
synthetic.zheng07_draws(130, seed=1) with x from test_gpu_interp_grad.make_x(..., 5), every one of
them with a finite reference -- no draw is left out; decorated: the rule for the draws of
test_gpu_joint_interp.get_case, the seed chosen from the reference alone.  (ngal > 0 is not
asserted: with two classes of halo tables the extrapolated ngal is legitimately negative outside
the grid.)
"""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assembias_grad_reference  # noqa: E402
import joint_interp_reference as reference  # noqa: E402
import joint_reference  # noqa: E402
import test_gpu_interp_grad as interp_suite  # noqa: E402
import test_gpu_joint_interp as joint_suite  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    LDS_LIMIT, RTOL, check_still_serves, device_call, largest, same_bits)
from util import assert_rel  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 64                                       # draws per workgroup (joint.h: kJointForwardDraws)
DRAW_COUNTS = [1, T - 1, T + 1, 2 * T + 2]   # the tile's edge, a second and a third workgroup
N_MAX = max(DRAW_COUNTS)
SLAB = 64                                    # joint_interp.h: kJointInterpForwardSlab

AUTO_CROSS = joint_suite.AUTO_CROSS
CROSS_CROSS = joint_suite.CROSS_CROSS
# name -> (parts, grid, n_prim, n_sec, classes); bins = 2 n_prim n_sec
SHAPES = {
    'rows-18': joint_suite.SHAPES['rows-18'],
    'rows-36-4x4': joint_suite.SHAPES['rows-36-4x4'],
    'rows-32-cross-first': joint_suite.SHAPES['rows-32-cross-first'],
    # a full r tile, a one-row table, the passes of two auto members dealt through the list
    'rows-36-full-tile': ((('auto', (20, )), ('auto', (1, )), ('cross', (7, ))), (4, ), 9, 2,
                          'two'),
    'slabs-36': joint_suite.SHAPES['slabs-36'],
    # 160 bins: two slabs of 64 and one of 32
    'slabs-160-4x4': joint_suite.SHAPES['slabs-160-4x4'],
    'one-auto': ((('auto', (3, )), ), (4, ), 9, 1, 'one'),
    'one-cross': ((('cross', (5, )), ), (4, ), 18, 1, 'two'),
    'rows-36-sec': joint_suite.SHAPES['rows-36-sec'],
    'slabs-36-sec': joint_suite.SHAPES['slabs-36-sec'],
}
MAIN = ['rows-18', 'rows-36-4x4', 'rows-32-cross-first', 'rows-36-full-tile', 'slabs-36',
        'slabs-160-4x4', 'one-auto', 'one-cross']
assert 2 * SLAB < 2 * 40 * 2 < 3 * SLAB

_joints = {}
_cases = {}


def get_joint(name, assembias=False):
    """(members, interpolators, JointInterpolator), made once."""
    from tabcorr_amd import JointInterpolator
    key = (name, assembias)
    if key not in _joints:
        parts, grid, n_prim, n_sec, classes = SHAPES[name]
        members = reference.make_members(grid, n_prim, n_sec, parts, classes, assembias=assembias)
        interpolators = [joint_suite.make_interpolator(member) for member in members]
        _joints[key] = (members, interpolators, JointInterpolator(interpolators))
    return _joints[key]


def get_case(name, modulate=False, assembias=False, x_kind='inside'):
    """The joint, draws (theta, x) and their reference, made once per combination and never
    modified: a batch of n draws is the first n of them."""
    key = (name, modulate, assembias, x_kind)
    if key not in _cases:
        members, interpolators, joint = get_joint(name, assembias)
        tables, _, points = members[0]
        setup = oracle.interpolator_setup(tables, points)

        def compute(theta, x, shared=True):
            with np.errstate(all='ignore'):
                return reference.jacobian_batch(members, theta, x, 10, modulate, assembias, shared)

        if not assembias:
            theta = synthetic.zheng07_draws(N_MAX, seed=1)
            x = interp_suite.make_x(points, setup, N_MAX, x_kind, 5)
            expect = compute(theta, x)
        else:
            # (test_gpu_joint_interp.get_case: the first seed from 5 on with a finite reference
            # that the rounding of the central columns does not reach)
            for seed in range(5, 25):
                theta = assembias_grad_reference.stress_draws(tables[0], N_MAX, seed=seed)
                x = interp_suite.make_x(points, setup, N_MAX, x_kind, seed)
                expect = compute(theta, x)
                if not reference.usable(expect):
                    continue
                allowance = RTOL * (np.abs(expect['dxi']) + expect['dxi_scale'])
                if assembias_grad_reference.rounding_of_centrals(
                        lambda: compute(theta, x, False)['dxi'], expect['dxi'],
                        allowance) <= 0.1:
                    break
            else:
                raise AssertionError('no seed gives usable draws for %s' % (key, ))
        # no draw is left out: every one of them has a finite reference
        assert reference.usable(expect), key
        assert np.all(np.isfinite(expect['xi'])), key
        for array in [theta, x] + list(expect.values()):
            array.setflags(write=False)
        _cases[key] = {
            'members': members, 'interpolators': interpolators, 'joint': joint, 'theta': theta,
            'x': x, 'reference': expect,
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


def concatenated(xis):
    return np.concatenate([xi.reshape(len(xi), -1) for xi in xis], axis=1)


def check_prediction(case, got, n, what):
    """ngal and xi of the first n draws against the reference, allowance RTOL |value| + RTOL
    scale; every member's block against its own predict_batch at 1e-10."""
    joint = case['joint']
    expect = reference.first(case['reference'], n)
    ngal, xis = got
    assert ngal.shape == (n, ) and len(xis) == len(case['interpolators'])
    for xi, interp in zip(xis, case['interpolators']):
        assert xi.shape == (n, ) + tuple(interp.tabcorr_list[0].tpcf_shape)
    worst = 0.0
    for name, value in (('ngal', ngal), ('xi', concatenated(xis))):
        assert value.shape == expect[name].shape, (what, name)
        allowance = RTOL * np.abs(expect[name]) + RTOL * expect[name + '_scale']
        error = np.abs(value - expect[name])
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(error == 0.0, 0.0, error / allowance)
        worst = max(worst, float(np.max(ratio)))
        assert np.all(error <= allowance), (what, name, float(np.max(ratio)))
    print('%s: max |error| / allowance = %.3g' % (what, worst))
    assert joint.n_r_total == expect['xi'].shape[1]


def check_chi2(chi2, case, data, precision, what):
    n = len(chi2)
    expect = reference.chi2_reference(reference.first(case['reference'], n), data, precision)
    error = np.abs(chi2 - expect[0])
    print('%s: max chi2 error / allowance = %.3g' % (what, np.max(error / expect[2])))
    assert np.all(error <= expect[2]), what


def check_all(name, modulate=False, assembias=False, x_kind='inside', counts=DRAW_COUNTS):
    case = get_case(name, modulate, assembias, x_kind)
    joint, options = case['joint'], case['options']
    for n in counts:
        theta, x = case['theta'][:n], case['x'][:n]
        what = '%s n=%d modulate=%s assembias=%s x=%s' % (name, n, modulate, assembias, x_kind)
        got = joint.predict_batch(theta, x, **options)
        check_prediction(case, got, n, what)
        for symmetric in (True, False):
            data, precision = operands(case, symmetric)
            ngal, chi2 = joint.chi2_batch(theta, x, data, precision, **options)
            assert ngal.shape == chi2.shape == (n, )
            # the two forms evaluate one number density
            assert same_bits((ngal, ), (got[0], ))
            check_chi2(chi2, case, data, precision, '%s symmetric=%s' % (what, symmetric))
    # the members' own calls, and the per-member list form of the data
    for xi, interp in zip(got[1], case['interpolators']):
        own = interp.predict_batch(theta, x, **options)
        assert_rel(got[0], own[0], RTOL, what + ' ngal against predict_batch')
        assert_rel(xi, own[1], RTOL, what + ' xi against predict_batch')
    parts = [data[part] for part in joint.slices]
    assert same_bits(joint.chi2_batch(theta, x, parts, precision, **options), (ngal, chi2))
    return case


# ---- 1. reference parity ------------------------------------------------------------------------

@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('name', MAIN)
def test_forward_matches_reference(name, modulate):
    check_all(name, modulate)


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('name', MAIN)
def test_outside_the_grid(name, modulate):
    """x beyond the grid on both sides with extrapolate=True: the outermost polynomial."""
    case = check_all(name, modulate, x_kind='outside')
    with pytest.raises(ValueError, match='extrapolation'):
        case['joint'].predict_batch(case['theta'], case['x'])


@pytest.mark.parametrize('x_kind', ['inside', 'outside'])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('name', ['rows-36-sec', 'slabs-36-sec'])
def test_decorated_forward_matches_reference(name, modulate, x_kind):
    """The decorated model, 7 columns of theta, in both forms: all four draw counts, x inside the
    grid and beyond it on both sides with extrapolate=True."""
    case = check_all(name, modulate, True, x_kind)
    assert case['theta'].shape == (N_MAX, 7)
    if x_kind == 'outside':
        with pytest.raises(ValueError, match='extrapolation'):
            case['joint'].predict_batch(case['theta'], case['x'], assembias=True)


def test_other_node_counts_take_the_generic_instance():
    """n_gauss_prim = 7: the instance for any number of nodes, against the reference with 7."""
    for name in ('rows-36-4x4', 'slabs-36'):
        case = get_case(name)
        n = T + 1
        theta, x = case['theta'][:n], case['x'][:n]
        with np.errstate(all='ignore'):
            expect = reference.jacobian_batch(case['members'], theta, x, 7)
        seven = dict(case, reference=expect)
        got = case['joint'].predict_batch(theta, x, n_gauss_prim=7)
        check_prediction(seven, got, n, name + ' 7 nodes')
        assert not np.array_equal(got[0], case['joint'].predict_batch(theta, x)[0])
        data, precision = operands(seven, False)
        ngal, chi2 = case['joint'].chi2_batch(theta, x, data, precision, n_gauss_prim=7)
        assert same_bits((ngal, ), (got[0], ))
        check_chi2(chi2, seven, data, precision, name + ' 7 nodes')


# ---- 2. exact properties ------------------------------------------------------------------------

def device_entries(joint, theta, x, data, precision, flags=0):
    """tc_joint_interp_predict_batch_device and tc_joint_interp_chi2_batch_device (data and
    precision are host arrays there too)."""
    from tabcorr_amd import _lib
    device = joint.to_device()
    n = len(theta)
    arguments = [theta, theta.shape[1], x, n, 10, flags]
    predicted = device_call(device, 'tc_joint_interp_predict_batch_device', arguments,
                            [n, (n, joint.n_r_total)], 'tc_joint_interp_synchronize')
    data, precision = _lib.contiguous(data), _lib.contiguous(precision)
    likelihood = device_call(device, 'tc_joint_interp_chi2_batch_device',
                             arguments + [_lib.as_double_p(data), _lib.as_double_p(precision)],
                             [n, n], 'tc_joint_interp_synchronize')
    return predicted, likelihood


@pytest.mark.parametrize('name', ['rows-36-4x4', 'rows-36-full-tile', 'slabs-160-4x4'])
def test_a_draw_has_its_bits_wherever_it_sits(name):
    """No tolerance: a draw's (ngal, xi, chi2) does not depend on the batch size or on its
    position in the batch, nor on the entry -- host arrays or device pointers."""
    from tabcorr_amd import _lib
    case = get_case(name)
    joint, theta, x = case['joint'], case['theta'], case['x']
    data, precision = operands(case, False)
    ngal, xis = joint.predict_batch(theta, x)
    flat = (ngal, concatenated(xis))
    full = joint.chi2_batch(theta, x, data, precision)
    assert all(np.all(np.isfinite(a)) for a in flat + full)
    assert same_bits((full[0], ), (ngal, ))
    for n in DRAW_COUNTS:
        one = joint.predict_batch(theta[:n], x[:n])
        assert same_bits((one[0], concatenated(one[1])), [a[:n] for a in flat]), (name, n)
        assert same_bits(joint.chi2_batch(theta[:n], x[:n], data, precision),
                         [a[:n] for a in full]), (name, n)
        predicted, likelihood = device_entries(joint, theta[:n], x[:n], data, precision)
        assert same_bits(predicted, [a[:n] for a in flat]), (name, n)
        assert same_bits(likelihood, [a[:n] for a in full]), (name, n)
    # another position in the batch: alone, and as draw 5 of the second workgroup
    for row in (T - 1, T, N_MAX - 1):
        one = joint.predict_batch(theta[row:row + 1], x[row:row + 1])
        assert same_bits((one[0], concatenated(one[1])), [a[row:row + 1] for a in flat])
        moved = [np.ascontiguousarray(np.roll(a, T + 5 - row, axis=0)) for a in (theta, x)]
        again = joint.predict_batch(*moved)
        assert same_bits((again[0][T + 5:T + 6], concatenated(again[1])[T + 5:T + 6]),
                         [a[row:row + 1] for a in flat])
        assert same_bits([a[T + 5:T + 6] for a in joint.chi2_batch(*moved, data, precision)],
                         [a[row:row + 1] for a in full])
    # modulate_with_cenocc through the flags of the device entries
    modulated = joint.chi2_batch(theta, x, data, precision, modulate_with_cenocc=True)
    assert same_bits(device_entries(joint, theta, x, data, precision,
                                    flags=_lib.FLAG_MODULATE_WITH_CENOCC)[1], modulated)
    assert not np.array_equal(modulated[1], full[1])


@pytest.mark.parametrize('name', ['rows-18', 'slabs-36'])
def test_large_host_calls_return_the_same_bits(name):
    """9100 draws, the 130 of the case seventy times over, on host arrays: beyond the page-locked
    staging of small calls the call travels in overlapping chunks on member 0's lanes, or (option
    "sync_chunks" = -1 of member 0's first table) in one piece through its device buffers.  Every
    block of 130 results is the small call's, bit for bit."""
    from tabcorr_amd import _lib
    case = get_case(name)
    joint = case['joint']
    data, precision = operands(case, False)
    small = joint.predict_batch(case['theta'], case['x'])
    small = (small[0], concatenated(small[1])) + tuple(
        joint.chi2_batch(case['theta'], case['x'], data, precision))
    theta, x = (np.ascontiguousarray(np.tile(a, (70, 1))) for a in (case['theta'], case['x']))
    assert theta.nbytes + x.nbytes + 16 * len(theta) > 512 * 1024
    handle = case['interpolators'][0].tabcorr_list[0].to_device().handle
    try:
        for chunks in (0, -1):
            _lib.check(_lib.load().tc_table_set_option(handle, b'sync_chunks', chunks))
            large = joint.predict_batch(theta, x)
            large = (large[0], concatenated(large[1])) + tuple(
                joint.chi2_batch(theta, x, data, precision))
            for got, expect in zip(large, small):
                assert np.array_equal(got, np.tile(expect, (70, ) + (1, ) * (expect.ndim - 1))), \
                    (name, chunks)
    finally:
        _lib.check(_lib.load().tc_table_set_option(handle, b'sync_chunks', 0))


def test_permuting_the_members_permutes_the_blocks():
    """The arithmetic of a row does not depend on the wave that runs it: every order of the
    members returns the same bits, block by block, and ngal does not depend on which members are
    in the joint -- not even on its form."""
    import itertools
    from tabcorr_amd import JointInterpolator
    case = get_case('rows-36-full-tile')
    interpolators, theta, x = case['interpolators'], case['theta'], case['x']
    ngal, xis = case['joint'].predict_batch(theta, x)
    for order in itertools.permutations(range(3)):
        got = JointInterpolator([interpolators[k] for k in order]).predict_batch(theta, x)
        assert same_bits((got[0], ), (ngal, )), order
        assert same_bits(got[1], [xis[k] for k in order]), order
    for k in (0, 1):
        alone = JointInterpolator([interpolators[k]]).predict_batch(theta, x)
        assert same_bits((alone[0], alone[1][0]), (ngal, xis[k])), k
    # (the cross member alone is a joint of the slab form)
    assert same_bits((JointInterpolator([interpolators[2]]).predict_batch(theta, x)[0], ),
                     (ngal, ))
    case = get_case('slabs-160-4x4')
    ngal, xis = case['joint'].predict_batch(case['theta'], case['x'])
    got = JointInterpolator(case['interpolators'][::-1]).predict_batch(case['theta'], case['x'])
    assert same_bits((got[0], ), (ngal, )) and same_bits(got[1], xis[::-1])


@pytest.mark.parametrize('name', ['rows-36-4x4', 'slabs-160-4x4'])
def test_a_permuted_member_changes_nothing(name):
    """A member other than member 0 whose list is a permutation of member 0's: tables are matched
    by grid node and the walk is member 0's, the results are the unpermuted joint's bit for bit."""
    from tabcorr_amd import JointInterpolator
    case = get_case(name)
    members = case['members']
    order = np.random.default_rng(9).permutation(len(members[0][0]))
    assert np.any(order != np.arange(len(order)))
    shuffled = joint_suite.make_interpolator(reference.permuted(members[1], order))
    joint = JointInterpolator([case['interpolators'][0], shuffled])
    data, precision = operands(case, False)
    theta, x = case['theta'], case['x']
    got, expect = joint.predict_batch(theta, x), case['joint'].predict_batch(theta, x)
    assert same_bits((got[0], ) + tuple(got[1]), (expect[0], ) + tuple(expect[1]))
    assert same_bits(joint.chi2_batch(theta, x, data, precision),
                     case['joint'].chi2_batch(theta, x, data, precision))


def test_reference_fixture_in_the_slab_form():
    """The reference's AbacusSummit interpolator (4 tables of 1104 bins, mode cross: 18 slabs, the
    last one partial) joined with a second member made of the same tables (the first five r rows,
    times 3): every member's block against its own predict_batch at 1e-10; the likelihood form
    evaluates the same number density, bit for bit."""
    from tabcorr_amd import Interpolator, JointInterpolator, TabCorr
    first = Interpolator.read(os.path.join(REPO, 'tests', 'golden', 'ds_efficient.hdf5'))
    assert len(first.tabcorr_list) == 4 and len(first.tabcorr_list[0].gal_type) == 1104
    halotabs = [TabCorr.from_arrays(t.gal_type, 3.0 * np.asarray(t.tpcf_matrix)[:5], (5, ),
                                    t.attrs) for t in first.tabcorr_list]
    second = Interpolator(halotabs, {key: first.points[:, d] for d, key in enumerate(first.keys)})
    joint = JointInterpolator([first, second])
    n = T + 1
    rng = np.random.default_rng(5)
    theta = synthetic.zheng07_draws(n, seed=9)
    theta[:, 0] = rng.uniform(12.5, 13.3, n)
    theta[:, 3] = rng.uniform(13.6, 14.4, n)
    x = np.stack([rng.uniform(xp[0], xp[-1], n) for xp in first.xp], axis=-1)
    ngal, xis = joint.predict_batch(theta, x)
    assert np.all(np.isfinite(ngal))
    own = [interp.predict_batch(theta, x) for interp in (first, second)]
    for xi, (own_ngal, own_xi) in zip(xis, own):
        assert np.all(np.isfinite(own_xi))
        assert_rel(ngal, own_ngal, RTOL)
        assert_rel(xi, own_xi, RTOL, floor=1e-12)
    xi = concatenated(xis)
    data, precision = joint_reference.coupled_data(xi[3], False, in_units_of_xi=True)
    got = joint.chi2_batch(theta, x, data, precision)
    assert same_bits((got[0], ), (ngal, )) and np.all(np.isfinite(got[1]))


# ---- 3. refusals --------------------------------------------------------------------------------

def check_everything_still_serves(members, interpolators, joint):
    """The joint's gradient call and every member's first table serve."""
    theta = synthetic.zheng07_draws(5, seed=2)
    x = interp_suite.make_x(members[0][2], None, 5, 'inside', 2)
    n = joint.n_r_total
    gradient = joint.chi2_grad_batch(theta, x, np.ones(n), np.eye(n))
    assert np.all(np.isfinite(gradient[1]))
    # (a forward call builds member 0's walk without its gradient matrices: its own derivative
    # call adds them)
    own = interpolators[0].predict_batch_grad(theta, x)
    assert all(np.all(np.isfinite(a)) for a in own)
    assert_rel(own[0], gradient[0], RTOL, 'ngal of predict_batch_grad')
    for (tables, _, _), interp in zip(members, interpolators):
        check_still_serves(interp.tabcorr_list[0], tables[0])


def test_refusals_leave_the_joint_and_its_members_usable():
    from tabcorr_amd import _lib
    case = get_case('rows-18')
    joint, members, interpolators = case['joint'], case['members'], case['interpolators']
    small, x = np.ascontiguousarray(case['theta'][:3]), np.ascontiguousarray(case['x'][:3])
    good_data, good_precision = np.zeros(8), np.eye(8)
    device = joint.to_device()
    lib = device.lib
    out = [np.empty(3), np.empty((3, 8))]
    pointers = [_lib.as_double_p(a) for a in out]
    p_theta, p_x = _lib.as_double_p(small), _lib.as_double_p(x)
    for flags, match in ((_lib.FLAG_LEAUTHAUD11, 'Zheng07 family'),
                         (_lib.FLAG_SEPARATE_GAL_TYPE, 'separate_gal_type'),
                         (32, 'unknown flags')):
        with device.lock:
            status = lib.tc_joint_interp_predict_batch(device.handle, p_theta, 5, p_x, 3, 10,
                                                       flags, *pointers)
        assert status == _lib.TC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match=match):
            _lib.check(status)
        with device.lock:
            status = lib.tc_joint_interp_chi2_batch_device(
                device.handle, None, 5, None, 3, 10, flags, _lib.as_double_p(good_data),
                _lib.as_double_p(good_precision), None, None)
        assert status == _lib.TC_ERR_UNSUPPORTED
    check_everything_still_serves(members, interpolators, joint)
    with device.lock:
        predict = lib.tc_joint_interp_predict_batch
        assert predict(device.handle, p_theta, 5, p_x, 3, 10, _lib.FLAG_ASSEMBIAS,
                       *pointers) == _lib.TC_ERR_INVALID
        assert predict(device.handle, p_theta, 5, p_x, 3, 10, 0, pointers[0],
                       None) == _lib.TC_ERR_INVALID
        assert predict(device.handle, p_theta, 5, None, 3, 10, 0, *pointers) == _lib.TC_ERR_INVALID
        assert lib.tc_joint_interp_chi2_batch(device.handle, p_theta, 5, p_x, 3, 10, 0, None,
                                              _lib.as_double_p(good_precision), pointers[0],
                                              pointers[0]) == _lib.TC_ERR_INVALID
        assert predict(device.handle, p_theta, 5, p_x, -1, 10, 0, *pointers) == _lib.TC_ERR_INVALID
        # n_draws == 0: nothing to do, nothing is read (as the joint of tables)
        assert predict(device.handle, None, 5, None, 0, 10, 0, None, None) == _lib.TC_OK
        assert lib.tc_joint_interp_chi2_batch_device(device.handle, None, 5, None, 0, 10, 0, None,
                                                     None, None, None) == _lib.TC_OK
    empty = joint.predict_batch(np.zeros((0, 5)), np.zeros((0, 1)))
    assert empty[0].shape == (0, ) and [xi.shape for xi in empty[1]] == [(0, 3), (0, 5)]
    assert [a.shape for a in joint.chi2_batch(np.zeros((0, 5)), np.zeros((0, 1)), good_data,
                                              good_precision)] == [(0, ), (0, )]
    check_everything_still_serves(members, interpolators, joint)
    check_prediction(case, joint.predict_batch(small, x), 3, 'afterwards')


def forward_lds(n_bins, n_total, weight_rows):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    _lib.check(_lib.load().tc_debug_joint_interp_forward_lds_bytes(1, n_bins, n_total, weight_rows,
                                                                   8, ctypes.byref(got)))
    return got.value


def test_what_the_kernel_does_not_serve_is_refused():
    """A mode-auto member of 21 r bins (two r tiles); a joint of 24 bins and 60 rows, whose
    passes' slabs go beyond 160 KiB (the gradient kernel, 16 draws per workgroup, serves it); and
    the first joint [auto (5, ), cross (3, )] on a grid (4, ) whose densities go beyond it by the
    formula (the one before it is served): NotImplementedError with a message, nothing is
    launched, and the joint's gradient calls -- where that kernel has the LDS -- and the members'
    tables go on serving."""
    from tabcorr_amd import JointInterpolator
    theta = synthetic.zheng07_draws(5, seed=2)
    limit = largest(lambda n_prim: forward_lds(4 * n_prim, 8, 4) <= LDS_LIMIT)
    pair = [('auto', (5, )), ('cross', (3, ))]
    assert forward_lds(24, 60, 4) > LDS_LIMIT
    for n_prim, parts, match, gradients in (
            (6, [('auto', (21, )), ('cross', (3, ))], 'r tile', True),
            (6, [('auto', (20, )), ('cross', (40, ))], 'LDS', True),
            (limit, pair, None, False), (limit + 1, pair, 'LDS', False)):
        members = reference.make_members((4, ), n_prim, 2, parts)
        interpolators = [joint_suite.make_interpolator(member) for member in members]
        joint = JointInterpolator(interpolators)
        x = interp_suite.make_x(members[0][2], None, 5, 'inside', 2)
        n = joint.n_r_total
        if match is None:
            ngal, xis = joint.predict_batch(theta, x)
            for interp, xi in zip(interpolators, xis):
                own = interp.predict_batch(theta, x)
                assert_rel(ngal, own[0], RTOL, 'ngal at the limit')
                assert_rel(xi, own[1], RTOL, 'xi at the limit')
            assert same_bits((joint.chi2_batch(theta, x, np.ones(n), np.eye(n))[0], ), (ngal, ))
        else:
            with pytest.raises(NotImplementedError, match=match):
                joint.predict_batch(theta, x)
            with pytest.raises(NotImplementedError, match=match):
                joint.chi2_batch(theta, x, np.ones(n), np.eye(n))
        if gradients:
            check_everything_still_serves(members, interpolators, joint)
        else:
            for (tables, _, _), interp in zip(members, interpolators):
                check_still_serves(interp.tabcorr_list[0], tables[0])


# ---- 4. the example -----------------------------------------------------------------------------

def test_example_runs_on_the_smallest_pair():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, 'examples', 'example_joint_interp_mcmc.py'),
         '--walkers', '16', '--steps', '5', '--n-prim', '9'],
        capture_output=True, text=True, timeout=120, cwd=REPO,
        env=dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', '')))
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'acceptance' in out.stdout
