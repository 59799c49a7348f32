"""The forward calls of a joint of tables on the device (JointLikelihood.predict_batch / chi2_batch,
the tc_joint_predict_batch / tc_joint_chi2_batch entry points) against the references the joint
already has: `joint_reference.jacobian_batch` for ngal and xi, `joint_reference.chi2_reference` for
chi2 and its allowance, `util.assert_rel(..., 1e-10)` per table block.  No new tolerance.  Needs an
MI355X.

Every case prints its largest error in units of its allowance.  Plain draws:
synthetic.zheng07_draws(130, seed=1), every one of them with a finite reference and ngal > 0 -- no
draw is left out; decorated: the tables and the rule for the draws of test_gpu_joint.py.
"""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assembias_grad_reference  # noqa: E402
import joint_reference  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    LDS_LIMIT, RTOL, check_still_serves, device_call, largest, same_bits)
from util import assert_rel, load_golden, table_from_golden  # noqa: E402

pytestmark = pytest.mark.gpu

T = 64                                       # draws per workgroup (joint.h: kJointForwardDraws)
DRAW_COUNTS = [1, T - 1, T + 1, 2 * T + 2]   # the tile's edge, a second and a third workgroup
N_MAX = max(DRAW_COUNTS)

# name -> (n_prim, n_sec, parts).  24 bins; the last one 108 bins.
JOINTS = {
    'auto5-cross3': (6, 2, [('auto', (5, )), ('cross', (3, ))]),
    'auto19-auto4-cross7': (6, 2, [('auto', (19, )), ('auto', (4, )), ('cross', (7, ))]),
    'cross6-cross2': (6, 2, [('cross', (6, )), ('cross', (2, ))]),
    'auto20': (6, 2, [('auto', (20, ))]),
    'cross1': (6, 2, [('cross', (1, ))]),
    'auto5-cross3-108': (27, 2, [('auto', (5, )), ('cross', (3, ))]),
}
REAL = 'bolplanck'                           # w_p + DeltaSigma: 60 bins, N = 38
REAL_DRAWS = 256

_joints = {}
_references = {}


def make_halotab(table, **kwargs):
    from tabcorr_amd import TabCorr
    return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                               table['attrs'], **kwargs)


def get_joint(name, assembias=False):
    """(table dicts, TabCorr list, JointLikelihood), made once."""
    from tabcorr_amd import JointLikelihood
    key = (name, assembias)
    if key not in _joints:
        if name == REAL:
            tables = [table_from_golden(load_golden('bolplanck_wp')),
                      table_from_golden(load_golden('bolplanck_ds'))]
        else:
            n_prim, n_sec, parts = JOINTS[name]
            tables = joint_reference.make_tables(n_prim, n_sec, parts, assembias)
        halotabs = [make_halotab(table) for table in tables]
        _joints[key] = (tables, halotabs, JointLikelihood(halotabs))
    return _joints[key]


def get_reference(name, modulate=False, assembias=False):
    """The draws and their joint reference (ngal, xi, dngal, dxi, scale), computed once and never
    modified: a batch of n draws is the first n of them."""
    key = (name, modulate, assembias)
    if key not in _references:
        tables = get_joint(name, assembias)[0]
        if not assembias:
            theta = synthetic.zheng07_draws(REAL_DRAWS if name == REAL else N_MAX, seed=1)
            with np.errstate(all='ignore'):
                reference = joint_reference.jacobian_batch(tables, theta, 10, modulate)
        else:
            module = assembias_grad_reference
            for seed in range(5, 25):
                theta = module.stress_draws(tables[0], N_MAX, seed=seed)
                with np.errstate(all='ignore'):
                    reference = joint_reference.jacobian_batch(tables, theta, 10, modulate, True)
                    parts = [module.jacobian_batch(t, theta, 10, modulate) for t in tables]
                if joint_reference.usable(reference) and all(
                        module.well_conditioned(t, theta, part, 10, modulate)
                        for t, part in zip(tables, parts)):
                    break
            else:
                raise AssertionError('no seed gives usable draws for %s' % (key, ))
        # no draw is left out: every one of them has galaxies and a finite reference
        assert joint_reference.usable(reference), key
        assert np.all(np.isfinite(reference[1])) and np.all(reference[0] > 0.0), key
        for array in (theta, ) + reference:
            array.setflags(write=False)
        _references[key] = (theta, reference)
    return _references[key]


def concatenated(xis):
    return np.concatenate([xi.reshape(len(xi), -1) for xi in xis], axis=1)


def check_prediction(joint, halotabs, got, reference, n, what):
    ngal, xis = got
    assert ngal.shape == (n, ) and len(xis) == len(halotabs)
    assert_rel(ngal, reference[0][:n], RTOL, what + ' ngal')
    for part, halotab, xi in zip(joint.slices, halotabs, xis):
        assert xi.shape == (n, ) + tuple(halotab.tpcf_shape)
        # (per table: the floor of assert_rel is that of the table's own scale)
        assert_rel(xi.reshape(n, -1), reference[1][:n, part], RTOL, what + ' xi')


def check_chi2(chi2, reference, data, precision, what):
    n = len(chi2)
    expect = joint_reference.chi2_reference(tuple(a[:n] for a in reference), data, precision)
    error = np.abs(chi2 - expect[0])
    print('%s: max chi2 error / allowance = %.3g' % (what, np.max(error / expect[2])))
    assert np.all(error <= expect[2]), what


def check_all(name, modulate, assembias):
    _, halotabs, joint = get_joint(name, assembias)
    theta, reference = get_reference(name, modulate, assembias)
    kwargs = dict(modulate_with_cenocc=modulate, assembias=assembias)
    for n in DRAW_COUNTS:
        what = '%s n=%d modulate=%s assembias=%s' % (name, n, modulate, assembias)
        got = joint.predict_batch(theta[:n], **kwargs)
        check_prediction(joint, halotabs, got, reference, n, what)
        for symmetric in (True, False):
            data, precision = joint_reference.coupled_data(reference[1][3], symmetric)
            if len(halotabs) > 1:
                first = joint.slices[0].stop
                assert np.all(precision[:first, first:] != 0.0)
            ngal, chi2 = joint.chi2_batch(theta[:n], data, precision, **kwargs)
            assert ngal.shape == chi2.shape == (n, )
            # the two forms evaluate one number density
            assert same_bits((ngal, ), (got[0], ))
            check_chi2(chi2, reference, data, precision, '%s symmetric=%s' % (what, symmetric))
    # the per-table list form of the data
    parts = [data[part].reshape(halotab.tpcf_shape)
             for part, halotab in zip(joint.slices, halotabs)]
    assert same_bits(joint.chi2_batch(theta[:n], parts, precision, **kwargs), (ngal, chi2))


# ---- 1. oracle parity -------------------------------------------------------------------------

@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('name', list(JOINTS))
def test_forward_matches_reference(name, modulate):
    check_all(name, modulate, False)


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
def test_decorated_forward_matches_reference(modulate):
    check_all('auto5-cross3', modulate, True)


def test_other_node_counts_take_the_generic_instance():
    """n_gauss_prim = 7: the instance for any number of nodes, against the reference with 7."""
    name = 'auto19-auto4-cross7'
    tables, halotabs, joint = get_joint(name)
    theta = get_reference(name)[0][:T + 1]
    with np.errstate(all='ignore'):
        reference = joint_reference.jacobian_batch(tables, theta, 7, False)
    got = joint.predict_batch(theta, n_gauss_prim=7)
    check_prediction(joint, halotabs, got, reference, len(theta), name + ' 7 nodes')
    assert not np.array_equal(got[0], joint.predict_batch(theta)[0])
    data, precision = joint_reference.coupled_data(reference[1][3], False)
    ngal, chi2 = joint.chi2_batch(theta, data, precision, n_gauss_prim=7)
    assert same_bits((ngal, ), (got[0], ))
    check_chi2(chi2, reference, data, precision, name + ' 7 nodes')


# ---- 2. the real pair ---------------------------------------------------------------------------

def test_real_pair():
    """w_p + DeltaSigma, 256 draws, a precision matrix in units of |xi| that couples the two: chi2
    against the reference AND against JointLikelihood.chi2_grad_batch within the reference's
    allowance; xi against each table's own predict_batch at 1e-10."""
    _, halotabs, joint = get_joint(REAL)
    theta, reference = get_reference(REAL)
    assert len(theta) == REAL_DRAWS
    data, precision = joint_reference.coupled_data(reference[1][3], False, in_units_of_xi=True)
    assert np.all(precision[:19, 19:] != 0.0)
    ngal, xis = joint.predict_batch(theta)
    check_prediction(joint, halotabs, (ngal, xis), reference, REAL_DRAWS, REAL)
    for halotab, xi in zip(halotabs, xis):
        own = halotab.predict_batch(theta)
        assert_rel(ngal, own[0], RTOL, 'ngal against the table')
        assert_rel(xi, own[1], RTOL, 'xi against the table')
    got = joint.chi2_batch(theta, data, precision)
    assert same_bits((got[0], ), (ngal, ))
    check_chi2(got[1], reference, data, precision, REAL)
    grad = joint.chi2_grad_batch(theta, data, precision)
    allowance = joint_reference.chi2_reference(reference, data, precision)[2]
    error = np.abs(got[1] - grad[1])
    print('chi2 against chi2_grad_batch: max error / allowance = %.3g' % np.max(error / allowance))
    assert np.all(error <= allowance)
    assert_rel(got[0], grad[0], RTOL, 'ngal against chi2_grad_batch')


# ---- 3. exact properties ------------------------------------------------------------------------

def device_predict(joint, theta, flags=0):
    n = len(theta)
    return device_call(joint.to_device(), 'tc_joint_predict_batch_device',
                       [theta, theta.shape[1], n, 10, flags], [n, (n, joint.n_r_total)],
                       synchronize='tc_joint_synchronize')


def device_chi2(joint, theta, data, precision, flags=0):
    """tc_joint_chi2_batch_device (data and precision are host arrays there too)."""
    from tabcorr_amd import _lib
    n = len(theta)
    data, precision = _lib.contiguous(data), _lib.contiguous(precision)
    return device_call(joint.to_device(), 'tc_joint_chi2_batch_device',
                       [theta, theta.shape[1], n, 10, flags, _lib.as_double_p(data),
                        _lib.as_double_p(precision)], [n, n], synchronize='tc_joint_synchronize')


@pytest.mark.parametrize('name', ['auto5-cross3', 'auto19-auto4-cross7', 'cross6-cross2', REAL])
def test_a_draw_has_its_bits_wherever_it_sits(name):
    """No tolerance: a draw's (ngal, xi, chi2) does not depend on the batch size or on its
    position in the batch, nor on the entry -- host arrays or device pointers."""
    from tabcorr_amd import _lib
    _, _, joint = get_joint(name)
    theta, reference = get_reference(name)
    theta = theta[:N_MAX]
    data, precision = joint_reference.coupled_data(reference[1][3], False, name == REAL)
    ngal, xis = joint.predict_batch(theta)
    flat = (ngal, concatenated(xis))
    full = joint.chi2_batch(theta, data, precision)
    assert all(np.all(np.isfinite(a)) for a in flat + full)
    assert same_bits((full[0], ), (ngal, ))
    for n in (1, T + 1, N_MAX):
        one = joint.predict_batch(theta[:n])
        assert same_bits((one[0], concatenated(one[1])), [a[:n] for a in flat])
        assert same_bits(joint.chi2_batch(theta[:n], data, precision), [a[:n] for a in full])
        assert same_bits(device_predict(joint, theta[:n]), [a[:n] for a in flat])
        assert same_bits(device_chi2(joint, theta[:n], data, precision), [a[:n] for a in full])
    # another position in the batch: alone, and as draw 5 of the second workgroup
    for row in (T - 1, T, N_MAX - 1):
        one = joint.predict_batch(theta[row:row + 1])
        assert same_bits((one[0], concatenated(one[1])), [a[row:row + 1] for a in flat])
        assert same_bits(joint.chi2_batch(theta[row:row + 1], data, precision),
                         [a[row:row + 1] for a in full])
        moved = np.ascontiguousarray(np.roll(theta, T + 5 - row, axis=0))
        again = joint.predict_batch(moved)
        assert same_bits((again[0][T + 5:T + 6], concatenated(again[1])[T + 5:T + 6]),
                         [a[row:row + 1] for a in flat])
        assert same_bits([a[T + 5:T + 6] for a in joint.chi2_batch(moved, data, precision)],
                         [a[row:row + 1] for a in full])
    # modulate_with_cenocc through the flags of the device entries
    modulated = joint.chi2_batch(theta, data, precision, modulate_with_cenocc=True)
    assert same_bits(device_chi2(joint, theta, data, precision,
                                 flags=_lib.FLAG_MODULATE_WITH_CENOCC), modulated)
    assert not np.array_equal(modulated[1], full[1])


def test_permuting_the_tables_permutes_the_blocks():
    """The arithmetic of a row does not depend on the wave that runs it, and ngal not on the tables
    at all: every order of the list returns the same bits, block by block."""
    import itertools
    from tabcorr_amd import JointLikelihood
    name = 'auto19-auto4-cross7'
    _, halotabs, joint = get_joint(name)
    theta, _ = get_reference(name)
    ngal, xis = joint.predict_batch(theta)
    for order in itertools.permutations(range(3)):
        got = JointLikelihood([halotabs[k] for k in order]).predict_batch(theta)
        assert same_bits((got[0], ), (ngal, ))
        assert same_bits(got[1], [xis[k] for k in order])
    for k, halotab in enumerate(halotabs):
        alone = JointLikelihood([halotab]).predict_batch(theta)
        assert same_bits((alone[0], alone[1][0]), (ngal, xis[k]))


# ---- 4. block structure ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['auto5-cross3', REAL])
def test_block_diagonal_precision_gives_the_sum_of_the_tables(name):
    """With a block-diagonal precision chi2 of [auto, cross] is the sum of the two tables' own
    chi2_batch results, within the allowance of the joint reference."""
    _, halotabs, joint = get_joint(name)
    theta, reference = get_reference(name)
    data, precision = joint_reference.coupled_data(reference[1][3], False, name == REAL)
    first = joint.slices[0].stop
    precision = precision.copy()
    precision[:first, first:] = 0.0
    precision[first:, :first] = 0.0
    ngal, chi2 = joint.chi2_batch(theta, data, precision)
    check_chi2(chi2, reference, data, precision, name + ' block-diagonal')
    total = np.zeros_like(chi2)
    for part, halotab in zip(joint.slices, halotabs):
        own = halotab.chi2_batch(theta, data[part], np.ascontiguousarray(precision[part, part]))
        assert_rel(own[0], ngal, RTOL, 'ngal')
        total += own[1]
    allowance = joint_reference.chi2_reference(reference, data, precision)[2]
    error = np.abs(chi2 - total)
    print('%s: max |chi2 - sum of the tables| / allowance = %.3g' % (
        name, np.max(error / allowance)))
    assert np.all(error <= allowance)


# ---- 5. degenerate draws --------------------------------------------------------------------------

def same_specials(got, expect, what):
    """NaN and inf where `expect` has them, with their signs; the rest at 1e-10."""
    got, expect = np.asarray(got), np.asarray(expect)
    assert got.shape == expect.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(expect)), what
    infinite = np.isinf(expect)
    assert np.array_equal(np.isinf(got), infinite), what
    assert np.array_equal(got[infinite], expect[infinite]), what
    finite = np.isfinite(expect)
    if np.any(finite):
        assert_rel(got[finite], expect[finite], RTOL, what)


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
def test_degenerate_draws(modulate):
    """One draw each with NaN in theta, sigma_logM = 0 and ngal = 0 (logMmin = logM0 = 20: no
    galaxy of either kind) between two ordinary ones: NaN and inf where the tables' own
    predict_batch and chi2_batch put them."""
    from tabcorr_amd import JointLikelihood
    name = 'auto19-auto4-cross7'
    _, halotabs, joint = get_joint(name)
    base, reference = get_reference(name, modulate)
    theta = np.array(base[:6])
    theta[1, 3] = np.nan
    theta[2, 1] = 0.0
    theta[3, 0] = theta[3, 2] = 20.0
    theta[4, 0] = np.nan
    kwargs = dict(modulate_with_cenocc=modulate)
    ngal, xis = joint.predict_batch(theta, **kwargs)
    assert ngal[3] == 0.0 and np.isnan(ngal[4]) and np.all(np.isfinite(ngal[[0, 5]]))
    assert all(np.all(np.isnan(xi[[3, 4]])) and np.all(np.isfinite(xi[[0, 5]])) for xi in xis)
    for k, (halotab, xi) in enumerate(zip(halotabs, xis)):
        own = halotab.predict_batch(theta, **kwargs)
        same_specials(ngal, own[0], 'ngal against table %d' % k)
        same_specials(xi, own[1], 'xi against table %d' % k)
        # the table alone in a joint against its own likelihood
        data, precision = joint_reference.coupled_data(
            reference[1][3][joint.slices[k]], False)
        alone = JointLikelihood([halotab]).chi2_batch(theta, data, precision, **kwargs)
        expect = halotab.chi2_batch(theta, data, precision, **kwargs)
        same_specials(alone[0], expect[0], 'ngal of the likelihood, table %d' % k)
        same_specials(alone[1], expect[1], 'chi2 against table %d' % k)
    # the coupled likelihood: the quadratic form of the tables' own predictions
    data, precision = joint_reference.coupled_data(reference[1][3], False)
    got = joint.chi2_batch(theta, data, precision, **kwargs)
    assert np.array_equal(got[0], ngal, equal_nan=True)
    delta = np.concatenate([halotab.predict_batch(theta, **kwargs)[1].reshape(len(theta), -1)
                            for halotab in halotabs], axis=1) - data
    with np.errstate(all='ignore'):
        expect = np.einsum('nr,rs,ns->n', delta, precision, delta)
    assert np.array_equal(np.isnan(got[1]), np.isnan(expect))
    assert np.array_equal(np.isnan(got[1]), [False, np.isnan(expect[1]), np.isnan(expect[2]),
                                             True, True, False])
    check_chi2(got[1][[0, 5]], tuple(a[[0, 5]] for a in reference), data, precision, 'ordinary')


# ---- 6. refusals ------------------------------------------------------------------------------------

def check_everything_still_serves(tables, halotabs, joint):
    theta = synthetic.zheng07_draws(5, seed=2)
    assert np.all(np.isfinite(joint.predict_batch_grad(theta)[0]))
    n = joint.n_r_total
    assert np.all(np.isfinite(joint.chi2_grad_batch(theta, np.ones(n), np.eye(n))[1]))
    for table, halotab in zip(tables, halotabs):
        check_still_serves(halotab, table)


def test_refusals_leave_the_joint_and_its_tables_usable():
    from tabcorr_amd import JointLikelihood, _lib
    name = 'auto5-cross3'
    tables, halotabs, joint = get_joint(name)
    theta, reference = get_reference(name)
    small = np.ascontiguousarray(theta[:3])
    good_data, good_precision = np.zeros(8), np.eye(8)
    # before any device
    for call in (lambda: joint.predict_batch(np.zeros((3, 7))),
                 lambda: joint.predict_batch(small, assembias=True),
                 lambda: joint.chi2_batch(small, np.zeros(7), good_precision),
                 lambda: joint.chi2_batch(small, good_data, np.eye(7))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.chi2_batch(np.zeros((3, 14)), good_data, good_precision, family='leauthaud11')
    check_everything_still_serves(tables, halotabs, joint)
    # the C entries: flags, the columns of the family, NULL pointers, no draws, no handle
    device = joint.to_device()
    lib = device.lib
    out = [np.empty(3), np.empty((3, 8))]
    pointers = [_lib.as_double_p(a) for a in out]
    for flags, match in ((_lib.FLAG_LEAUTHAUD11, 'Zheng07 family'),
                         (_lib.FLAG_SEPARATE_GAL_TYPE, 'separate_gal_type'),
                         (32, 'unknown flags')):
        with device.lock:
            status = lib.tc_joint_predict_batch(device.handle, _lib.as_double_p(small), 5, 3, 10,
                                                flags, *pointers)
        assert status == _lib.TC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match=match):
            _lib.check(status)
    with device.lock:
        assert lib.tc_joint_predict_batch(device.handle, _lib.as_double_p(small), 5, 3, 10,
                                          _lib.FLAG_ASSEMBIAS, *pointers) == _lib.TC_ERR_INVALID
        assert lib.tc_joint_predict_batch(device.handle, _lib.as_double_p(small), 5, 3, 10, 0,
                                          pointers[0], None) == _lib.TC_ERR_INVALID
        assert lib.tc_joint_chi2_batch(device.handle, _lib.as_double_p(small), 5, 3, 10, 0, None,
                                       _lib.as_double_p(good_precision), pointers[0],
                                       pointers[0]) == _lib.TC_ERR_INVALID
        assert lib.tc_joint_predict_batch(device.handle, _lib.as_double_p(small), 5, -1, 10, 0,
                                          *pointers) == _lib.TC_ERR_INVALID
        # n_draws == 0: nothing to do, nothing is read
        assert lib.tc_joint_predict_batch(device.handle, None, 5, 0, 10, 0, None,
                                          None) == _lib.TC_OK
        assert lib.tc_joint_chi2_batch_device(device.handle, None, 5, 0, 10, 0, None, None, None,
                                              None) == _lib.TC_OK
    assert lib.tc_joint_predict_batch(None, _lib.as_double_p(small), 5, 3, 10, 0,
                                      *pointers) == _lib.TC_ERR_INVALID
    empty = joint.predict_batch(np.zeros((0, 5)))
    assert empty[0].shape == (0, ) and [xi.shape for xi in empty[1]] == [(0, 5), (0, 3)]
    assert [a.shape for a in joint.chi2_batch(np.zeros((0, 5)), good_data, good_precision)] == \
        [(0, ), (0, )]
    check_everything_still_serves(tables, halotabs, joint)
    check_prediction(joint, halotabs, joint.predict_batch(small), reference, 3, 'afterwards')


def forward_lds(n_bins, n_total):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    _lib.check(_lib.load().tc_debug_joint_forward_lds_bytes(n_bins, n_total, 8, ctypes.byref(got)))
    return got.value


def test_what_the_kernel_does_not_serve_is_refused():
    """A mode-auto member of 21 r bins (two r tiles), and the first joint [auto (5, ), cross (3, )]
    of 4 n_prim bins whose workgroup would need more than 160 KiB by the formula (the one before it
    is served): NotImplementedError with a message, nothing is launched, and the joint's gradient
    calls and the members' own calls go on serving."""
    from tabcorr_amd import JointLikelihood
    theta = synthetic.zheng07_draws(5, seed=2)
    limit = largest(lambda n_prim: forward_lds(4 * n_prim, 8) <= LDS_LIMIT)
    pair = [('auto', (5, )), ('cross', (3, ))]
    for n_prim, parts, match in ((6, [('auto', (21, )), ('cross', (3, ))], 'r tile'),
                                 (limit, pair, None), (limit + 1, pair, 'LDS')):
        tables = joint_reference.make_tables(n_prim, 2, parts)
        halotabs = [make_halotab(table) for table in tables]
        joint = JointLikelihood(halotabs)
        n = joint.n_r_total
        if match is None:
            ngal, xis = joint.predict_batch(theta)
            for halotab, xi in zip(halotabs, xis):
                own = halotab.predict_batch(theta)
                assert_rel(ngal, own[0], RTOL, 'ngal at the limit')
                assert_rel(xi, own[1], RTOL, 'xi at the limit')
            assert same_bits((joint.chi2_batch(theta, np.ones(n), np.eye(n))[0], ), (ngal, ))
        else:
            with pytest.raises(NotImplementedError, match=match):
                joint.predict_batch(theta)
            with pytest.raises(NotImplementedError, match=match):
                joint.chi2_batch(theta, np.ones(n), np.eye(n))
        check_everything_still_serves(tables, halotabs, joint)
