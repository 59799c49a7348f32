"""The joint likelihood of several tables on the device (JointLikelihood, the tc_joint_* entry
points) against the joint reference of joint_reference.py: the per-table reference Jacobians
concatenated, chi2, its gradient and the Fisher matrix in NumPy against a precision matrix that
couples the tables.  Needs an MI355X.

Allowances are the existing ones with N = sum n_r for n_r (joint_reference.py), no new number.
Every case prints its largest error in units of its allowance.  Draws: grad_reference.stress_draws
(seed 5), every one of them usable -- no draw is left out.
"""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assembias_grad_reference  # noqa: E402
import fisher_reference  # noqa: E402
import grad_reference  # noqa: E402
import joint_reference  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    D, LDS_LIMIT, RTOL, check_still_serves, device_call, largest, same_bits)
from util import assert_rel, load_golden, table_from_golden  # noqa: E402

pytestmark = pytest.mark.gpu

DRAW_COUNTS = [1, D + 1, 2 * D + 1]          # partial and several workgroups
N_MAX = max(DRAW_COUNTS)

AUTO3, CROSS5 = ('auto', (3, )), ('cross', (5, ))
# name -> (n_prim, n_sec, parts).  18 bins; 36 bins (more than two row tiles, no multiple of 16);
# 32 bins (whole tiles); the order reversed; 9 auto r rows over 4 waves in tables of fewer r bins
# than waves, a cross table between them; no auto table at all.
JOINTS = {
    'auto3-cross5-18': (9, 1, [AUTO3, CROSS5]),
    'auto3-cross5-36': (9, 2, [AUTO3, CROSS5]),
    'auto3-cross5-32': (16, 1, [AUTO3, CROSS5]),
    'cross5-auto3-36': (9, 2, [CROSS5, AUTO3]),
    'auto3-cross2-auto6-36': (9, 2, [AUTO3, ('cross', (2, )), ('auto', (6, ))]),
    'cross5-cross3-36': (9, 2, [CROSS5, ('cross', (3, ))]),
}
REAL = 'bolplanck'                           # w_p + DeltaSigma: 60 bins, N = 38, 10^2 against 10^14
NAMES = list(JOINTS) + [REAL]

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


def get_reference(name, modulate, assembias=False):
    """N_MAX draws and their joint reference (ngal, xi, dngal, dxi, scale), computed once and never
    modified: a batch of n draws is the first n of them.  Plain: seed 5, and every draw is usable.
    Decorated: the rule of test_gpu_assembias_grad.py -- the first seed from 5 on with which every
    draw is usable and the reference's own rounding stays below a tenth of the allowance, chosen
    from the reference alone."""
    key = (name, modulate, assembias)
    if key not in _references:
        tables = get_joint(name, assembias)[0]
        if not assembias:
            theta = grad_reference.stress_draws(tables[0], N_MAX, seed=5)
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
        assert len(theta) == N_MAX and joint_reference.usable(reference), key
        for array in (theta, ) + reference:
            array.setflags(write=False)
        _references[key] = (theta, reference)
    return _references[key]


def operands(name, reference, symmetric):
    """A data vector near draw 3's joint vector and a precision matrix that couples the tables
    (in units of |xi| for the real pair, whose tables differ by twelve orders of magnitude)."""
    data, precision = joint_reference.coupled_data(reference[1][3], symmetric, name == REAL)
    first = get_joint(name)[2].slices[0].stop
    assert np.all(precision[:first, first:] != 0.0)
    return data, precision


def concatenated(parts, leading):
    """The per-table results of predict_batch_grad on one joint axis."""
    return np.concatenate([np.reshape(part, leading + (-1, )) for part in parts], axis=-1)


def check_symmetric_to_the_bit(fisher):
    assert np.array_equal(fisher, fisher.transpose(0, 2, 1), equal_nan=True)


def check_all(name, n_draws, modulate, assembias):
    tables, halotabs, joint = get_joint(name, assembias)
    theta, reference = get_reference(name, modulate, assembias)
    theta = theta[:n_draws]
    q = theta.shape[1]
    kwargs = dict(modulate_with_cenocc=modulate, assembias=assembias)
    what = '%s n=%d modulate=%s assembias=%s' % (name, n_draws, modulate, assembias)

    ngal, xis, dngal, dxis = joint.predict_batch_grad(theta, **kwargs)
    assert ngal.shape == (n_draws, ) and dngal.shape == (n_draws, q)
    for halotab, xi, dxi in zip(halotabs, xis, dxis):
        assert xi.shape == (n_draws, ) + tuple(halotab.tpcf_shape)
        assert dxi.shape == (n_draws, q) + tuple(halotab.tpcf_shape)
    assert_rel(ngal, reference[0][:n_draws], RTOL, what + ' ngal')
    for part, xi in zip(joint.slices, xis):
        # (per table: the floor of assert_rel is that of the table's own scale)
        assert_rel(xi.reshape(n_draws, -1), reference[1][:n_draws, part], RTOL, what + ' xi')
    joint_reference.check_derivatives(dngal, concatenated(dxis, (n_draws, q)), reference, what)

    dxi_ref, a = joint_reference.fisher_jacobian(reference)
    for symmetric in (True, False):
        data, precision = operands(name, reference, symmetric)
        label = '%s symmetric=%s' % (what, symmetric)
        grad = joint.chi2_grad_batch(theta, data, precision, **kwargs)
        assert [g.shape for g in grad] == [(n_draws, ), (n_draws, ), (n_draws, q), (n_draws, q)]
        joint_reference.check_chi2(grad[1], grad[3], reference, data, precision, label)
        full = joint.chi2_fisher_batch(theta, data, precision, **kwargs)
        assert full[4].shape == (n_draws, q, q)
        # the chi2 outputs do not depend on whether the Fisher matrix is asked for
        assert same_bits(full[:4], grad)
        assert same_bits((full[0], full[2]), (ngal, dngal))
        fisher_reference.check(full[4], dxi_ref, a, precision, 'fisher ' + label)
        check_symmetric_to_the_bit(full[4])
        # ... and the matrix not on the data
        forecast = joint.fisher_batch(theta, precision, **kwargs)
        assert same_bits(forecast, (full[0], full[2], full[4]))
    # the per-table list form of the data
    parts = [data[part].reshape(halotab.tpcf_shape)
             for part, halotab in zip(joint.slices, halotabs)]
    assert same_bits(joint.chi2_fisher_batch(theta, parts, precision, **kwargs), full)


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('name', NAMES)
def test_joint_matches_reference(name, n_draws, modulate):
    check_all(name, n_draws, modulate, False)


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', [1, N_MAX])
@pytest.mark.parametrize('name', ['auto3-cross5-36', 'auto3-cross2-auto6-36'])
def test_decorated_joint_matches_reference(name, n_draws, modulate):
    check_all(name, n_draws, modulate, True)


# ---- bits -------------------------------------------------------------------------------------

def device_predict(joint, theta, flags=0):
    device = joint.to_device()
    n, q, total = len(theta), theta.shape[1], joint.n_r_total
    return device_call(device, 'tc_joint_predict_grad_batch_device', [theta, q, n, 10, flags],
                       [n, (n, total), (n, q), (n, q, total)], synchronize='tc_joint_synchronize')


def device_chi2(joint, theta, data, precision, flags=0, fisher=True):
    """tc_joint_chi2_grad_batch_device (data and precision are host arrays there too); fisher
    False: NULL is passed for it (device_call allocates its outputs, so the entry is called by
    hand)."""
    from tabcorr_amd import _lib
    device = joint.to_device()
    n, q = len(theta), theta.shape[1]
    data, precision = _lib.contiguous(data), _lib.contiguous(precision)
    arguments = [theta, q, n, 10, flags, _lib.as_double_p(data), _lib.as_double_p(precision)]
    shapes = [n, n, (n, q), (n, q)]
    if fisher:
        return device_call(device, 'tc_joint_chi2_grad_batch_device', arguments,
                           shapes + [(n, q, q)], synchronize='tc_joint_synchronize')
    return device_call(WithoutFisher(device), 'chi2_without_fisher', arguments, shapes,
                       synchronize='tc_joint_synchronize')


class WithoutFisher:
    """device_call's view of a joint whose likelihood entry is given fisher = NULL behind the
    outputs that device_call allocates."""

    def __init__(self, device):
        self.lock, self.handle, self.lib = device.lock, device.handle, self
        self.library = device.lib

    def __getattr__(self, name):
        if name == 'chi2_without_fisher':
            return lambda handle, *passed: self.library.tc_joint_chi2_grad_batch_device(
                handle, *passed, None)
        return getattr(self.library, name)


@pytest.mark.parametrize('name', ['auto3-cross5-36', 'auto3-cross2-auto6-36', 'cross5-cross3-36',
                                  REAL])
def test_exact_properties(name):
    """What follows from the design, no tolerance: the device-pointer entries return the bits of
    the host-array ones; a draw alone has the bits it has inside a batch of 33; with fisher = NULL
    the chi2 outputs are the same bits."""
    _, _, joint = get_joint(name)
    theta, reference = get_reference(name, False)
    data, precision = operands(name, reference, False)
    ngal, xis, dngal, dxis = joint.predict_batch_grad(theta)
    flat = (ngal, concatenated(xis, (N_MAX, )), dngal, concatenated(dxis, (N_MAX, 5)))
    full = joint.chi2_fisher_batch(theta, data, precision)
    assert all(np.all(np.isfinite(a)) for a in flat + full)
    for n in DRAW_COUNTS:
        assert same_bits(device_predict(joint, theta[:n]), [a[:n] for a in flat])
        assert same_bits(device_chi2(joint, theta[:n], data, precision), [a[:n] for a in full])
    assert same_bits(device_chi2(joint, theta, data, precision, fisher=False), full[:4])
    for row in (0, D, N_MAX - 1):
        one = joint.predict_batch_grad(theta[row:row + 1])
        assert same_bits((one[0], concatenated(one[1], (1, )), one[2],
                          concatenated(one[3], (1, 5))), [a[row:row + 1] for a in flat])
        assert same_bits(joint.chi2_fisher_batch(theta[row:row + 1], data, precision),
                         [a[row:row + 1] for a in full])
    # modulate_with_cenocc and the decoration through the flags of the device entry
    from tabcorr_amd import _lib
    modulated = joint.chi2_fisher_batch(theta, data, precision, modulate_with_cenocc=True)
    assert same_bits(device_chi2(joint, theta, data, precision,
                                 flags=_lib.FLAG_MODULATE_WITH_CENOCC), modulated)
    assert not np.array_equal(modulated[1], full[1])


SINGLE = [((9, 2, (3, )), 'auto'), ((16, 1, (5, )), 'auto'), ((9, 2, (5, )), 'cross'),
          ((33, 2, (3, )), 'cross')]


@pytest.mark.parametrize('assembias', [False, True], ids=['plain', 'decorated'])
@pytest.mark.parametrize('shape,mode', SINGLE,
                         ids=['%s-%dx%d' % (m, s[0], s[1]) for s, m in SINGLE])
def test_joint_of_one_table_has_the_bits_of_the_table(shape, mode, assembias):
    """The pieces and their order are those of the table kernels: a joint of ONE table returns the
    bits of that table's own predict_batch_grad / chi2_fisher_batch -- mode auto the same products
    on the matrix pipe, mode cross the one fma chain in bin order that the slabs of
    grad_cross_kernel amount to (132 bins: three slabs)."""
    from tabcorr_amd import JointLikelihood
    module = assembias_grad_reference if assembias else grad_reference
    make = assembias_grad_reference.synthetic_table if assembias else synthetic.synthetic_table
    table = make(shape[0], shape[1], shape[2], mode, seed=3)
    halotab = make_halotab(table)
    joint = JointLikelihood([halotab])
    theta = module.stress_draws(table, N_MAX, seed=5)
    for modulate in (False, True):
        kwargs = dict(modulate_with_cenocc=modulate, assembias=assembias)
        own = halotab.predict_batch_grad(theta, **kwargs)
        got = joint.predict_batch_grad(theta, **kwargs)
        assert same_bits((got[0], got[1][0], got[2], got[3][0]), own)
        data, precision = joint_reference.coupled_data(own[1][3], False)
        assert same_bits(joint.chi2_fisher_batch(theta, data, precision, **kwargs),
                         halotab.chi2_fisher_batch(theta, data, precision, **kwargs))


def test_real_tables_alone_have_their_own_bits():
    _, halotabs, _ = get_joint(REAL)
    from tabcorr_amd import JointLikelihood
    theta, _ = get_reference(REAL, False)
    for halotab in halotabs:
        own = halotab.predict_batch_grad(theta)
        got = JointLikelihood([halotab]).predict_batch_grad(theta)
        assert same_bits((got[0], got[1][0], got[2], got[3][0]), own)


# ---- block structure ----------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['auto3-cross5-36', REAL])
def test_block_diagonal_precision_gives_the_sum_of_the_tables(name):
    """With a block-diagonal precision chi2, dchi2 and fisher of [auto, cross] are the sums of
    the two tables' own chi2_fisher_batch results, within the sum of the two tables' allowances
    (those of test_gpu_grad.py and fisher_reference.py for each table alone)."""
    tables, halotabs, joint = get_joint(name)
    theta, reference = get_reference(name, False)
    data, precision = operands(name, reference, False)
    first = joint.slices[0].stop
    precision = precision.copy()
    precision[:first, first:] = 0.0
    precision[first:, :first] = 0.0
    got = joint.chi2_fisher_batch(theta, data, precision)
    total = [np.zeros_like(a) for a in got[1:]]
    allow = [np.zeros_like(a) for a in (got[1], got[3], got[4])]
    for part, halotab in zip(joint.slices, halotabs):
        block = np.ascontiguousarray(precision[part, part])
        own = halotab.chi2_fisher_batch(theta, data[part], block)
        assert same_bits((own[0], own[2]), (got[0], got[2]))
        for k in (1, 3, 4):
            total[k - 1] += own[k]
        alone = tuple(np.ascontiguousarray(a[..., part]) if a.ndim > 1 and i in (1, 3, 4)
                      else a for i, a in enumerate(reference))
        expect = joint_reference.chi2_reference(alone, data[part], block)
        allow[0] += expect[2]
        allow[1] += expect[3]
        dxi, a = joint_reference.fisher_jacobian(alone)
        allow[2] += fisher_reference.allowance(dxi, a, block)
    for k, bound in zip((1, 3, 4), allow):
        error = np.abs(got[k] - total[k - 1])
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(error == 0.0, 0.0, error / bound)
        print('%s output %d: max error / allowance = %.3g' % (name, k, np.max(ratio)))
        assert np.all(error <= bound)


# ---- refusals -----------------------------------------------------------------------------------

def joint_lds(n_bins, n_central, n_r_total, chi2, n_params=5):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    _lib.check(_lib.load().tc_debug_joint_lds_bytes(n_bins, n_central, n_r_total, int(chi2),
                                                    n_params, ctypes.byref(got)))
    return got.value


def check_joint_still_serves(name='auto3-cross5-36'):
    _, _, joint = get_joint(name)
    theta, reference = get_reference(name, False)
    ngal = joint.predict_batch_grad(theta[:3])[0]
    assert_rel(ngal, reference[0][:3], RTOL)


def test_a_joint_beyond_the_lds_is_refused_on_the_host():
    """The largest n_prim (one secondary bin: n_prim centrals and n_prim satellites) whose joint
    [auto (3,), cross (5,)] fits 160 KiB, by the formula; one more is refused -- also for a joint
    of cross tables only, each of which is served alone --, and nothing is launched: the tables go
    on serving, and so does a joint."""
    from tabcorr_amd import JointLikelihood
    for parts, chi2 in (([AUTO3, CROSS5], True), ([CROSS5, ('cross', (3, ))], False)):
        limit = largest(lambda n: joint_lds(2 * n, n, 8, chi2) <= LDS_LIMIT)
        for n_prim, served in ((limit, True), (limit + 1, False)):
            tables = joint_reference.make_tables(n_prim, 1, parts)
            halotabs = [make_halotab(table) for table in tables]
            joint = JointLikelihood(halotabs)
            theta = synthetic.zheng07_draws(5, seed=2)
            data, precision = np.ones(8), np.eye(8)
            call = ((lambda: joint.chi2_grad_batch(theta, data, precision)) if chi2
                    else (lambda: joint.predict_batch_grad(theta)))
            if served:
                assert np.all(np.isfinite(call()[0]))
            else:
                with pytest.raises(NotImplementedError, match='LDS'):
                    call()
                if not chi2:
                    # each cross table alone is served: its kernel walks the bins in slabs
                    assert np.all(np.isfinite(halotabs[0].predict_batch_grad(theta)[0]))
            for table, halotab in zip(tables, halotabs):
                check_still_serves(halotab, table)
    check_joint_still_serves()


def test_unsupported_requests_leave_the_joint_usable():
    from tabcorr_amd import JointLikelihood, _lib
    name = 'auto3-cross5-36'
    tables, halotabs, joint = get_joint(name)
    theta, _ = get_reference(name, False)
    device = joint.to_device()
    lib = device.lib
    n = 3
    out = [np.empty(n), np.empty((n, 8)), np.empty((n, 5)), np.empty((n, 5, 8))]
    pointers = [_lib.as_double_p(a) for a in out]
    small = np.ascontiguousarray(theta[:n])
    for flags, match in ((_lib.FLAG_LEAUTHAUD11, 'Zheng07 family'),
                         (_lib.FLAG_SEPARATE_GAL_TYPE, 'separate_gal_type'),
                         (32, 'unknown flags')):
        with device.lock:
            status = lib.tc_joint_predict_grad_batch(device.handle, _lib.as_double_p(small), 5, n,
                                                     10, flags, *pointers)
        assert status == _lib.TC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError, match=match):
            _lib.check(status)
    # the wrong number of columns for the family the flags select
    with device.lock:
        assert lib.tc_joint_predict_grad_batch(
            device.handle, _lib.as_double_p(small), 5, n, 10, _lib.FLAG_ASSEMBIAS,
            *pointers) == _lib.TC_ERR_INVALID
    with pytest.raises(NotImplementedError):
        joint.predict_batch_grad(np.zeros((3, 14)), family='leauthaud11')
    # a float32 table and a table with other bins: no joint, in Python and in C
    single = make_halotab(tables[1], compute_dtype='float32')
    other_table = synthetic.synthetic_table(9, 1, (5, ), 'cross', seed=3)
    other = make_halotab(other_table)
    for halotab, match in ((single, 'float64'), (other, 'gal_type')):
        with pytest.raises(ValueError, match=match):
            JointLikelihood([halotabs[0], halotab])
        handles = (ctypes.c_void_p * 2)(halotabs[0].to_device().handle.value,
                                        halotab.to_device().handle.value)
        handle = ctypes.c_void_p()
        assert lib.tc_joint_create(handles, 2, ctypes.byref(handle)) == _lib.TC_ERR_INVALID
        assert b'table 1' in lib.tc_last_error() and handle.value is None
    info = (ctypes.c_int(), ctypes.c_int(), (ctypes.c_int * 2)())
    _lib.check(lib.tc_joint_info(device.handle, ctypes.byref(info[0]), ctypes.byref(info[1]),
                                 info[2]))
    assert (info[0].value, info[1].value, list(info[2])) == (2, 8, [0, 3])
    for table, halotab in zip(tables + [other_table], halotabs + [other]):
        check_still_serves(halotab, table)
    # (1e-5: the float32 path's stated tolerance)
    check_still_serves(single, tables[1], rtol=1e-5)
    check_joint_still_serves(name)


# ---- un-batched forms ---------------------------------------------------------------------------

def model_of(theta, modulate, decorated):
    from tabcorr_amd import Zheng07Model
    from tabcorr_amd.models import ZHENG07_ASSEMBIAS_KEYS
    model = Zheng07Model(redshift=0.0, modulate_with_cenocc=modulate,
                         sec_haloprop_key='halo_nfw_conc' if decorated else None)
    for key, value in zip(ZHENG07_ASSEMBIAS_KEYS, theta):
        model.param_dict[key] = value
    return model


@pytest.mark.parametrize('decorated', [False, True], ids=['plain', 'decorated'])
def test_model_object_calls(decorated):
    """predict_grad(model) and chi2_fisher(model, data, precision) return the bits of row 0 of the
    batched calls, keyed by the parameter names."""
    from tabcorr_amd.models import ZHENG07_ASSEMBIAS_KEYS, ZHENG07_KEYS
    name = 'auto3-cross5-36'
    _, halotabs, joint = get_joint(name, decorated)
    theta, reference = get_reference(name, True, decorated)
    data, precision = operands(name, reference, False)
    keys = ZHENG07_ASSEMBIAS_KEYS if decorated else ZHENG07_KEYS
    model = model_of(theta[0], True, decorated)
    kwargs = dict(modulate_with_cenocc=True, assembias=decorated)
    batch = joint.predict_batch_grad(theta, **kwargs)
    ngal, xis, dngal, dxis = joint.predict_grad(model, assembias=decorated)
    assert isinstance(ngal, float) and ngal == batch[0][0]
    assert list(dngal) == list(keys) == list(dxis)
    for t, halotab in enumerate(halotabs):
        assert xis[t].shape == tuple(halotab.tpcf_shape)
        assert np.array_equal(xis[t], batch[1][t][0])
        for k, key in enumerate(keys):
            assert np.array_equal(dxis[key][t], batch[3][t][0, k])
    assert [dngal[key] for key in keys] == list(batch[2][0])
    full = joint.chi2_fisher_batch(theta, data, precision, **kwargs)
    one = joint.chi2_fisher(model, data, precision, assembias=decorated)
    assert one[0] == full[0][0] and one[1] == full[1][0]
    assert list(one[2]) == list(keys) == list(one[3])
    assert [one[2][key] for key in keys] == list(full[2][0])
    assert [one[3][key] for key in keys] == list(full[3][0])
    assert np.array_equal(one[4], full[4][0])
    if decorated:
        # without the keyword a decorated model stays refused
        with pytest.raises(NotImplementedError, match='plain Zheng07'):
            joint.predict_grad(model)
