"""The Python layer between the classes and the C ABI, without a GPU: the occupation seam's one
call path (`tabcorr_amd/_seam.py`, `_lib.SEAM_ENTRIES`), the model resolver of the un-batched
derivative calls (`_grad.model_columns`) and the base the two joints share, through a stub device
that records what an entry is called with and writes a known pattern through the output
pointers."""

import ctypes
import threading

import numpy as np
import pytest

from tabcorr_amd import (Interpolator, JointInterpolator, JointLikelihood, Leauthaud11Model,
                         TabCorr, Zheng07Model, _forward, _grad, _lib, _seam, synthetic)
from tabcorr_amd.models import (LEAUTHAUD11_KEYS, ZHENG07_ASSEMBIAS_KEYS, ZHENG07_KEYS)

V, D, I64, U, INT = (ctypes.c_void_p, _lib.c_double_p, ctypes.c_int64, ctypes.c_uint,
                     ctypes.c_int)
# the seam's entries and their argument lists, as the commit before `SEAM_ENTRIES` spelt them
SEAM_SYMBOLS = {('table', 'predict'): 'tc_predict_occupation_vjp_batch',
                ('table', 'chi2'): 'tc_chi2_occupation_grad_batch',
                ('joint', 'predict'): 'tc_joint_predict_occupation_vjp_batch',
                ('joint', 'chi2'): 'tc_joint_chi2_occupation_grad_batch',
                ('interp', 'predict'): 'tc_interp_predict_occupation_vjp_batch',
                ('interp', 'chi2'): 'tc_interp_chi2_occupation_grad_batch'}
SEAM_SIGNATURES = {
    'tc_predict_occupation_vjp_batch': [V, D, I64, U, D, D, D, D, D],
    'tc_chi2_occupation_grad_batch': [V, D, I64, U, D, D, D, D, D],
    'tc_joint_predict_occupation_vjp_batch': [V, D, I64, U, D, D, D, D, D],
    'tc_joint_chi2_occupation_grad_batch': [V, D, I64, U, D, D, D, D, D],
    'tc_interp_predict_occupation_vjp_batch': [V, D, D, I64, U, D, D, D, D, D, D],
    'tc_interp_chi2_occupation_grad_batch': [V, D, D, I64, U, D, D, D, D, D, D, D],
    'tc_predict_occupation_vjp_batch_device': [V, V, I64, U, V, V, V, V, V],
    'tc_chi2_occupation_grad_batch_device': [V, V, I64, U, D, D, V, V, V],
    'tc_joint_predict_occupation_vjp_batch_device': [V, V, I64, U, V, V, V, V, V],
    'tc_joint_chi2_occupation_grad_batch_device': [V, V, I64, U, D, D, V, V, V],
    'tc_interp_predict_occupation_vjp_batch_device': [V, V, V, I64, U, V, V, V, V, V, V],
    'tc_interp_chi2_occupation_grad_batch_device': [V, V, V, I64, U, D, D, V, V, V, V, V]}
N_DRAWS = 3
SHAPES = [(5, ), (3, 4)]


# ---- the stub ------------------------------------------------------------------------------------

class Pointer:
    """What `_lib.as_double_p` returns under the `stub` fixture: the array itself."""

    def __init__(self, array):
        assert isinstance(array, np.ndarray)
        self.array = array


class Lock:
    def __init__(self):
        self.held = 0
        self.entered = 0

    def __enter__(self):
        self.held += 1
        self.entered += 1

    def __exit__(self, *exc):
        self.held -= 1


def pattern(j, size):
    """What the stub writes through output `j` of a call."""
    return 1000.0 * (j + 1) + np.arange(size)


class Library:
    """Every attribute is an entry that checks its arguments against `_lib.SIGNATURES[symbol]`
    (their number; an array or NULL where the entry takes a double pointer, the handle first, an
    integer elsewhere), records ``(symbol, arguments)`` and writes `pattern` through its last
    `n_outputs` pointers."""

    def __init__(self, device):
        self.device = device
        self.calls = []
        self.n_outputs = 0

    def __getattr__(self, symbol):
        signature = _lib.SIGNATURES[symbol]

        def entry(*arguments):
            assert len(arguments) == len(signature), (symbol, len(arguments), len(signature))
            assert self.device.lock.held == 1
            assert arguments[0] is self.device.handle
            for argument, kind in zip(arguments[1:], signature[1:]):
                if kind is D:
                    assert argument is None or isinstance(argument, Pointer), (symbol, argument)
                    if argument is not None:
                        assert argument.array.dtype == np.float64
                        assert argument.array.flags.c_contiguous
                else:
                    assert isinstance(argument, (int, np.integer)), (symbol, argument)
            self.calls.append((symbol, arguments))
            outputs = arguments[len(arguments) - self.n_outputs:]
            for j, argument in enumerate(outputs):
                if argument is not None:
                    argument.array.reshape(-1)[:] = pattern(j, argument.array.size)
            return _lib.TC_OK
        return entry


class Device:
    def __init__(self, n_r):
        self.handle = ctypes.c_void_p(1234)
        self.lock = Lock()
        self.n_r = n_r
        self.lib = Library(self)


@pytest.fixture
def stub(monkeypatch):
    """`Device(n_r)` factories whose entries see the arrays: `_lib.as_double_p` hands them on."""
    monkeypatch.setattr(_lib, 'as_double_p', Pointer)
    monkeypatch.setattr(_forward, 'p', Pointer)

    def make(n_r, n_outputs):
        device = Device(n_r)
        device.lib.n_outputs = n_outputs
        return device
    return make


def halotab_of(table):
    return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                               table['attrs'])


def make_interpolator(tpcf_shape, mode='auto'):
    """A (4, 5) grid in two interleaved classes, as tests/test_interp_vjp_cpu.py builds one."""
    tables, keys, points = synthetic.synthetic_interpolator((4, 5), 3, 1, tpcf_shape, mode, seed=7)
    for k, table in enumerate(tables):
        if k % 2:
            table['gal_type'] = table['gal_type'].copy()
            table['gal_type']['n_h'] *= 1.3
    interp = Interpolator([halotab_of(t) for t in tables],
                          {key: points[:, d] for d, key in enumerate(keys)})
    return interp, np.tile(points.mean(axis=0), (N_DRAWS, 1))


# ---- the signatures ------------------------------------------------------------------------------

def test_seam_signatures_are_the_hand_written_ones():
    assert _lib.SEAM_ENTRIES == SEAM_SYMBOLS
    for name, expect in SEAM_SIGNATURES.items():
        assert _lib.SIGNATURES[name] == expect, name
    seam = [name for name in _lib.SIGNATURES if 'occupation_vjp' in name or
            'occupation_grad' in name]
    assert sorted(seam) == sorted(SEAM_SIGNATURES)


# ---- the arguments of `_seam.call` ---------------------------------------------------------------

# (a table has no forward-only form; g_ngal belongs to the form 'predict')
SEAM_CASES = [(kind, form, mode) for kind, form in SEAM_SYMBOLS
              for mode in ('backward', 'no_g_ngal', 'forward')
              if not (mode == 'forward' and kind == 'table') and
              not (mode == 'no_g_ngal' and form == 'chi2')]


@pytest.mark.parametrize('kind,form,mode', SEAM_CASES)
def test_seam_call_arguments(stub, kind, form, mode):
    """The symbol, which arguments are NULL, and the arrays -- C-contiguous float64 (the stub
    checks) of the expected sizes, the caller's own where they are inputs."""
    interp = kind == 'interp'
    n_bins, n_r = 6, 5
    n_x = {'predict': 1, 'chi2': 2}[form] if interp else 0
    device = stub(n_r, 3 + n_x)
    occupation = np.ones((N_DRAWS, 2, n_bins) if interp else (N_DRAWS, n_bins))
    x = np.zeros((N_DRAWS, 2)) if interp else None
    g_xi, g_ngal = np.ones((N_DRAWS, n_r)), np.ones(N_DRAWS)
    data, precision = np.zeros(n_r), np.eye(n_r)
    backward = mode != 'forward'
    if form == 'predict':
        cotangents = (g_xi, None if mode == 'no_g_ngal' else g_ngal) if backward else None
        got = _seam.call(device, kind, form, occupation, x, cotangents=cotangents)
        middle = [None, None] if not backward else [cotangents[1], g_xi]
    else:
        got = _seam.call(device, kind, form, occupation, x, operands=(data, precision),
                         gradient=backward)
        middle = [data, precision]
    symbol, arguments = device.lib.calls[-1]
    assert len(device.lib.calls) == 1 and device.lock.entered == 1
    assert symbol == SEAM_SYMBOLS[kind, form]
    inputs = [occupation] + ([x] if interp else [])
    head = arguments[1:1 + len(inputs)]
    assert all(pointer.array is array for pointer, array in zip(head, inputs))
    assert arguments[1 + len(inputs):3 + len(inputs)] == (N_DRAWS, 0)
    for pointer, array in zip(arguments[3 + len(inputs):5 + len(inputs)], middle):
        assert (pointer is None) if array is None else (pointer.array is array)
    outputs = arguments[5 + len(inputs):]
    sizes = [N_DRAWS, N_DRAWS * n_r if form == 'predict' else N_DRAWS]
    sizes += ([occupation.size] + [2 * N_DRAWS] * n_x) if backward else [None] * (1 + n_x)
    assert len(outputs) == len(sizes) == len(got)
    for j, (pointer, size, result) in enumerate(zip(outputs, sizes, got)):
        if size is None:
            assert pointer is None and result is None
        else:
            assert pointer.array is result and result.size == size
            assert np.array_equal(result.reshape(-1), pattern(j, size))
    # the flat arrays, in the shapes of their inputs where they are derivatives
    assert got[1].shape == ((N_DRAWS, n_r) if form == 'predict' else (N_DRAWS, ))
    if backward:
        assert got[2].shape == occupation.shape
        assert all(result.shape == x.shape for result in got[3:])


def test_cotangents_shapes_and_messages():
    g_xi, g_ngal = _seam.cotangents(np.ones((3, 3, 4)), np.ones(3), 3, True, (3, 4))
    assert g_xi.shape == (3, 12) and g_ngal.shape == (3, )
    assert g_xi.flags.c_contiguous and g_xi.dtype == np.float64
    g_xi, g_ngal = _seam.cotangents(np.ones((3, 4), dtype=np.float32), 2, 1, False, (3, 4))
    assert g_xi.shape == (1, 12) and g_ngal.shape == (1, ) and g_ngal[0] == 2.0
    assert g_xi.dtype == np.float64
    assert _seam.cotangents(np.ones((3, 5)), None, 3, True, (5, ))[1] is None
    for bad in (np.ones((2, 5)), np.ones(5), np.ones((3, 6))):
        with pytest.raises(ValueError, match=r'g_xi must have shape \(3, 5\), got'):
            _seam.cotangents(bad, None, 3, True, (5, ))
    with pytest.raises(ValueError, match=r'g_xi must have shape \(5,\), got'):
        _seam.cotangents(np.ones((1, 5)), None, 1, False, (5, ))
    for bad in (np.ones(2), np.ones((3, 1)), 1.0):
        with pytest.raises(ValueError, match=r'g_ngal must have shape \(3,\), got'):
            _seam.cotangents(np.ones((3, 5)), bad, 3, True, (5, ))
    with pytest.raises(ValueError, match=r'g_ngal must have shape \(\), got'):
        _seam.cotangents(np.ones(5), np.ones(1), 1, False, (5, ))


# ---- what the classes return ---------------------------------------------------------------------

@pytest.mark.parametrize('tpcf_shape', SHAPES)
def test_table_seam_outputs(stub, tpcf_shape):
    table = synthetic.synthetic_table(3, 1, tpcf_shape, 'auto', seed=1)
    halotab = halotab_of(table)
    n_bins, n_r = len(table['gal_type']), int(np.prod(tpcf_shape))
    halotab._device = device = stub(n_r, 3)
    occupation = np.ones((N_DRAWS, n_bins))
    g_xi = np.ones((N_DRAWS, ) + tpcf_shape)
    ngal, xi, g_occupation = halotab.predict_vjp(occupation, g_xi, np.ones(N_DRAWS))
    assert np.array_equal(ngal, pattern(0, N_DRAWS))
    assert np.array_equal(xi, pattern(1, N_DRAWS * n_r).reshape((N_DRAWS, ) + tpcf_shape))
    assert np.array_equal(g_occupation, pattern(2, occupation.size).reshape(occupation.shape))
    ngal, xi, g_occupation = halotab.predict_vjp(occupation[0], g_xi[0])
    assert device.lib.calls[-1][1][4] is None
    assert ngal == 1000.0 and np.ndim(ngal) == 0
    assert np.array_equal(xi, pattern(1, n_r).reshape(tpcf_shape))
    assert np.array_equal(g_occupation, pattern(2, n_bins))
    data, precision = np.zeros(tpcf_shape), np.eye(n_r)
    ngal, chi2, dchi2 = halotab.chi2_grad_occupation(occupation, data, precision)
    assert np.array_equal(ngal, pattern(0, N_DRAWS)) and np.array_equal(chi2, pattern(1, N_DRAWS))
    assert np.array_equal(dchi2, pattern(2, occupation.size).reshape(occupation.shape))
    ngal, chi2, dchi2 = halotab.chi2_grad_occupation(occupation[0], data, precision)
    assert (ngal, chi2) == (1000.0, 2000.0) and np.array_equal(dchi2, pattern(2, n_bins))
    assert [symbol for symbol, _ in device.lib.calls] == [
        SEAM_SYMBOLS['table', 'predict']] * 2 + [SEAM_SYMBOLS['table', 'chi2']] * 2


def test_joint_seam_outputs(stub, monkeypatch):
    """An auto table of shape (5, ) and a cross table of shape (3, 4): the joint axis of 17."""
    tables = [synthetic.synthetic_table(3, 1, shape, mode, seed=1)
              for shape, mode in zip(SHAPES, ('auto', 'cross'))]
    joint = JointLikelihood([halotab_of(t) for t in tables])
    n_bins, n = len(tables[0]['gal_type']), joint.n_r_total
    assert n == 17
    device = stub(n, 3)
    monkeypatch.setattr(joint, 'to_device', lambda: device)
    occupation = np.ones((N_DRAWS, n_bins))
    flat = pattern(1, N_DRAWS * n).reshape(N_DRAWS, n)
    expect_xis = [flat[:, :5], flat[:, 5:].reshape(N_DRAWS, 3, 4)]
    g_xis = [np.full((N_DRAWS, 5), 2.0), np.full((N_DRAWS, 3, 4), 3.0)]

    for call, backward in ((lambda: joint.predict_vjp(occupation, g_xis, np.ones(N_DRAWS)), True),
                           (lambda: joint.predict_vjp(occupation, np.ones((N_DRAWS, n))), True),
                           (lambda: joint.predict_occupation(occupation), False)):
        got = call()
        assert np.array_equal(got[0], pattern(0, N_DRAWS))
        assert all(np.array_equal(a, b) for a, b in zip(got[1], expect_xis)) and len(got[1]) == 2
        if backward:
            assert np.array_equal(got[2], pattern(2, occupation.size).reshape(occupation.shape))
        else:
            assert len(got) == 2 and device.lib.calls[-1][1][4:6] == (None, None)
            assert device.lib.calls[-1][1][-1] is None
    # (the list of cotangents arrives concatenated on the joint axis)
    assert np.array_equal(device.lib.calls[0][1][5].array,
                          np.hstack([np.full((N_DRAWS, 5), 2.0), np.full((N_DRAWS, 12), 3.0)]))
    # un-batched: a float, arrays of each table's shape, one row
    ngal, xis, g_occupation = joint.predict_vjp(occupation[0], [g[0] for g in g_xis], 0.5)
    assert ngal == 1000.0 and [a.shape for a in xis] == SHAPES
    assert np.array_equal(xis[1], pattern(1, n)[5:].reshape(3, 4))
    assert np.array_equal(g_occupation, pattern(2, n_bins))
    assert np.array_equal(device.lib.calls[-1][1][4].array, [0.5])
    ngal, xis = joint.predict_occupation(occupation[0])
    assert ngal == 1000.0 and [a.shape for a in xis] == SHAPES
    data, precision = np.zeros(n), np.eye(n)
    ngal, chi2, dchi2 = joint.chi2_grad_occupation(occupation, data, precision)
    assert np.array_equal(chi2, pattern(1, N_DRAWS)) and dchi2.shape == occupation.shape
    assert np.array_equal(dchi2.reshape(-1), pattern(2, occupation.size))
    ngal, chi2 = joint.chi2_occupation(occupation, [data[:5], data[5:]], precision)
    assert np.array_equal(ngal, pattern(0, N_DRAWS)) and np.array_equal(chi2, pattern(1, N_DRAWS))
    assert device.lib.calls[-1][1][-1] is None
    ngal, chi2, dchi2 = joint.chi2_grad_occupation(occupation[0], data, precision)
    assert (ngal, chi2) == (1000.0, 2000.0) and np.array_equal(dchi2, pattern(2, n_bins))
    assert joint.chi2_occupation(occupation[0], data, precision) == (1000.0, 2000.0)
    with pytest.raises(ValueError, match='g_xis'):
        joint.predict_vjp(occupation, None)
    assert joint._device is None


@pytest.mark.parametrize('tpcf_shape', SHAPES)
def test_interpolator_seam_outputs(stub, tpcf_shape):
    interp, x = make_interpolator(tpcf_shape)
    n_bins, n_r = len(interp.tabcorr_list[0].gal_type), int(np.prod(tpcf_shape))
    assert len(interp.class_tables) == 2
    interp._classes_checked = True
    occupation = np.ones((N_DRAWS, 2, n_bins))
    g_xi = np.ones((N_DRAWS, ) + tpcf_shape)
    expect_xi = pattern(1, N_DRAWS * n_r).reshape((N_DRAWS, ) + tpcf_shape)
    expect_docc = pattern(2, occupation.size).reshape(occupation.shape)

    interp._device = device = stub(n_r, 4)
    ngal, xi, g_occupation, g_x = interp.predict_vjp(occupation, x, g_xi, np.ones(N_DRAWS))
    assert np.array_equal(ngal, pattern(0, N_DRAWS)) and np.array_equal(xi, expect_xi)
    assert np.array_equal(g_occupation, expect_docc)
    assert np.array_equal(g_x, pattern(3, x.size).reshape(x.shape))
    assert interp.predict_vjp(occupation, x, g_xi)[3].shape == x.shape
    assert device.lib.calls[-1][1][5] is None and device.lib.calls[-1][1][6] is not None
    ngal, xi = interp.predict_occupation(occupation, x)
    assert np.array_equal(ngal, pattern(0, N_DRAWS)) and np.array_equal(xi, expect_xi)
    assert device.lib.calls[-1][1][5:7] == (None, None)
    assert device.lib.calls[-1][1][-2:] == (None, None)

    interp._device = device = stub(n_r, 5)
    data, precision = np.zeros(tpcf_shape), np.eye(n_r)
    got = interp.chi2_grad_occupation(occupation, x, data, precision)
    assert len(got) == 5 and np.array_equal(got[1], pattern(1, N_DRAWS))
    assert np.array_equal(got[2], expect_docc)
    assert np.array_equal(got[3], pattern(3, x.size).reshape(x.shape))
    assert np.array_equal(got[4], pattern(4, x.size).reshape(x.shape))
    ngal, chi2 = interp.chi2_occupation(occupation, x, data, precision)
    assert np.array_equal(ngal, pattern(0, N_DRAWS)) and np.array_equal(chi2, pattern(1, N_DRAWS))
    assert device.lib.calls[-1][1][-3:] == (None, None, None)
    with pytest.raises(ValueError, match='g_xi'):
        interp.predict_vjp(occupation, x, None)


# ---- the two joints through their base -----------------------------------------------------------

def pointer_positions(arguments):
    return [k for k, argument in enumerate(arguments) if isinstance(argument, Pointer)]


@pytest.mark.parametrize('assembias', [False, True])
def test_joints_pass_x_where_the_signatures_have_it(stub, monkeypatch, assembias):
    """Every batched call of both joints: theta first, x behind theta's column count for a joint
    of interpolators and nowhere for a joint of tables (the stub holds every argument against the
    entry's signature), the operands, the outputs, and the results split by member."""
    tables = [synthetic.synthetic_table(3, 2, shape, mode, seed=1)
              for shape, mode in zip(SHAPES, ('auto', 'cross'))]
    joint = JointLikelihood([halotab_of(t) for t in tables])
    first, x = make_interpolator(SHAPES[0])
    second, _ = make_interpolator(SHAPES[1], 'cross')
    joint_interp = JointInterpolator([first, second])
    n_model = 7 if assembias else 5
    theta = np.hstack([synthetic.zheng07_draws(N_DRAWS, seed=2), np.zeros((N_DRAWS, 2))])
    theta = np.ascontiguousarray(theta[:, :n_model])
    n = 17
    data, precision = np.zeros(n), np.eye(n)
    flags = _lib.FLAG_ASSEMBIAS if assembias else 0
    family = 'assembias' if assembias else 'zheng07'

    for kind, obj, draws, n_extra in (('joint', joint, (theta, ), 0),
                                      ('joint_interp', joint_interp, (theta, x), 2)):
        assert obj.n_r_total == n and obj.kind == kind
        n_cols = n_model + n_extra
        head = (n_model, ) + ((x, ) if n_extra else ()) + (N_DRAWS, 10, flags)

        def check(device, symbol, operands, n_outputs):
            got_symbol, arguments = device.lib.calls[-1]
            assert got_symbol == symbol and len(device.lib.calls) == 1
            assert arguments[1].array is theta
            for argument, expect in zip(arguments[2:], head):
                if isinstance(expect, np.ndarray):
                    assert argument.array is expect
                else:
                    assert argument == expect and not isinstance(argument, Pointer)
            rest = arguments[2 + len(head):]
            assert len(rest) == len(operands) + n_outputs
            for argument, expect in zip(rest, operands):
                assert np.array_equal(argument.array, expect)

        def split(flat, leading):
            return [flat[..., :5].reshape(leading + (5, )),
                    flat[..., 5:].reshape(leading + (3, 4))]

        def device_for(n_outputs):
            device = stub(n, n_outputs)
            monkeypatch.setattr(obj, 'to_device', lambda: device)
            return device

        device = device_for(2)
        ngal, xis = obj.predict_batch(*draws, assembias=assembias)
        check(device, _lib.FORWARD_ENTRIES[kind, 'predict', 'host'], (), 2)
        assert np.array_equal(ngal, pattern(0, N_DRAWS))
        expect = split(pattern(1, N_DRAWS * n).reshape(N_DRAWS, n), (N_DRAWS, ))
        assert all(np.array_equal(a, b) for a, b in zip(xis, expect)) and len(xis) == 2
        device = device_for(2)
        ngal, chi2 = obj.chi2_batch(*draws, data, precision, assembias=assembias)
        check(device, _lib.FORWARD_ENTRIES[kind, 'chi2', 'host'], (data, precision), 2)
        assert np.array_equal(chi2, pattern(1, N_DRAWS))

        device = device_for(4)
        ngal, xis, dngal, dxis = obj.predict_batch_grad(*draws, assembias=assembias)
        check(device, _lib.GRAD_ENTRIES[kind, family, 'predict'], (), 4)
        assert dngal.shape == (N_DRAWS, n_cols)
        expect = split(pattern(3, N_DRAWS * n_cols * n).reshape(N_DRAWS, n_cols, n),
                       (N_DRAWS, n_cols))
        assert all(np.array_equal(a, b) for a, b in zip(dxis, expect)) and len(dxis) == 2
        assert [a.shape for a in xis] == [(N_DRAWS, 5), (N_DRAWS, 3, 4)]
        device = device_for(5)   # (the optional fisher is NULL, behind four outputs)
        got = obj.chi2_grad_batch(*draws, data, precision, assembias=assembias)
        check(device, _lib.GRAD_ENTRIES[kind, family, 'chi2'], (data, precision), 5)
        assert device.lib.calls[-1][1][-1] is None and len(got) == 4
        assert got[3].shape == (N_DRAWS, n_cols)
        device = device_for(5)
        got = obj.chi2_fisher_batch(*draws, [data[:5], data[5:]], precision, assembias=assembias)
        check(device, _lib.GRAD_ENTRIES[kind, family, 'fisher'], (data, precision), 5)
        assert len(got) == 5 and got[4].shape == (N_DRAWS, n_cols, n_cols)
        assert np.array_equal(got[4].reshape(-1), pattern(4, N_DRAWS * n_cols * n_cols))
        device = device_for(5)
        ngal, dngal, fisher = obj.fisher_batch(*draws, precision, assembias=assembias)
        check(device, _lib.GRAD_ENTRIES[kind, family, 'fisher'], (np.zeros(n), precision), 5)
        assert np.array_equal(dngal.reshape(-1), pattern(2, N_DRAWS * n_cols))
        assert np.array_equal(fisher.reshape(-1), pattern(4, N_DRAWS * n_cols * n_cols))
        # the signature has a double pointer at x's place exactly for a joint of interpolators
        signature = _lib.SIGNATURES[_lib.GRAD_ENTRIES[kind, family, 'chi2']]
        assert (signature[3] is D) == (kind == 'joint_interp')
        assert (3 in pointer_positions(device.lib.calls[-1][1])) == (kind == 'joint_interp')
        # refusals come before any device
        monkeypatch.setattr(obj, 'to_device', lambda: pytest.fail('device touched'))
        with pytest.raises(NotImplementedError):
            obj.predict_batch(*draws, assembias=assembias, family='leauthaud11')
        with pytest.raises(ValueError, match='family must be'):
            obj.chi2_batch(*draws, data, precision, assembias=assembias, family='zheng08')
        with pytest.raises(ValueError, match='precision'):
            obj.chi2_fisher_batch(*draws, data[:-1], precision, assembias=assembias)
        with pytest.raises(ValueError, match='theta must have shape'):
            obj.chi2_grad_batch(*draws, data, precision, assembias=not assembias)
    with pytest.raises(ValueError, match='x must have shape'):
        joint_interp.predict_batch_grad(theta, x[:, :1], assembias=assembias)
    outside = x.copy()
    outside[0, 0] = 1e3
    with pytest.raises(ValueError, match='extrapolation'):
        joint_interp.fisher_batch(theta, outside, precision, assembias=assembias)


# ---- the model resolver --------------------------------------------------------------------------

def decorated_model(**kwargs):
    return Zheng07Model(sec_haloprop_key='halo_nfw_conc',
                        mean_occupation_centrals_assembias_param1=0.3,
                        mean_occupation_satellites_assembias_param1=-0.2, **kwargs)


def test_model_columns_zheng07():
    model = Zheng07Model(modulate_with_cenocc=True)
    theta, options, columns, jacobian = _grad.model_columns(model, False, 'predict_grad')
    assert theta.shape == (1, 5) and theta.dtype == np.float64
    assert list(theta[0]) == [model.param_dict[key] for key in ZHENG07_KEYS]
    assert options == {'assembias': False, 'modulate_with_cenocc': True}
    assert list(columns.items()) == [(key, (k, 1.0)) for k, key in enumerate(ZHENG07_KEYS)]
    assert jacobian is None
    # the decorated model, and extra keys behind the model's
    model = decorated_model()
    theta, options, columns, jacobian = _grad.model_columns(model, True, 'fisher', ['a', 'b'],
                                                            leauthaud11=True)
    assert theta.shape == (1, 7)
    assert list(theta[0]) == [model.param_dict[key] for key in ZHENG07_ASSEMBIAS_KEYS]
    assert options == {'assembias': True, 'modulate_with_cenocc': False}
    assert list(columns.items()) == [(key, (k, 1.0)) for k, key in
                                     enumerate(ZHENG07_ASSEMBIAS_KEYS + ('a', 'b'))]
    assert jacobian is None


@pytest.mark.parametrize('redshift', [0.0, 0.25])
def test_model_columns_leauthaud11(redshift):
    """The sixteen keys on the eleven device columns by the entries of `device_jacobian`: 1 and
    a - 1 for a relation's two, 1 for the other six; the extra keys behind them; the Jacobian
    block-diagonal with their identity."""
    model = Leauthaud11Model(redshift=redshift, modulate_with_cenocc=True)
    scale = 1.0 / (1.0 + redshift) - 1.0
    assert (scale == 0.0) == (redshift == 0.0)
    expect = {}
    for k in range(5):
        expect[LEAUTHAUD11_KEYS[2 * k]] = (k, 1.0)
        expect[LEAUTHAUD11_KEYS[2 * k + 1]] = (k, scale)
    for k in range(5, 11):
        expect[LEAUTHAUD11_KEYS[k + 5]] = (k, 1.0)
    for extra in ((), ('log_eta', 'alpha_s')):
        theta, options, columns, jacobian = _grad.model_columns(model, False, 'fisher', extra,
                                                                leauthaud11=True)
        assert np.array_equal(theta, model.device_theta()[np.newaxis])
        assert options == {'family': 'leauthaud11', 'modulate_with_cenocc': True}
        every = dict(expect, **{key: (11 + d, 1.0) for d, key in enumerate(extra)})
        assert list(columns.items()) == list(every.items())
        assert list(columns) == list(LEAUTHAUD11_KEYS + extra)
        block = np.zeros((11 + len(extra), 16 + len(extra)))
        block[:11, :16] = model.device_jacobian()
        block[11:, 16:] = np.eye(len(extra))
        assert np.array_equal(jacobian, block)
        # the columns are the Jacobian's non-zero pattern
        for j, (key, (k, factor)) in enumerate(columns.items()):
            assert jacobian[k, j] == factor
            assert np.count_nonzero(jacobian[:, j]) == (factor != 0.0)


def test_model_columns_refuses_what_the_parent_refused():
    class Other:
        pass

    plain, decorated, leauthaud = Zheng07Model(), decorated_model(), Leauthaud11Model()
    cases = [(plain, True, True, ValueError), (plain, True, False, ValueError),
             (decorated, False, True, NotImplementedError),
             (decorated, False, False, NotImplementedError),
             (leauthaud, False, False, NotImplementedError),   # a joint serves no Leauthaud11
             (leauthaud, True, True, ValueError), (leauthaud, True, False, ValueError),
             (Other(), False, True, NotImplementedError), (Other(), True, True, ValueError)]
    for model, assembias, leauthaud11, error in cases:
        with pytest.raises(error, match='the_call'):
            _grad.model_columns(model, assembias, 'the_call', leauthaud11=leauthaud11)


def test_keyed_keeps_the_bits_with_factor_one():
    values = np.array([np.inf, -np.inf, np.nan, -0.0, 5e-324, 1.0 / 3.0, -np.nan])
    columns = {str(k): (k, 1.0) for k in range(len(values))}
    got = np.array(list(_grad.keyed(values, columns).values()))
    assert np.array_equal(got.view(np.uint64), values.view(np.uint64))
    assert all(type(value) is float for value in _grad.keyed(values, columns).values())
    rows = np.stack([values, values[::-1]], axis=1)
    got = np.array(list(_grad.keyed(rows, columns).values()))
    assert np.array_equal(got.view(np.uint64), rows.view(np.uint64))
    # a factor scales its column
    assert _grad.keyed(np.array([2.0, 3.0]), {'a': (1, -0.5), 'b': (1, 0.0)}) == {'a': -1.5,
                                                                                  'b': 0.0}


# ---- Zheng07: the Fisher matrix is returned as it is ---------------------------------------------

def special(n_cols):
    """A Fisher matrix and a gradient row with inf, NaN and -0.0 among their entries."""
    fisher = np.arange(float(n_cols * n_cols)).reshape(1, n_cols, n_cols)
    fisher[0, 0, 0], fisher[0, 1, 0], fisher[0, 0, 1] = np.inf, np.nan, np.nan
    fisher[0, 2, 2], fisher[0, 3, 3], fisher[0, 1, 1] = -0.0, -np.inf, 0.0
    row = np.arange(float(n_cols))[np.newaxis].copy()
    row[0, :4] = np.inf, np.nan, -0.0, -np.inf
    return fisher, row


def same_words(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize('assembias', [False, True])
def test_zheng07_fisher_keeps_inf_and_nan(assembias):
    """With the batched method returning a matrix that holds inf, NaN and -0.0, the un-batched
    Zheng07 form of each class returns those words: no product with a Jacobian (inf * 0 = NaN)."""
    n_model = 7 if assembias else 5
    keys = ZHENG07_ASSEMBIAS_KEYS if assembias else ZHENG07_KEYS
    model = decorated_model() if assembias else Zheng07Model()
    seen = []

    def batched(n_cols, full):
        fisher, row = special(n_cols)
        ngal = np.array([2.5])

        def call(theta, *arguments, **options):
            seen.append((theta.shape, len(arguments), options))
            return (ngal, np.array([7.0]), row, row[:, ::-1], fisher) if full else \
                (ngal, row, fisher)
        return call, fisher, row

    table = synthetic.synthetic_table(3, 2, (5, ), 'auto', seed=1)
    halotab = halotab_of(table)
    halotab.fisher_batch, fisher, row = batched(n_model, False)
    ngal, dngal, got = halotab.fisher(model, np.eye(5), check_consistency=False,
                                      assembias=assembias)
    assert ngal == 2.5 and type(ngal) is float
    assert same_words(got, fisher[0]) and list(dngal) == list(keys)
    assert same_words(list(dngal.values()), row[0])
    assert seen[-1] == ((1, n_model), 1, {'n_gauss_prim': 10, 'modulate_with_cenocc': False,
                                          'assembias': assembias})
    assert halotab._device is None

    interp, x = make_interpolator((5, ))
    for d, key in enumerate(interp.keys):
        model.param_dict[key] = float(x[0, d])
    interp.fisher_batch, fisher, row = batched(n_model + 2, False)
    ngal, dngal, got = interp.fisher(model, np.eye(5), check_consistency=False,
                                     assembias=assembias)
    assert same_words(got, fisher[0]) and list(dngal) == list(keys) + list(interp.keys)
    assert same_words(list(dngal.values()), row[0])
    assert seen[-1][:2] == ((1, n_model), 2) and seen[-1][2]['extrapolate'] is False

    joint = JointLikelihood([halotab])
    joint.chi2_fisher_batch, fisher, row = batched(n_model, True)
    ngal, chi2, dngal, dchi2, got = joint.chi2_fisher(model, np.zeros(5), np.eye(5),
                                                      check_consistency=False,
                                                      assembias=assembias)
    assert (ngal, chi2) == (2.5, 7.0) and same_words(got, fisher[0])
    assert same_words(list(dngal.values()), row[0])
    assert same_words(list(dchi2.values()), row[0, ::-1]) and list(dchi2) == list(keys)
    assert seen[-1][:2] == ((1, n_model), 2)

    joint_interp = JointInterpolator([interp])
    joint_interp.chi2_fisher_batch, fisher, row = batched(n_model + 2, True)
    ngal, chi2, dngal, dchi2, got = joint_interp.chi2_fisher(
        model, np.zeros(5), np.eye(5), extrapolate=True, check_consistency=False,
        assembias=assembias)
    assert same_words(got, fisher[0]) and list(dngal) == list(keys) + list(interp.keys)
    assert same_words(list(dchi2.values()), row[0, ::-1])
    assert seen[-1][:2] == ((1, n_model), 3) and seen[-1][2]['extrapolate'] is True
    assert joint_interp._device is None and interp._device is None


def test_leauthaud11_fisher_is_carried_by_the_jacobian():
    """J^T F J with the block-diagonal J, the gradient by the columns' factors."""
    model = Leauthaud11Model(redshift=0.25)
    interp, x = make_interpolator((5, ))
    for d, key in enumerate(interp.keys):
        model.param_dict[key] = float(x[0, d])
    rng = np.random.default_rng(5)
    fisher, row = rng.normal(size=(1, 13, 13)), rng.normal(size=(1, 13))
    interp.fisher_batch = lambda theta, x, precision, **options: (np.ones(1), row, fisher)
    _, dngal, got = interp.fisher(model, np.eye(5), check_consistency=False)
    own = model.device_jacobian()
    jacobian = np.zeros((13, 18))
    jacobian[:11, :16], jacobian[11:, 16:] = own, np.eye(2)
    assert same_words(got, jacobian.T @ fisher[0] @ jacobian)
    assert list(dngal) == list(LEAUTHAUD11_KEYS) + list(interp.keys)
    np.testing.assert_array_equal(list(dngal.values()), row[0] @ jacobian)


# ---- the handle owners ---------------------------------------------------------------------------

def test_handle_destroys_once_with_its_symbol():
    class Lib:
        def __init__(self):
            self.destroyed = []

        def tc_thing_destroy(self, handle):
            self.destroyed.append(handle.value)

    lib = Lib()
    owner = _lib.Handle(lib, ctypes.c_void_p(77), 'tc_thing_destroy')
    assert owner.lib is lib and owner.handle.value == 77
    owner.__del__()
    owner.__del__()
    assert lib.destroyed == [77] and owner.handle is None
    # an owner whose construction failed before it had a handle, and a NULL handle
    _lib.Handle.__new__(_lib.Handle).__del__()
    _lib.Handle(lib, ctypes.c_void_p(), 'tc_thing_destroy').__del__()
    assert lib.destroyed == [77]
    from tabcorr_amd import interpolator, joint, tabcorr
    for owner_class in (tabcorr._DeviceTable, interpolator._DeviceInterpolator,
                        joint._DeviceJoint, joint._DeviceJointInterp):
        assert issubclass(owner_class, _lib.Handle)
        assert '__del__' not in vars(owner_class)


def test_joint_locks_are_one_class_over_an_ordered_list():
    from tabcorr_amd import joint

    class Table:
        def __init__(self):
            self.lock = threading.RLock()

    tables = [Table() for _ in range(3)]
    ordered = joint._DeviceJoint.ordered_locks(tables[::-1])
    assert ordered == joint._DeviceJoint.ordered_locks(tables)
    assert sorted(map(id, ordered)) == sorted(id(t.lock) for t in tables)
    from tabcorr_amd.interpolator import _HandleLocks
    members = [type('Member', (), {'lock': _HandleLocks(tables[:2])})(),
               type('Member', (), {'lock': _HandleLocks(tables[1:])})()]
    ordered = joint._DeviceJointInterp.ordered_locks(members)
    assert ordered == joint._DeviceJointInterp.ordered_locks(members[::-1])
    assert len(ordered) == 2 + 3 and {id(m.lock.own) for m in members} == set(map(id, ordered[:2]))
    locks = joint._Locks(ordered)
    with locks:
        assert all(lock._is_owned() for lock in ordered)
    assert not any(lock._is_owned() for lock in ordered)
