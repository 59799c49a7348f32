"""The occupation seam of a joint on the device (JointLikelihood.predict_occupation, predict_vjp,
chi2_occupation and chi2_grad_occupation; the tc_joint_predict_occupation_vjp_* and
tc_joint_chi2_occupation_grad_* entry points) against the composed NumPy reference of
joint_vjp_reference.py.  Needs an MI355X.

Allowance of a gradient element: |got - ref| <= 1e-10 (|ref| + scale), the scale the sum of the
tables' scales (vjp_reference); ngal and xi to 1e-10 relative; chi2 as test_gpu_vjp.check_chi2.
Every case prints its largest error in units of that allowance.  The shapes are those of
test_gpu_joint.py, the occupations those of test_gpu_vjp.py.
"""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_reference  # noqa: E402
import joint_vjp_reference  # noqa: E402
import vjp_reference  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    D, LDS_LIMIT, RTOL, check_still_serves, device_call, largest, same_bits)
from test_gpu_vjp import check_chi2, check_gradient, occupations_of  # noqa: E402
from util import assert_rel, load_golden, table_from_golden  # noqa: E402

pytestmark = pytest.mark.gpu

DRAW_COUNTS = [1, D + 1, 2 * D + 1]
N_MAX = max(DRAW_COUNTS)
KINDS = ['zheng07', 'random']

AUTO3, CROSS5 = ('auto', (3, )), ('cross', (5, ))
# name -> (n_prim, n_sec, parts), as test_gpu_joint.py: 18 bins; 36 bins (more than two row tiles,
# no multiple of 16); 32 bins (whole tiles); the order reversed; registers carried across two auto
# tables with a cross table between them; no auto table at all (P e needs rows of its own).
JOINTS = {
    'auto3-cross5-18': (9, 1, [AUTO3, CROSS5]),
    'auto3-cross5-36': (9, 2, [AUTO3, CROSS5]),
    'auto3-cross5-32': (16, 1, [AUTO3, CROSS5]),
    'cross5-auto3-36': (9, 2, [CROSS5, AUTO3]),
    'auto3-cross2-auto6-36': (9, 2, [AUTO3, ('cross', (2, )), ('auto', (6, ))]),
    'cross5-cross3-36': (9, 2, [CROSS5, ('cross', (3, ))]),
}
REAL = 'bolplanck'
NAMES = list(JOINTS)

_joints = {}
_occupations = {}
_references = {}


def make_halotab(table, **kwargs):
    from tabcorr_amd import TabCorr
    return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                               table['attrs'], **kwargs)


def make_joint(tables):
    from tabcorr_amd import JointLikelihood
    halotabs = [make_halotab(table) for table in tables]
    return halotabs, JointLikelihood(halotabs)


def get_joint(name):
    """(table dicts, TabCorr list, JointLikelihood), made once."""
    if name not in _joints:
        if name == REAL:
            tables = [table_from_golden(load_golden('bolplanck_wp')),
                      table_from_golden(load_golden('bolplanck_ds'))]
        else:
            n_prim, n_sec, parts = JOINTS[name]
            tables = joint_reference.make_tables(n_prim, n_sec, parts)
        _joints[name] = (tables, ) + make_joint(tables)
    return _joints[name]


def get_occupations(name, kind):
    key = (name, kind)
    if key not in _occupations:
        _occupations[key] = occupations_of(get_joint(name)[0][0], kind, N_MAX)
        _occupations[key].setflags(write=False)
    return _occupations[key]


def unit_rows(tables):
    """A cross row (the second of the first cross table) and an auto row (the last of the second
    auto table, of the only one otherwise) of the joint axis; None where there is no such table."""
    slices = joint_vjp_reference.slices_of(tables)
    modes = [table['attrs']['mode'] for table in tables]
    cross = [s for s, m in zip(slices, modes) if m == 'cross']
    auto = [s for s, m in zip(slices, modes) if m == 'auto']
    return (cross[0].start + 1 if cross else None, auto[-1].stop - 1 if auto else None)


def cotangents(name, which):
    """g (N_MAX, N) on the joint axis and g_ngal (N_MAX) or None: 'random', 'no_ngal', 'ngal'
    (g = 0, g_ngal = 1), 'unit_R' (the unit vector of row R alone)."""
    n = get_joint(name)[2].n_r_total
    rng = np.random.default_rng(17)
    g, g_ngal = rng.normal(size=(N_MAX, n)), rng.normal(size=N_MAX)
    if which == 'no_ngal':
        g_ngal = None
    elif which == 'ngal':
        g, g_ngal = np.zeros((N_MAX, n)), np.ones(N_MAX)
    elif which.startswith('unit_'):
        g, g_ngal = np.zeros((N_MAX, n)), None
        g[:, int(which[5:])] = 1.0
    return g, g_ngal


def usable(reference):
    """No draw is left out: every reference draw has galaxies and is finite."""
    return np.all(reference[0] > 0.0) and all(np.all(np.isfinite(a)) for a in reference)


def get_reference(name, kind, which):
    """Occupations, cotangents and the reference (ngal, xi, g_occupation, scale) of N_MAX draws,
    computed once and never modified: a batch of n draws is the first n."""
    key = (name, kind, which)
    if key not in _references:
        occupation = get_occupations(name, kind)
        g, g_ngal = cotangents(name, which)
        reference = joint_vjp_reference.vjp_batch(get_joint(name)[0], occupation, g, g_ngal)
        assert len(reference[0]) == N_MAX and usable(reference), key
        for array in (g, g_ngal) + reference:
            if array is not None:
                array.setflags(write=False)
        _references[key] = (occupation, g, g_ngal, reference)
    return _references[key]


def flat(xis, n):
    """The per-table results on one joint axis."""
    return np.concatenate([np.reshape(part, (n, -1)) for part in xis], axis=1)


def check_call(joint, occupation, g, g_ngal, reference, n, what, as_list):
    """predict_vjp of the first n draws against the reference, the cotangents as a list of
    per-table arrays or flat; predict_occupation returns the same bits."""
    g_xis = joint._split(g[:n], (n, )) if as_list else g[:n]
    ngal, xis, g_occupation = joint.predict_vjp(occupation[:n], g_xis,
                                                None if g_ngal is None else g_ngal[:n])
    assert ngal.shape == (n, ) and g_occupation.shape == occupation[:n].shape
    assert [xi.shape for xi in xis] == [(n, ) + tuple(h.tpcf_shape) for h in joint.tabcorr_list]
    assert_rel(ngal, reference[0][:n], RTOL, what + ' ngal')
    assert_rel(flat(xis, n), reference[1][:n], RTOL, what + ' xi')
    check_gradient(g_occupation, reference[2][:n], reference[3][:n], what)
    forward = joint.predict_occupation(occupation[:n])
    assert same_bits((forward[0], flat(forward[1], n)), (ngal, flat(xis, n)))
    return ngal, xis, g_occupation


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', NAMES)
def test_joint_vjp_matches_reference(name, kind):
    """Random cotangents with and without g_ngal at 1, 17 and 33 draws; at 17 draws g_ngal = 1
    alone (the bare n_h) and the unit vectors of a cross row and of an auto row of the second auto
    table (single rows of the Jacobian)."""
    tables, _, joint = get_joint(name)
    for which in ('random', 'no_ngal'):
        occupation, g, g_ngal, reference = get_reference(name, kind, which)
        for n in DRAW_COUNTS:
            what = '%s %s %s n=%d' % (name, kind, which, n)
            check_call(joint, occupation, g, g_ngal, reference, n, what, which == 'random')
    for which in ['ngal'] + ['unit_%d' % r for r in unit_rows(tables) if r is not None]:
        occupation, g, g_ngal, reference = get_reference(name, kind, which)
        what = '%s %s %s n=%d' % (name, kind, which, D + 1)
        got = check_call(joint, occupation, g, g_ngal, reference, D + 1, what, False)
        if which == 'ngal':
            assert_rel(got[2], np.broadcast_to(tables[0]['gal_type']['n_h'], got[2].shape), RTOL)
    # un-batched
    occupation, g, g_ngal, reference = get_reference(name, kind, 'random')
    full = joint.predict_vjp(occupation, g, g_ngal)
    one = joint.predict_vjp(occupation[2], [part[2] for part in joint._split(g, (N_MAX, ))],
                            g_ngal[2])
    assert np.ndim(one[0]) == 0 and one[0] == full[0][2] and np.array_equal(one[2], full[2][2])
    assert all(a.shape == tuple(h.tpcf_shape) and np.array_equal(a, b[2])
               for a, b, h in zip(one[1], full[1], joint.tabcorr_list))
    assert same_bits(joint.predict_vjp(occupation[2], g[2], g_ngal[2])[2:], one[2:])
    forward = joint.predict_occupation(occupation[2])
    assert forward[0] == one[0] and all(np.array_equal(a, b) for a, b in zip(forward[1], one[1]))


# ---- the likelihood form ------------------------------------------------------------------------

def operands(name, kind, symmetric):
    """A data vector near draw 3's joint vector and a precision matrix that couples the tables
    (in units of |xi| for the real pair)."""
    xi = get_reference(name, kind, 'no_ngal')[3][1][3]
    data, precision = joint_reference.coupled_data(xi, symmetric, name == REAL)
    first = get_joint(name)[2].slices[0].stop
    assert np.all(precision[:first, first:] != 0.0)
    return data, precision


def check_likelihood(joint, tables, occupation, data, precision, what):
    """chi2_grad_occupation at 1, 17 and 33 draws against the reference; chi2_occupation returns
    the bits of its (ngal, chi2)."""
    reference = joint_vjp_reference.chi2_grad_batch(tables, occupation, data, precision)
    assert usable(reference), what
    for n in DRAW_COUNTS:
        got = joint.chi2_grad_occupation(occupation[:n], data, precision)
        assert got[0].shape == got[1].shape == (n, ) and got[2].shape == occupation[:n].shape
        check_chi2(got, reference, data, precision, '%s n=%d' % (what, n))
        assert same_bits(joint.chi2_occupation(occupation[:n], data, precision), got[:2])
    return got


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('name', NAMES)
def test_joint_chi2_gradient_matches_reference(name, symmetric):
    """chi2 and dchi2 / dn of the joint data vector against a precision matrix whose off-diagonal
    blocks couple the tables; the non-symmetric one pins the P_sym convention."""
    tables, _, joint = get_joint(name)
    for kind in KINDS:
        occupation = get_occupations(name, kind)
        data, precision = operands(name, kind, symmetric)
        got = check_likelihood(joint, tables, occupation, data, precision,
                               'chi2 %s %s %s' % (name, kind, symmetric))
    # data as a list of per-table arrays; un-batched
    parts = [data[part] for part in joint.slices]
    assert same_bits(joint.chi2_grad_occupation(occupation, parts, precision), got)
    one = joint.chi2_grad_occupation(occupation[2], data, precision)
    assert np.ndim(one[0]) == 0 and np.ndim(one[1]) == 0
    assert one[0] == got[0][2] and one[1] == got[1][2] and np.array_equal(one[2], got[2][2])
    alone = joint.chi2_occupation(occupation[2], data, precision)
    assert np.ndim(alone[1]) == 0 and alone == (one[0], one[1])


def test_real_pair():
    """w_p + DeltaSigma of tests/golden (60 bins, N = 38, twelve orders of magnitude apart), the
    precision matrix in units of |xi|."""
    tables, _, joint = get_joint(REAL)
    for which in ('random', 'no_ngal'):
        occupation, g, g_ngal, reference = get_reference(REAL, 'zheng07', which)
        check_call(joint, occupation, g, g_ngal, reference, D + 1, REAL + ' ' + which,
                   which == 'random')
    data, precision = operands(REAL, 'zheng07', False)
    check_likelihood(joint, tables, get_occupations(REAL, 'zheng07'), data, precision,
                     'chi2 ' + REAL)


# ---- bits ---------------------------------------------------------------------------------------

SINGLE = [((9, 2, (3, )), 'auto'), ((16, 1, (5, )), 'auto'), ((9, 2, (5, )), 'cross'),
          ((33, 2, (3, )), 'cross')]


@pytest.mark.parametrize('shape,mode', SINGLE,
                         ids=['%s-%dx%d' % (m, s[0], s[1]) for s, m in SINGLE])
def test_joint_of_one_table_has_the_bits_of_the_table(shape, mode):
    """The pieces are those of the table kernels and an absent term is an exact zero: a joint of
    ONE table returns the bits of that table's own predict_vjp / chi2_grad_occupation (mode cross,
    132 bins: three slabs of vjp_cross_kernel against the one fma chain)."""
    from tabcorr_amd import JointLikelihood
    table = synthetic.synthetic_table(shape[0], shape[1], shape[2], mode, seed=3)
    halotab = make_halotab(table)
    joint = JointLikelihood([halotab])
    n_r = int(np.prod(shape[2]))
    rng = np.random.default_rng(17)
    g, g_ngal = rng.normal(size=(N_MAX, n_r)), rng.normal(size=N_MAX)
    for kind in KINDS:
        occupation = occupations_of(table, kind, N_MAX)
        for weights in (g_ngal, None):
            own = halotab.predict_vjp(occupation, g, weights)
            got = joint.predict_vjp(occupation, [g], weights)
            assert np.all(np.isfinite(own[2]))
            assert same_bits((got[0], got[1][0], got[2]), own)
        data, precision = joint_reference.coupled_data(own[1][3], False)
        own = halotab.chi2_grad_occupation(occupation, data, precision)
        assert np.all(np.isfinite(own[2]))
        assert same_bits(joint.chi2_grad_occupation(occupation, data, precision), own)


@pytest.mark.parametrize('mode', ['auto', 'cross'])
def test_same_mode_joint_matches_the_stacked_table(mode):
    """A joint of same-mode tables against the table kernel on the one table whose matrices are
    concatenated along r: 1e-10 (|value| + scale)."""
    tables = joint_reference.make_tables(9, 2, [(mode, (3, )), (mode, (6, ))])
    _, joint = make_joint(tables)
    one = joint_vjp_reference.stacked(tables)
    halotab = make_halotab(one)
    rng = np.random.default_rng(17)
    g, g_ngal = rng.normal(size=(N_MAX, 9)), rng.normal(size=N_MAX)
    for kind in KINDS:
        occupation = occupations_of(tables[0], kind, N_MAX)
        scale = vjp_reference.vjp_batch(one, occupation, g, g_ngal)[3]
        expect = halotab.predict_vjp(occupation, g, g_ngal)
        got = joint.predict_vjp(occupation, g, g_ngal)
        assert_rel(got[0], expect[0], RTOL)
        assert_rel(flat(got[1], N_MAX), expect[1], RTOL)
        check_gradient(got[2], expect[2], scale, 'stacked %s %s' % (mode, kind))


def device_vjp(joint, occupation, g=None, g_ngal=None, data=None, precision=None, flags=0,
               backward=True):
    """The `_device` entries on fresh device arrays: the prediction form (g, or forward only) or
    the likelihood form (data and precision, host arrays there too)."""
    from tabcorr_amd import _lib
    device = joint.to_device()
    n, total = len(occupation), joint.n_r_total
    view = device if backward else WithoutLastOutput(device)
    if data is not None:
        data, precision = _lib.contiguous(np.ravel(data)), _lib.contiguous(precision)
        return device_call(view, 'tc_joint_chi2_occupation_grad_batch_device',
                           [occupation, n, flags, _lib.as_double_p(data),
                            _lib.as_double_p(precision)],
                           [n, n] + [occupation.shape] * backward,
                           synchronize='tc_joint_synchronize')
    return device_call(view, 'tc_joint_predict_occupation_vjp_batch_device',
                       [occupation, n, flags, g_ngal, g],
                       [n, (n, total)] + [occupation.shape] * backward,
                       synchronize='tc_joint_synchronize')


class WithoutLastOutput:
    """device_call's view of a joint whose entries are given NULL for the gradient behind the
    outputs that device_call allocates: the forward-only forms."""

    def __init__(self, device):
        self.lock, self.handle, self.lib = device.lock, device.handle, self
        self.library = device.lib

    def __getattr__(self, name):
        entry = getattr(self.library, name)
        if name.endswith('_batch_device'):
            return lambda handle, *passed: entry(handle, *passed, None)
        return entry


@pytest.mark.parametrize('name', ['auto3-cross5-36', 'auto3-cross2-auto6-36', 'cross5-cross3-36'])
def test_batch_invariance(name):
    """A draw's results are the same bits alone, in 17 draws (at two different columns of a
    workgroup) and in 33 draws, through the host and the device entries, with and without the
    gradient.  Draw 5 has an all-zero occupation: its own results are NaN, none of its
    neighbours' are."""
    _, _, joint = get_joint(name)
    occupation = np.array(get_occupations(name, 'random'))
    occupation[5] = 0.0
    g, g_ngal = cotangents(name, 'random')
    data, precision = operands(name, 'random', False)
    others = np.arange(N_MAX) != 5

    def predict(rows, device=False):
        if device:
            return device_vjp(joint, occupation[rows], g[rows], g_ngal[rows])
        ngal, xis, g_occupation = joint.predict_vjp(occupation[rows], g[rows], g_ngal[rows])
        return ngal, flat(xis, len(ngal)), g_occupation

    def likelihood(rows, device=False):
        if device:
            return device_vjp(joint, occupation[rows], data=data, precision=precision)
        return joint.chi2_grad_occupation(occupation[rows], data, precision)

    for call in (predict, likelihood):
        full = call(slice(0, N_MAX))
        assert full[0][5] == 0.0 and np.all(np.isnan(full[1][5])) and np.all(np.isnan(full[2][5]))
        assert all(np.all(np.isfinite(a[others])) for a in full)
        for rows in (slice(0, 1), slice(0, D + 1), slice(3, D + 4), slice(D, D + 1),
                     slice(N_MAX - 1, N_MAX), slice(5, 6), slice(6, 7)):
            assert same_bits(call(rows), [a[rows] for a in full]), (call.__name__, rows)
        for n in DRAW_COUNTS:
            assert same_bits(call(slice(0, n), device=True), [a[:n] for a in full])
    # the forward-only forms and g_ngal = NULL through the device entries
    full = predict(slice(0, N_MAX))
    assert same_bits(device_vjp(joint, occupation, backward=False), full[:2])
    assert same_bits(device_vjp(joint, occupation, data=data, precision=precision,
                                backward=False), likelihood(slice(0, N_MAX))[:2])
    without = joint.predict_vjp(occupation, g)
    assert same_bits(device_vjp(joint, occupation, g),
                     (without[0], flat(without[1], N_MAX), without[2]))


# ---- what is refused ----------------------------------------------------------------------------

def joint_vjp_lds(n_bins, n_r_total, n_r_auto):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    _lib.check(_lib.load().tc_debug_joint_vjp_lds_bytes(n_bins, n_r_total, n_r_auto,
                                                        ctypes.byref(got)))
    return got.value


def check_joint_still_serves(name='auto3-cross5-36'):
    """A joint serves the seam and the forward likelihood (JointLikelihood.chi2_batch)."""
    _, _, joint = get_joint(name)
    occupation, g, g_ngal, reference = get_reference(name, 'random', 'random')
    check_call(joint, occupation, g, g_ngal, reference, D + 1, 'still serves', False)
    n = joint.n_r_total
    ngal, chi2 = joint.chi2_batch(synthetic.zheng07_draws(5, seed=2), np.ones(n), np.eye(n))
    assert np.all(np.isfinite(ngal)) and np.all(np.isfinite(chi2))


def test_lds_limit():
    """N = 2, [auto (1,), cross (1,)], n_sec = 1: the joint with the most bins that the budget
    admits runs with (nearly) the whole LDS of a CU and matches the reference in all four calls;
    one more primary bin is refused by all four, naming LDS, before anything is launched: its
    tables go on serving predict_batch, and a joint the seam and chi2_batch."""
    parts = [('auto', (1, )), ('cross', (1, ))]
    n_prim = largest(lambda n: joint_vjp_lds(2 * n, 2, 1) <= LDS_LIMIT)
    tables = joint_reference.make_tables(n_prim, 1, parts)
    _, joint = make_joint(tables)
    n = D + 1
    occupation = occupations_of(tables[0], 'random', n)
    rng = np.random.default_rng(17)
    g, g_ngal = rng.normal(size=(n, 2)), rng.normal(size=n)
    reference = joint_vjp_reference.vjp_batch(tables, occupation, g, g_ngal)
    assert usable(reference)
    what = 'LDS limit, %d bins' % (2 * n_prim)
    check_call(joint, occupation, g, g_ngal, reference, n, what, True)
    data, precision = joint_reference.coupled_data(reference[1][3], False)
    assert precision[0, 1] != 0.0 and precision[1, 0] != 0.0
    got = joint.chi2_grad_occupation(occupation, data, precision)
    check_chi2(got, joint_vjp_reference.chi2_grad_batch(tables, occupation, data, precision),
               data, precision, what + ' chi2')
    assert same_bits(joint.chi2_occupation(occupation, data, precision), got[:2])

    tables = joint_reference.make_tables(n_prim + 1, 1, parts)
    halotabs, joint = make_joint(tables)
    occupation = np.ones((3, 2 * n_prim + 2))
    for call in (lambda: joint.predict_occupation(occupation),
                 lambda: joint.predict_vjp(occupation, np.ones((3, 2))),
                 lambda: joint.chi2_occupation(occupation, np.ones(2), np.eye(2)),
                 lambda: joint.chi2_grad_occupation(occupation, np.ones(2), np.eye(2))):
        with pytest.raises(NotImplementedError, match='LDS'):
            call()
    for table, halotab in zip(tables, halotabs):
        check_still_serves(halotab, table)
    check_joint_still_serves()


def test_invalid_requests_leave_the_joint_usable():
    """flags != 0 and exactly one of g_xi / g_occupation NULL are TC_ERR_INVALID; n_draws = 0 is
    served (nothing to do), a negative count is not."""
    from tabcorr_amd import _lib
    name = 'auto3-cross5-36'
    _, _, joint = get_joint(name)
    device = joint.to_device()
    lib = device.lib
    occupation = np.array(get_occupations(name, 'random')[:5])
    n = joint.n_r_total
    g = np.ones((5, n))
    p = _lib.as_double_p
    out = [np.empty(5), np.empty((5, n)), np.empty_like(occupation)]
    data, precision = np.ones(n), np.eye(n)

    def vjp(flags=0, n_draws=5, g_xi=g, g_occupation=out[2]):
        with device.lock:
            return lib.tc_joint_predict_occupation_vjp_batch(
                device.handle, p(occupation), n_draws, flags, None,
                None if g_xi is None else p(g_xi), p(out[0]), p(out[1]),
                None if g_occupation is None else p(g_occupation))

    def chi2(flags=0, n_draws=5):
        with device.lock:
            return lib.tc_joint_chi2_occupation_grad_batch(
                device.handle, p(occupation), n_draws, flags, p(data), p(precision), p(out[0]),
                p(np.empty(5)), p(out[2]))

    for flags in (_lib.FLAG_SEPARATE_GAL_TYPE, _lib.FLAG_ASSEMBIAS, _lib.FLAG_LEAUTHAUD11):
        for status in (vjp(flags), chi2(flags)):
            assert status == _lib.TC_ERR_INVALID
            with pytest.raises(ValueError, match='flags'):
                _lib.check(status)
    for status in (vjp(g_xi=None), vjp(g_occupation=None)):
        assert status == _lib.TC_ERR_INVALID
        with pytest.raises(ValueError, match='g_xi'):
            _lib.check(status)
    assert vjp(n_draws=-1) == _lib.TC_ERR_INVALID and chi2(n_draws=-1) == _lib.TC_ERR_INVALID
    assert vjp(n_draws=0) == _lib.TC_OK and chi2(n_draws=0) == _lib.TC_OK
    assert vjp() == _lib.TC_OK and vjp(g_xi=None, g_occupation=None) == _lib.TC_OK
    check_joint_still_serves(name)
