"""The occupation seam of an interpolator on the device (Interpolator.predict_occupation,
predict_vjp, chi2_occupation and chi2_grad_occupation; the tc_interp_predict_occupation_vjp_* and
tc_interp_chi2_occupation_grad_* entry points) against the NumPy reference of
interp_vjp_reference.py.  Needs an MI355X.

Allowance of a gradient element: |got - ref| <= 1e-10 (|ref| + scale) with the reference's scale of
the cancelling terms; ngal, xi and chi2 to 1e-10 relative.  Every case prints its largest error in
units of that allowance.  A batch of n draws is the first n of the 35 of its case, and its results
are the bits of those rows of the 35-draw call.
"""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interp_grad_reference  # noqa: E402
import interp_vjp_reference as reference  # noqa: E402
import leauthaud11_grad_reference as leauthaud11  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    D, LDS_LIMIT, RTOL, check_refused, check_still_serves, chi2_data, device_call, largest,
    same_bits)
from test_gpu_vjp import check_gradient, decorated_draws  # noqa: E402
from util import REPO, assert_rel  # noqa: E402

pytestmark = pytest.mark.gpu

DRAW_COUNTS = [1, D + 1, 2 * D + 3]
N_MAX = max(DRAW_COUNTS)
KINDS = ['zheng07', 'decorated', 'random']

# (n_prim, n_sec, tpcf_shape, mode).  Mode auto: 18 bins (a padded row tile and a padded step of
# four columns), 32 bins (whole tiles, two secondary bins), a shaped tpcf.  Mode cross: 70 bins (two
# slabs, the second partial) and 8 bins.
AUTO_TABLES = [(9, 1, (3, ), 'auto'), (8, 2, (19, ), 'auto'), (5, 1, (2, 3), 'auto')]
CROSS_TABLES = [(35, 1, (13, ), 'cross'), (4, 1, (3, ), 'cross')]
TABLES = AUTO_TABLES + CROSS_TABLES
GRIDS = [(4, ), (4, 5)]

_cases = {}
_references = {}


def table_id(table):
    return '%s-%dx%d-r%s' % (table[3], table[0], table[1], 'x'.join(map(str, table[2])))


def make_tables(table, grid, classes):
    """Tables and points of a synthetic grid.  classes: 'one' (a shared gal_type), 'two' (every
    other table in list order has another n_h: two classes interleaved, so that the walk order
    differs from the list order), 'own' (every table its own n_h: C = K)."""
    tables, keys, points = synthetic.synthetic_interpolator(grid, table[0], table[1], table[2],
                                                            table[3], seed=3)
    for k, one in enumerate(tables):
        factor = {'one': 1.0, 'two': 1.0 + 0.2 * (k % 2), 'own': 1.0 + 0.03 * k}[classes]
        if factor != 1.0:
            one['gal_type'] = one['gal_type'].copy()
            one['gal_type']['n_h'] *= factor
    return tables, keys, points


def make_interpolator(tables, keys, points, **kwargs):
    from tabcorr_amd import Interpolator, TabCorr
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'],
                                    **kwargs) for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)})


def make_x(points, n, kind, seed=5):
    """(n, D) grid parameters: 'inside' uniform over the grid; 'node' on grid nodes (table k % K
    for draw k); 'edge' the last knot of the first axis; 'outside' beyond the grid, below on even
    draws and above on odd ones."""
    rng = np.random.default_rng(seed)
    low, high = points.min(axis=0), points.max(axis=0)
    x = rng.uniform(low, high, size=(n, points.shape[1]))
    if kind == 'node':
        x = points[np.arange(n) % len(points)].copy()
    elif kind == 'edge':
        x[:, 0] = high[0]
    elif kind == 'outside':
        span = high - low
        x[0::2] = low - rng.uniform(0.05, 0.3, size=x[0::2].shape) * span
        x[1::2] = high + rng.uniform(0.05, 0.3, size=x[1::2].shape) * span
    else:
        assert kind == 'inside'
    return x


def class_occupations(walk, kind, n_draws=N_MAX, theta_of=None):
    """(n_draws, C, n_bins) occupations, drawn independently per class, every class of every draw
    with galaxies: from the oracle for plain or decorated Zheng07 draws (per class the first seed
    that leaves no draw empty), or random positive numbers of which about a quarter, never all, are
    exactly zero."""
    n_bins = len(walk.tables[0]['gal_type'])
    rows = []
    for v, k in enumerate(walk.class_tables):
        table = walk.tables[k]
        if kind == 'random':
            rng = np.random.default_rng([n_bins, v])
            occupation = rng.uniform(0.1, 2.0, size=(n_draws, n_bins))
            zero = rng.uniform(size=occupation.shape) < 0.25
            zero[np.arange(n_draws), rng.integers(n_bins, size=n_draws)] = False
            occupation[zero] = 0.0
        else:
            for seed in range(5 + 20 * v, 25 + 20 * v):
                theta = decorated_draws(n_draws, seed) if theta_of is None else theta_of(
                    n_draws, seed)
                occupation = np.array([oracle.mean_occupation(table, oracle.Zheng07(
                    t[:5], assembias=t[5:] if kind == 'decorated' else None)) for t in theta])
                if np.all(occupation @ table['gal_type']['n_h'] > 0.0):
                    break
            else:
                raise AssertionError('no seed gives draws with galaxies')
        rows.append(occupation)
    return np.ascontiguousarray(np.stack(rows, axis=1))


def get_case(table, grid, classes='two', x_kind='inside', n=N_MAX):
    """Interpolator, tables, the reference's walk and the x of the case's n draws, made once per
    combination and never modified."""
    key = (table, grid, classes, x_kind, n)
    if key not in _cases:
        tables, keys, points = make_tables(table, grid, classes)
        setup = oracle.interpolator_setup(tables, points)
        walk = reference.Walk(tables, setup, points)
        n_classes = {'one': 1, 'two': 2, 'own': len(tables)}[classes]
        assert len(walk.class_tables) == n_classes
        x = make_x(points, n, x_kind)
        x.setflags(write=False)
        _cases[key] = {'key': key, 'interp': make_interpolator(tables, keys, points),
                       'tables': tables, 'points': points, 'setup': setup, 'walk': walk, 'x': x,
                       'n': n,
                       'shape': table[2], 'n_r': int(np.prod(table[2])),
                       'extrapolate': x_kind == 'outside', 'occupations': {}}
    return _cases[key]


def get_occupations(case, kind):
    if kind not in case['occupations']:
        case['occupations'][kind] = class_occupations(case['walk'], kind, case['n'])
        case['occupations'][kind].setflags(write=False)
    return case['occupations'][kind]


def cotangents(n_r, which, n_draws=N_MAX):
    """g (n_draws, n_r) and g_ngal (n_draws) or None: 'random'; 'no_ngal'; 'unit_R': the unit
    vector of r bin R alone; 'ngal': g = 0 and g_ngal = 1."""
    rng = np.random.default_rng(17)
    g, g_ngal = rng.normal(size=(n_draws, n_r)), rng.normal(size=n_draws)
    if which == 'no_ngal':
        g_ngal = None
    elif which == 'ngal':
        g, g_ngal = np.zeros((n_draws, n_r)), np.ones(n_draws)
    elif which.startswith('unit_'):
        g, g_ngal = np.zeros((n_draws, n_r)), None
        g[:, int(which[5:])] = 1.0
    return g, g_ngal


def get_reference(case, kind, which):
    """Occupations, cotangents and the reference of the case's draws, computed once and never
    modified: a batch of n draws is the first n."""
    key = (case['key'], kind, which)
    if key not in _references:
        occupation = get_occupations(case, kind)
        g, g_ngal = cotangents(case['n_r'], which, case['n'])
        expect = reference.batch(reference.vjp, case['walk'], occupation, case['x'], g, g_ngal)
        assert reference.usable(expect), key
        for array in [g, g_ngal] + list(expect.values()):
            if array is not None:
                array.setflags(write=False)
        _references[key] = {'occupation': occupation, 'g': g, 'g_ngal': g_ngal, 'expect': expect,
                            'full': None}
    return _references[key]


def check_call(case, kind, which, n, what):
    """predict_vjp of the first n draws against the reference and against the rows of the call
    with all the case's draws (bits); predict_occupation returns the same bits."""
    interp, ref = case['interp'], get_reference(case, kind, which)
    occupation, x, expect = ref['occupation'], case['x'], ref['expect']
    g = ref['g'].reshape((case['n'], ) + case['shape'])
    g_ngal = ref['g_ngal']

    def call(count):
        return interp.predict_vjp(occupation[:count], x[:count], g[:count],
                                  None if g_ngal is None else g_ngal[:count],
                                  extrapolate=case['extrapolate'])

    if ref['full'] is None:
        ref['full'] = call(case['n'])
    got = call(n)
    ngal, xi, g_occupation, g_x = got
    assert ngal.shape == (n, ) and xi.shape == (n, ) + case['shape']
    assert g_occupation.shape == occupation[:n].shape and g_x.shape == x[:n].shape
    assert_rel(ngal, expect['ngal'][:n], RTOL, what + ' ngal')
    assert_rel(xi.reshape(n, -1), expect['xi'][:n], RTOL, what + ' xi')
    check_gradient(g_occupation, expect['g_occupation'][:n], expect['g_occupation_scale'][:n],
                   what + ' g_occupation')
    check_gradient(g_x, expect['g_x'][:n], expect['g_x_scale'][:n], what + ' g_x')
    assert same_bits(got, [a[:n] for a in ref['full']]), what + ': the rows of the 35-draw call'
    forward = interp.predict_occupation(occupation[:n], x[:n], extrapolate=case['extrapolate'])
    assert same_bits(forward, got[:2]), what + ': forward only'
    return got


# ---- the prediction form -------------------------------------------------------------------------

@pytest.mark.parametrize('grid', GRIDS, ids=['4', '4x5'])
@pytest.mark.parametrize('table', TABLES, ids=table_id)
def test_vjp_matches_reference(table, grid):
    """Two interleaved classes, x inside the grid.  Random cotangents with and without g_ngal at
    1, 17 and 35 draws for the three kinds of occupations; at 17 draws g_ngal = 1 alone and the
    unit vectors of the first and the last r bin (single rows of the Jacobian)."""
    case = get_case(table, grid)
    name = '%s grid %s' % (table_id(table), 'x'.join(map(str, grid)))
    for kind in KINDS:
        for which in ('random', 'no_ngal'):
            for n in DRAW_COUNTS:
                check_call(case, kind, which, n, '%s %s %s n=%d' % (name, kind, which, n))
    for which in sorted({'unit_0', 'unit_%d' % (case['n_r'] - 1), 'ngal'}):
        got = check_call(case, 'zheng07', which, D + 1, '%s %s n=%d' % (name, which, D + 1))
        if which == 'ngal':
            # dngal/docc[v] = class_weights[:, v] n_h,v, as `class_weights` documents
            weights = case['interp'].class_weights(case['x'][:D + 1])
            walk = case['walk']
            for v, k in enumerate(walk.class_tables):
                n_h = walk.tables[k]['gal_type']['n_h']
                expect = weights[:, v, np.newaxis] * n_h
                scale = get_reference(case, 'zheng07', which)['expect']['g_occupation_scale']
                assert np.all(np.abs(got[2][:, v] - expect) <=
                              RTOL * (np.abs(expect) + scale[:D + 1, v]))


@pytest.mark.parametrize('classes', ['one', 'own'])
@pytest.mark.parametrize('table', [AUTO_TABLES[0], CROSS_TABLES[0]], ids=table_id)
def test_classes_of_halo_tables(table, classes):
    """One class (the occupation may then be (n, n_bins)) and C = K = 20 on the 4 x 5 grid."""
    case = get_case(table, (4, 5), classes=classes)
    interp = case['interp']
    assert len(interp.class_tables) == {'one': 1, 'own': 20}[classes]
    assert np.array_equal(interp.table_class, case['walk'].table_class)
    for kind in ('zheng07', 'random'):
        got = check_call(case, kind, 'random', D + 1, '%s classes=%s %s' % (
            table_id(table), classes, kind))
    if classes == 'one':
        ref = get_reference(case, 'random', 'random')
        n = D + 1
        flat = interp.predict_vjp(ref['occupation'][:n, 0], case['x'][:n],
                                  ref['g'][:n].reshape((n, ) + case['shape']), ref['g_ngal'][:n])
        assert flat[2].shape == (n, 1, ref['occupation'].shape[2]) and same_bits(flat, got)


@pytest.mark.parametrize('x_kind', ['node', 'edge', 'outside'])
@pytest.mark.parametrize('table', [AUTO_TABLES[0], CROSS_TABLES[0]], ids=table_id)
def test_positions_of_x(table, x_kind):
    """Exactly on a grid node, on the right edge, outside the grid on both sides with
    extrapolate=True (without it: ValueError)."""
    case = get_case(table, (4, 5), x_kind=x_kind)
    interp, walk = case['interp'], case['walk']
    n = 2 * D + 3
    got = check_call(case, 'random', 'random', n, '%s x=%s' % (table_id(table), x_kind))
    ref = get_reference(case, 'random', 'random')
    if x_kind == 'outside':
        xp = case['setup']['xp']
        assert all(np.all((case['x'][:, d] < xp[d][0]) | (case['x'][:, d] > xp[d][-1]))
                   for d in range(2))
        with pytest.raises(ValueError, match='extrapolation'):
            interp.predict_vjp(ref['occupation'], case['x'],
                               ref['g'].reshape((N_MAX, ) + case['shape']))
        with pytest.raises(ValueError, match='extrapolation'):
            interp.predict_occupation(ref['occupation'], case['x'])
    if x_kind == 'node':
        # the node's class has the gradient of that table's own predict_vjp, the other is zero
        scale = ref['expect']['g_occupation_scale']
        for d in range(0, n, 7):
            k = d % len(walk.tables)
            v = walk.table_class[k]
            own = interp.tabcorr_list[k].predict_vjp(
                ref['occupation'][d, v], ref['g'][d].reshape(case['shape']), ref['g_ngal'][d])
            assert np.all(np.abs(got[2][d, v] - own[2]) <= RTOL * (np.abs(own[2]) + scale[d, v]))
            assert np.all(np.abs(got[2][d, 1 - v]) <= RTOL * scale[d, 1 - v])
            assert_rel(got[0][d], own[0], RTOL)
            assert_rel(got[1][d], own[1], RTOL)


# ---- the likelihood form -------------------------------------------------------------------------

def check_likelihood(case, kind, data, precision, counts, what):
    """chi2_grad_occupation against the reference and the rows of the 35-draw call (bits);
    chi2_occupation returns the bits of its (ngal, chi2)."""
    interp = case['interp']
    occupation, x = get_occupations(case, kind), case['x']
    expect = reference.batch(reference.chi2_grad, case['walk'], occupation, x, data=data,
                             precision=precision)
    assert reference.usable(expect), what

    def call(count, gradient=True):
        function = interp.chi2_grad_occupation if gradient else interp.chi2_occupation
        return function(occupation[:count], x[:count], data, precision,
                        extrapolate=case['extrapolate'])

    full = call(case['n'])
    for n in counts:
        got = call(n)
        ngal, chi2, dchi2_docc, dchi2_dx, dngal_dx = got
        assert ngal.shape == chi2.shape == (n, ) and dchi2_docc.shape == occupation[:n].shape
        assert dchi2_dx.shape == dngal_dx.shape == x[:n].shape
        label = '%s n=%d' % (what, n)
        assert_rel(ngal, expect['ngal'][:n], RTOL, label + ' ngal')
        print('%s: max |chi2 - reference| / (1e-10 |reference|) = %.3g' % (
            label, np.max(np.abs(chi2 - expect['chi2'][:n]) / (RTOL * np.abs(expect['chi2'][:n])))))
        assert_rel(chi2, expect['chi2'][:n], RTOL, label + ' chi2')
        check_gradient(dchi2_docc, expect['g_occupation'][:n], expect['g_occupation_scale'][:n],
                       label + ' dchi2_docc')
        check_gradient(dchi2_dx, expect['g_x'][:n], expect['g_x_scale'][:n], label + ' dchi2_dx')
        check_gradient(dngal_dx, expect['dngal_dx'][:n], expect['dngal_dx_scale'][:n],
                       label + ' dngal_dx')
        assert same_bits(got, [a[:n] for a in full]), label + ': the rows of the 35-draw call'
        assert same_bits(call(n, gradient=False), got[:2]), label + ': forward only'
    return full


LIKELIHOOD_CASES = [(AUTO_TABLES[0], (4, 5)), (AUTO_TABLES[1], (4, )), (AUTO_TABLES[2], (4, )),
                    (CROSS_TABLES[0], (4, 5)), (CROSS_TABLES[1], (4, ))]


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('table,grid', LIKELIHOOD_CASES,
                         ids=[table_id(t) + '-' + 'x'.join(map(str, g))
                              for t, g in LIKELIHOOD_CASES])
def test_chi2_gradient_matches_reference(table, grid, symmetric):
    """chi2, dchi2/docc, dchi2/dx and dngal/dx at 1, 17 and 35 draws for random occupations and at
    35 draws for the two model kinds; the non-symmetric precision pins the P_sym convention."""
    case = get_case(table, grid)
    xi = get_reference(case, 'random', 'no_ngal')['expect']['xi'][3]
    data, precision = chi2_data(xi.reshape(case['shape']), symmetric)
    what = 'chi2 %s %s' % (table_id(table), 'spd' if symmetric else 'nonsymmetric')
    check_likelihood(case, 'random', data, precision, DRAW_COUNTS, what + ' random')
    for kind in ('zheng07', 'decorated'):
        check_likelihood(case, kind, data, precision, [N_MAX], what + ' ' + kind)


# ---- the reference's fixture ---------------------------------------------------------------------

def test_abacus_summit_fixture():
    """tests/golden/ds_efficient.hdf5: four mode-cross tables of 1104 bins (18 slabs, the last
    partial), 17 draws, both forms."""
    from tabcorr_amd import Interpolator
    interp = Interpolator.read(os.path.join(REPO, 'tests', 'golden', 'ds_efficient.hdf5'))
    tables = [{'gal_type': h.gal_type.as_array(),
               'tpcf_matrix': np.asarray(h.tpcf_matrix, dtype=np.float64),
               'tpcf_shape': tuple(h.tpcf_shape), 'attrs': dict(h.attrs)}
              for h in interp.tabcorr_list]
    assert len(tables) == 4 and len(tables[0]['gal_type']) == 1104
    assert tables[0]['attrs']['mode'] == 'cross'
    setup = oracle.interpolator_setup(tables, interp.points)
    walk = reference.Walk(tables, setup, interp.points)
    assert np.array_equal(interp.table_class, walk.table_class)
    n = D + 1
    rng = np.random.default_rng(5)

    def theta_of(n_draws, seed):
        theta = synthetic.zheng07_draws(n_draws, seed=seed)
        theta[:, 0] = rng.uniform(12.5, 13.3, n_draws)
        theta[:, 3] = rng.uniform(13.6, 14.4, n_draws)
        return theta

    occupation = class_occupations(walk, 'zheng07', n, theta_of)
    x = make_x(interp.points, n, 'inside')
    shape = tuple(tables[0]['tpcf_shape'])
    n_r = int(np.prod(shape))
    case = {'key': 'ds_efficient', 'interp': interp, 'walk': walk, 'x': x, 'shape': shape, 'n': n,
            'n_r': n_r, 'extrapolate': False, 'occupations': {'zheng07': occupation}}
    g, g_ngal = cotangents(n_r, 'random', n)
    expect = reference.batch(reference.vjp, walk, occupation, x, g, g_ngal)
    assert reference.usable(expect)
    got = interp.predict_vjp(occupation, x, g.reshape((n, ) + shape), g_ngal)
    assert_rel(got[0], expect['ngal'], RTOL, 'fixture ngal')
    assert_rel(got[1].reshape(n, -1), expect['xi'], RTOL, 'fixture xi')
    check_gradient(got[2], expect['g_occupation'], expect['g_occupation_scale'],
                   'fixture g_occupation')
    check_gradient(got[3], expect['g_x'], expect['g_x_scale'], 'fixture g_x')
    assert same_bits(interp.predict_occupation(occupation, x), got[:2])
    # the precision matrix in units of |xi|
    data = expect['xi'][3] * (1.0 + 0.05 * rng.normal(size=n_r))
    size = np.abs(data)
    precision = (np.diag(rng.uniform(1.0, 2.0, size=n_r)) +
                 0.01 * rng.normal(size=(n_r, n_r))) / np.outer(size, size)
    check_likelihood(case, 'zheng07', data.reshape(shape), precision, [n], 'fixture chi2')


# ---- the device entries --------------------------------------------------------------------------

class WithoutLastOutputs:
    """device_call's view of an interpolator whose entries are given NULL for the `count` outputs
    behind those that device_call allocates: the forward-only forms."""

    def __init__(self, device, count):
        self.lock, self.handle, self.lib = device.lock, device.handle, self
        self.library, self.count = device.lib, count

    def __getattr__(self, name):
        entry = getattr(self.library, name)
        if name.endswith('_batch_device'):
            return lambda handle, *passed: entry(handle, *passed, *[None] * self.count)
        return entry


def device_vjp(interp, occupation, x, g=None, g_ngal=None, data=None, precision=None,
               backward=True):
    """The `_device` entries on fresh device arrays: the prediction form (g, or forward only) or
    the likelihood form (data and precision, host arrays there too)."""
    from tabcorr_amd import _lib
    device = interp.to_device()
    n, n_r = len(occupation), len(interp.tabcorr_list[0].tpcf_matrix)
    if data is not None:
        data, precision = _lib.contiguous(np.ravel(data)), _lib.contiguous(precision)
        view = device if backward else WithoutLastOutputs(device, 3)
        return device_call(view, 'tc_interp_chi2_occupation_grad_batch_device',
                           [occupation, x, n, 0, _lib.as_double_p(data),
                            _lib.as_double_p(precision)],
                           [n, n] + [occupation.shape, x.shape, x.shape] * backward,
                           synchronize='tc_interp_synchronize')
    view = device if backward else WithoutLastOutputs(device, 2)
    return device_call(view, 'tc_interp_predict_occupation_vjp_batch_device',
                       [occupation, x, n, 0, g_ngal, g],
                       [n, (n, n_r)] + [occupation.shape, x.shape] * backward,
                       synchronize='tc_interp_synchronize')


@pytest.mark.parametrize('table', [AUTO_TABLES[0], CROSS_TABLES[0]], ids=table_id)
def test_device_entries_and_batch_invariance(table):
    """The `_device` entries return the bits of the host-array ones, in both forms, with and
    without the gradient and with g_ngal = NULL; a draw's results are the same bits alone and at
    another column of a workgroup."""
    case = get_case(table, (4, 5))
    interp = case['interp']
    ref = get_reference(case, 'random', 'random')
    occupation, x, g, g_ngal = np.array(ref['occupation']), np.array(case['x']), ref['g'], \
        ref['g_ngal']
    shaped = g.reshape((N_MAX, ) + case['shape'])
    xi = ref['expect']['xi'][3]
    data, precision = chi2_data(xi.reshape(case['shape']), False)

    def predict(rows):
        got = interp.predict_vjp(occupation[rows], x[rows], shaped[rows], g_ngal[rows])
        return got[0], got[1].reshape(len(got[0]), -1), got[2], got[3]

    def likelihood(rows):
        return interp.chi2_grad_occupation(occupation[rows], x[rows], data, precision)

    for call in (predict, likelihood):
        full = call(slice(0, N_MAX))
        assert all(np.all(np.isfinite(a)) for a in full)
        for rows in (slice(3, D + 4), slice(D, D + 1), slice(N_MAX - 1, N_MAX), slice(6, 7)):
            assert same_bits(call(rows), [a[rows] for a in full]), (call.__name__, rows)
    full = predict(slice(0, N_MAX))
    chi2 = likelihood(slice(0, N_MAX))
    for n in DRAW_COUNTS:
        assert same_bits(device_vjp(interp, occupation[:n], x[:n], g[:n], g_ngal[:n]),
                         [a[:n] for a in full])
        assert same_bits(device_vjp(interp, occupation[:n], x[:n], data=data,
                                    precision=precision), [a[:n] for a in chi2])
    assert same_bits(device_vjp(interp, occupation, x, backward=False), full[:2])
    assert same_bits(device_vjp(interp, occupation, x, data=data, precision=precision,
                                backward=False), chi2[:2])
    without = interp.predict_vjp(occupation, x, shaped)
    assert same_bits(device_vjp(interp, occupation, x, g),
                     (without[0], without[1].reshape(N_MAX, -1), without[2], without[3]))


# ---- what is refused -----------------------------------------------------------------------------

def interp_vjp_lds(mode, n_bins, n_r, n_dim):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    _lib.check(_lib.load().tc_debug_interp_vjp_lds_bytes({'auto': 0, 'cross': 1}[mode], n_bins,
                                                         n_r, n_dim, ctypes.byref(got)))
    return got.value


def check_interpolator_still_serves(interp, tables, points, rtol=RTOL):
    """Every table serves predict_batch, and the interpolator its own."""
    for halotab, table in zip(interp.tabcorr_list, tables):
        check_still_serves(halotab, table, rtol)
    theta = synthetic.zheng07_draws(5, seed=2)
    x = make_x(points, 5, 'inside')
    setup = oracle.interpolator_setup(tables, points)
    expect = oracle.interpolator_predict_zheng07_batch(tables, setup, theta, x)
    ngal, xi = interp.predict_batch(theta, x)
    assert_rel(ngal, expect[0], rtol)
    assert_rel(xi, expect[1], rtol)


def seam_calls(interp, n_classes, n_bins, shape, points):
    """The four calls of the seam on three draws of ones."""
    n_r = int(np.prod(shape))
    occupation = np.ones((3, n_classes, n_bins))
    x = make_x(points, 3, 'inside')
    return [lambda _=None: interp.predict_occupation(occupation, x),
            lambda _=None: interp.predict_vjp(occupation, x, np.ones((3, ) + shape)),
            lambda _=None: interp.chi2_occupation(occupation, x, np.ones(shape), np.eye(n_r)),
            lambda _=None: interp.chi2_grad_occupation(occupation, x, np.ones(shape), np.eye(n_r))]


def test_lds_limit_auto():
    """One axis, three r bins, n_sec = 1: the grid of mode-auto tables with the most bins that the
    documented budget (vjp.h, through its host-only hook) admits runs with (nearly) the whole LDS
    of a CU and matches the reference in both forms; one more primary bin -- the first shape
    beyond the budget (tests/test_interp_vjp_cpu.py) -- is refused by all four calls, naming LDS,
    before anything is launched: the tables and the interpolator go on serving."""
    n_prim = largest(lambda n: interp_vjp_lds('auto', 2 * n, 3, 1) <= LDS_LIMIT)
    assert 2 * n_prim + 2 == 396
    table = (n_prim, 1, (3, ), 'auto')
    case = get_case(table, (4, ), n=D + 1)
    what = 'LDS limit, %d bins' % (2 * n_prim)
    check_call(case, 'random', 'random', D + 1, what)
    xi = get_reference(case, 'random', 'random')['expect']['xi'][3]
    data, precision = chi2_data(xi.reshape((3, )), False)
    check_likelihood(case, 'random', data, precision, [D + 1], what + ' chi2')
    beyond = (n_prim + 1, 1, (3, ), 'auto')
    tables, keys, points = make_tables(beyond, (4, ), 'two')
    interp = make_interpolator(tables, keys, points)
    for call in seam_calls(interp, 2, 2 * n_prim + 2, (3, ), points):
        check_refused(interp.tabcorr_list[0], tables[0], call)
    check_interpolator_still_serves(interp, tables, points)


def test_unsupported_requests_leave_the_interpolator_usable():
    """A float32 interpolator and a wrong occupation shape through the Python layer; flags and a
    partial set of NULL outputs at the C level."""
    from tabcorr_amd import _lib
    table = AUTO_TABLES[0]
    tables, keys, points = make_tables(table, (4, ), 'two')
    single = make_interpolator(tables, keys, points, compute_dtype='float32')
    n_bins = len(tables[0]['gal_type'])
    # (1e-5: the float32 path's stated tolerance)
    for call in seam_calls(single, 2, n_bins, table[2], points):
        check_refused(single.tabcorr_list[0], tables[0], call, 'float64', 1e-5)
    check_interpolator_still_serves(single, tables, points, 1e-5)

    case = get_case(table, (4, ))
    interp = case['interp']
    for call in seam_calls(interp, 3, n_bins, table[2], points) + \
            seam_calls(interp, 2, n_bins + 1, table[2], points):
        with pytest.raises(ValueError, match='occupation'):
            call()
    check_interpolator_still_serves(interp, case['tables'], case['points'])

    device = interp.to_device()
    lib = device.lib
    n_r = case['n_r']
    occupation = np.array(get_occupations(case, 'random')[:5])
    x = np.array(case['x'][:5])
    g = np.ones((5, n_r))
    p = _lib.as_double_p
    out = {'ngal': np.empty(5), 'xi': np.empty((5, n_r)), 'chi2': np.empty(5),
           'g_occupation': np.empty_like(occupation), 'g_x': np.empty_like(x),
           'dngal_dx': np.empty_like(x)}
    data, precision = np.ones(n_r), np.eye(n_r)

    def vjp(flags=0, n_draws=5, skip=()):
        given = {name: None if name in skip else p(array)
                 for name, array in (('g_xi', g), ('g_occupation', out['g_occupation']),
                                     ('g_x', out['g_x']))}
        with device.lock:
            return lib.tc_interp_predict_occupation_vjp_batch(
                device.handle, p(occupation), p(x), n_draws, flags, None, given['g_xi'],
                p(out['ngal']), p(out['xi']), given['g_occupation'], given['g_x'])

    def chi2(flags=0, n_draws=5, skip=()):
        given = [None if name in skip else p(out[name])
                 for name in ('g_occupation', 'g_x', 'dngal_dx')]
        with device.lock:
            return lib.tc_interp_chi2_occupation_grad_batch(
                device.handle, p(occupation), p(x), n_draws, flags, p(data), p(precision),
                p(out['ngal']), p(out['chi2']), *given)

    for flags in (_lib.FLAG_SEPARATE_GAL_TYPE, _lib.FLAG_ASSEMBIAS):
        for status in (vjp(flags), chi2(flags)):
            assert status == _lib.TC_ERR_UNSUPPORTED
            with pytest.raises(NotImplementedError):
                _lib.check(status)
    for skip in (('g_xi', ), ('g_occupation', ), ('g_x', ), ('g_xi', 'g_x')):
        status = vjp(skip=skip)
        assert status == _lib.TC_ERR_INVALID
        with pytest.raises(ValueError, match='g_xi'):
            _lib.check(status)
    for skip in (('g_occupation', ), ('g_x', ), ('dngal_dx', ), ('g_occupation', 'dngal_dx')):
        status = chi2(skip=skip)
        assert status == _lib.TC_ERR_INVALID
        with pytest.raises(ValueError, match='dchi2_docc'):
            _lib.check(status)
    assert vjp(n_draws=-1) == _lib.TC_ERR_INVALID and chi2(n_draws=-1) == _lib.TC_ERR_INVALID
    assert vjp(n_draws=0) == _lib.TC_OK and chi2(n_draws=0) == _lib.TC_OK
    assert vjp() == _lib.TC_OK and chi2() == _lib.TC_OK
    assert vjp(skip=('g_xi', 'g_occupation', 'g_x')) == _lib.TC_OK
    assert chi2(skip=('g_occupation', 'g_x', 'dngal_dx')) == _lib.TC_OK
    check_interpolator_still_serves(interp, case['tables'], case['points'])
    check_call(case, 'random', 'random', D + 1, 'after the refusals')


# ---- end to end: a model the device families do not serve through an interpolator ---------------

def test_leauthaud11_gradient_through_the_seam():
    """A Leauthaud11 model on a 4-node interpolator: chi2_grad_occupation contracted with
    d<N>/dtheta of leauthaud11_grad_reference.py is the gradient of chi2 with respect to the
    eleven parameters, compared with that reference's own Jacobian interpolated over the tables
    (dchi2/dtheta_k = g . sum_t c_t dxi_t,k with g = 2 P_sym (xi - data)); dchi2/dx comes with it.
    Allowance per column: 1e-10 (|reference| + scale), scale = sum_r |g|_r sum_t |c_t| scale_t,k
    with the reference's per-table scale of the cancelling terms and |g| as in
    `vjp_reference.chi2_grad`."""
    table = AUTO_TABLES[0]
    case = get_case(table, (4, ))
    interp, walk, tables = case['interp'], case['walk'], case['tables']
    n = 6
    theta = leauthaud11.leauthaud11_draws(n, seed=5)
    x = np.array(case['x'][:n])
    n_bins = len(tables[0]['gal_type'])
    occupation = np.empty((n, len(walk.class_tables), n_bins))
    docc = np.empty((n, len(walk.class_tables), leauthaud11.N_PARAMS, n_bins))
    for d in range(n):
        for v, k in enumerate(walk.class_tables):
            occupation[d, v] = oracle.mean_occupation(tables[k],
                                                      oracle.Leauthaud11(theta[d], False))
            shared = {}
            for column in range(leauthaud11.N_PARAMS):
                docc[d, v, column] = oracle.mean_occupation(
                    tables[k], leauthaud11.Derivative(theta[d], column, False, shared))
    per_table = [leauthaud11.jacobian_batch(one, theta) for one in tables]
    assert all(leauthaud11.usable(result) for result in per_table)
    xi_t = np.array([r[1].reshape(n, -1) for r in per_table])                  # (K, n, n_r)
    dxi_t = np.array([r[3].reshape(n, leauthaud11.N_PARAMS, -1) for r in per_table])
    scale_t = np.array([r[4] for r in per_table])                              # (K, n, 11)
    weights = [interp_grad_reference.table_weights(case['setup'], case['points'], x[d])
               for d in range(n)]
    c = np.array([w[0] for w in weights])                                      # (n, K)
    dc = np.array([w[1] for w in weights])                                     # (n, D, K)
    abs_c = np.array([w[2] for w in weights])
    xi = np.einsum('dk,kdr->dr', c, xi_t)
    data, precision = chi2_data(xi[3], False)
    p_sym = 0.5 * (precision + precision.T)
    g = 2.0 * (xi - data) @ p_sym
    g_abs = 2.0 * (np.abs(xi) + np.abs(data)) @ np.abs(p_sym)
    expect = np.einsum('dr,dk,kdpr->dp', g, c, dxi_t)
    scale = np.sum(g_abs, axis=1)[:, np.newaxis] * np.einsum('dk,kdp->dp', abs_c, scale_t)
    expect_x = np.einsum('dr,dek,kdr->de', g, dc, xi_t)

    ngal, chi2, dchi2_docc, dchi2_dx, dngal_dx = interp.chi2_grad_occupation(
        occupation, x, data, precision)
    got = np.einsum('dvi,dvpi->dp', dchi2_docc, docc)
    e = xi - data
    assert_rel(chi2, np.einsum('dr,rs,ds->d', e, precision, e), RTOL, 'leauthaud11 chi2')
    check_gradient(got, expect, scale, 'leauthaud11 dchi2/dtheta through the seam')
    seam = reference.batch(reference.chi2_grad, walk, occupation, x, data=data,
                           precision=precision)
    check_gradient(dchi2_dx, expect_x, seam['g_x_scale'], 'leauthaud11 dchi2/dx')
    check_gradient(dngal_dx, seam['dngal_dx'], seam['dngal_dx_scale'], 'leauthaud11 dngal/dx')
