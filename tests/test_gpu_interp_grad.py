"""Interpolator gradients on the device (Interpolator.predict_batch_grad / chi2_grad_batch /
predict_grad, the tc_interp_*_grad_* entry points) against the reference Jacobian of
interp_grad_reference.py, the forward interpolator and the table gradients.  Needs an MI355X.

Allowance everywhere: 1e-10 relative plus 1e-10 of the absolute scale of the terms that cancel
(interp_grad_reference.jacobian), the gradient suite's own.  Every case prints its largest error
in units of that allowance.  Logical logM0 values sit at node midpoints over the nodes of all
tables (grad_reference.centre_log_m0).
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference  # noqa: E402
import interp_grad_reference as reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    D, LDS_LIMIT, RTOL, chi2_data, device_call, largest, same_bits)
from util import assert_rel  # noqa: E402

pytestmark = pytest.mark.gpu

DRAW_COUNTS = [1, D + 1, 2 * D + 3]
N_MAX = max(DRAW_COUNTS)

_cases = {}


def make_tables(grid, n_prim, n_sec, tpcf_shape, mode, classes):
    """Tables and points of a synthetic grid.  classes: 'one' (a shared gal_type), 'two' (every
    other table in list order has another n_h: two classes interleaved), 'own' (every table its
    own n_h: K classes), 'shuffled' (two classes, the list in a random order)."""
    tables, keys, points = synthetic.synthetic_interpolator(grid, n_prim, n_sec, tpcf_shape, mode,
                                                            seed=40)
    for k, table in enumerate(tables):
        factor = {'one': 1.0, 'two': 1.0 + 0.2 * (k % 2), 'shuffled': 1.0 + 0.2 * (k % 2),
                  'own': 1.0 + 0.03 * k}[classes]
        if factor != 1.0:
            table['gal_type'] = table['gal_type'].copy()
            table['gal_type']['n_h'] *= factor
    if classes == 'shuffled':
        order = np.random.default_rng(9).permutation(len(tables))
        tables, points = [tables[k] for k in order], points[order]
    return tables, keys, points


def make_interpolator(tables, keys, points, **kwargs):
    from tabcorr_amd import Interpolator, TabCorr
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'],
                                    **kwargs) for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)})


def make_x(points, setup, n, kind, seed):
    """(n, D) extra parameters: 'inside' uniform over the grid; 'node' on grid nodes (table
    k % K for draw k); 'knot' an interior knot of the last axis; 'last' the last knot of the
    first axis; 'outside' beyond the grid, below on even draws and above on odd ones."""
    rng = np.random.default_rng(seed)
    low, high = points.min(axis=0), points.max(axis=0)
    x = rng.uniform(low, high, size=(n, points.shape[1]))
    if kind == 'node':
        x = points[np.arange(n) % len(points)].copy()
    elif kind == 'knot':
        x[:, -1] = setup['xp'][-1][1 + np.arange(n) % (len(setup['xp'][-1]) - 2)]
    elif kind == 'last':
        x[:, 0] = high[0]
    elif kind == 'outside':
        span = high - low
        x[0::2] = low - rng.uniform(0.05, 0.3, size=x[0::2].shape) * span
        x[1::2] = high + rng.uniform(0.05, 0.3, size=x[1::2].shape) * span
    else:
        assert kind == 'inside'
    return x


def get_case(grid, n_prim, n_sec, tpcf_shape, mode, classes='one', modulate=False, n_gauss=10,
             x_kind='inside'):
    """Interpolator, its tables, draws (theta, x) and their reference, made once per combination
    and never modified: a batch of n draws is the first n of them.  The seed of the draws is the
    first one from 5 on with which every draw has galaxies and only finite reference results,
    chosen from the reference alone."""
    key = (grid, n_prim, n_sec, tpcf_shape, mode, classes, modulate, n_gauss, x_kind)
    if key not in _cases:
        tables, keys, points = make_tables(grid, n_prim, n_sec, tpcf_shape, mode, classes)
        setup = oracle.interpolator_setup(tables, points)
        nodes = np.unique(np.concatenate([grad_reference.nodes_of(t, n_gauss) for t in tables]))
        for seed in range(5, 25):
            theta = grad_reference.centre_log_m0(
                grad_reference.stress_draws(tables[0], N_MAX, seed=seed, n_gauss_prim=n_gauss),
                nodes)
            x = make_x(points, setup, N_MAX, x_kind, seed)
            with np.errstate(all='ignore'):
                expect = reference.jacobian_batch(tables, setup, points, theta, x, n_gauss,
                                                  modulate)
            if reference.usable(expect):
                break
        else:
            raise AssertionError('no seed gives usable draws for %s' % (key, ))
        for array in [theta, x] + list(expect.values()):
            array.setflags(write=False)
        _cases[key] = {'interp': make_interpolator(tables, keys, points), 'tables': tables,
                       'points': points, 'setup': setup, 'theta': theta, 'x': x,
                       'reference': expect, 'modulate': modulate, 'n_gauss': n_gauss,
                       'extrapolate': x_kind == 'outside'}
    return _cases[key]


def call(case, n, **kwargs):
    return case['interp'].predict_batch_grad(
        case['theta'][:n], case['x'][:n], n_gauss_prim=case['n_gauss'],
        extrapolate=case['extrapolate'], modulate_with_cenocc=case['modulate'], **kwargs)


def check_case(case, n, what):
    """Shapes, the reference Jacobian, and ngal / xi against the forward interpolator."""
    interp = case['interp']
    got = call(case, n)
    shape = tuple(interp.tabcorr_list[0].tpcf_shape)
    n_cols = 5 + len(interp.keys)
    assert got[0].shape == (n, ) and got[1].shape == (n, ) + shape
    assert got[2].shape == (n, n_cols) and got[3].shape == (n, n_cols) + shape
    reference.check(got, reference.first(case['reference'], n), what)
    ngal, xi = interp.predict_batch(case['theta'][:n], case['x'][:n],
                                    n_gauss_prim=case['n_gauss'],
                                    extrapolate=case['extrapolate'],
                                    modulate_with_cenocc=case['modulate'])
    assert_rel(got[0], ngal, RTOL, what + ' ngal against predict_batch')
    assert_rel(got[1], xi, RTOL, what + ' xi against predict_batch')
    return got


# Mode auto: 14 and 28 bins (n_sec 1 and 2: one row tile and a second one), 18 bins (a second row
# tile with two rows); five r bins and twelve reported as (3, 4); ten nodes and one; grids of one,
# two and three dimensions.  Mode cross: 36 bins and 66 (one slab of 64 plus two bins).
# Entries: grid, n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss.
MAIN_CASES = [
    ((4, ), 7, 1, (5, ), 'auto', False, 10),
    ((4, 5), 7, 2, (5, ), 'auto', False, 10),
    ((4, 4, 4), 7, 1, (5, ), 'auto', False, 10),
    ((4, 5), 9, 1, (3, 4), 'auto', True, 10),
    ((4, ), 9, 1, (5, ), 'auto', False, 1),
    ((4, 5), 7, 1, (3, 4), 'auto', True, 1),
    ((4, 5), 18, 1, (5, ), 'cross', False, 10),
    ((4, 5), 33, 1, (3, 4), 'cross', True, 10),
    ((4, ), 18, 1, (5, ), 'cross', True, 1),
]


def main_id(case):
    grid, n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss = case
    return '%s-%s-%dx%d-r%s-%s-ng%d' % (
        mode, 'x'.join(map(str, grid)), n_prim, n_sec, 'x'.join(map(str, tpcf_shape)),
        'modulate' if modulate else 'plain', n_gauss)


@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('entry', MAIN_CASES, ids=main_id)
def test_gradient_matches_reference_jacobian(entry, n_draws):
    grid, n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss = entry
    case = get_case(grid, n_prim, n_sec, tpcf_shape, mode, modulate=modulate, n_gauss=n_gauss)
    check_case(case, n_draws, '%s n=%d' % (main_id(entry), n_draws))


@pytest.mark.parametrize('classes', ['own', 'two', 'one', 'shuffled'])
@pytest.mark.parametrize('mode,n_prim', [('auto', 7), ('cross', 18)])
def test_classes_of_halo_tables(mode, n_prim, classes):
    """K classes, two classes interleaved in list order, one class, a shuffled list: the walk is
    class by class, the results are those of the list."""
    case = get_case((4, 5), n_prim, 1, (5, ), mode, classes=classes)
    n_classes = len(np.unique(case['setup']['unique_inverse']))
    assert n_classes == {'own': 20, 'two': 2, 'one': 1, 'shuffled': 2}[classes]
    check_case(case, D + 1, '%s classes=%s' % (mode, classes))


@pytest.mark.parametrize('x_kind', ['node', 'knot', 'last', 'outside'])
@pytest.mark.parametrize('mode,n_prim', [('auto', 7), ('cross', 18)])
def test_positions_of_x(mode, n_prim, x_kind):
    """On a grid node, on an interior knot of one axis, on the last knot, outside the grid on
    both sides with extrapolate=True."""
    case = get_case((4, 5), n_prim, 1, (5, ), mode, classes='two', x_kind=x_kind)
    n = 2 * D + 3
    got = check_case(case, n, '%s x=%s' % (mode, x_kind))
    if x_kind == 'outside':
        xp = case['setup']['xp']
        assert all(np.all((case['x'][:, d] < xp[d][0]) | (case['x'][:, d] > xp[d][-1]))
                   for d in range(2))
        with pytest.raises(ValueError, match='extrapolation'):
            case['interp'].predict_batch_grad(case['theta'][:n], case['x'][:n])
    if x_kind == 'node':
        # the value and the theta derivatives are those of the node's table
        expect = reference.first(case['reference'], n)
        for k in range(0, n, 7):
            table = case['interp'].tabcorr_list[k % 20]
            one = table.predict_batch_grad(case['theta'][k:k + 1])
            mine = (got[0][k:k + 1], got[1][k:k + 1], got[2][k:k + 1, :5], got[3][k:k + 1, :5])
            for name, a, b in zip(('ngal', 'xi', 'dngal', 'dxi'), mine, one):
                scale = expect[name + '_scale'][k:k + 1]
                scale = scale[:, :5] if name in ('dngal', 'dxi') else scale
                assert np.all(np.abs(a - b) <= RTOL * np.abs(b) + RTOL * scale), (name, k)


def test_grid_of_identical_tables():
    """d/dx is zero within the allowance and d/dtheta that of the single table."""
    tables, keys, points = synthetic.synthetic_interpolator((4, 5), 7, 1, (5, ), 'auto', seed=40)
    tables = [tables[0]] * len(tables)
    interp = make_interpolator(tables, keys, points)
    setup = oracle.interpolator_setup(tables, points)
    n = D + 1
    for seed in range(5, 25):
        theta = grad_reference.stress_draws(tables[0], n, seed=seed)
        x = make_x(points, setup, n, 'inside', seed)
        with np.errstate(all='ignore'):
            expect = reference.jacobian_batch(tables, setup, points, theta, x)
        if reference.usable(expect):
            break
    assert reference.usable(expect)
    got = interp.predict_batch_grad(theta, x)
    reference.check(got, expect, 'identical tables')
    assert np.all(np.abs(got[2][:, 5:]) <= RTOL * expect['dngal_scale'][:, 5:])
    assert np.all(np.abs(got[3][:, 5:]) <= RTOL * expect['dxi_scale'][:, 5:])
    one = interp.tabcorr_list[0].predict_batch_grad(theta)
    for name, a, b in (('ngal', got[0], one[0]), ('xi', got[1], one[1]),
                       ('dngal', got[2][:, :5], one[2]), ('dxi', got[3][:, :5], one[3])):
        scale = expect[name + '_scale']
        scale = scale[:, :5] if name in ('dngal', 'dxi') else scale
        assert np.all(np.abs(a - b) <= RTOL * np.abs(b) + RTOL * scale), name


# ---- the likelihood ---------------------------------------------------------------------------

def chi2_inputs(case, symmetric):
    """A data vector near draw 3's xi and a precision matrix."""
    return chi2_data(case['reference']['xi'][3].ravel(), symmetric)


def check_chi2_values(got, expect, data, precision, what):
    """chi2 = e^T P e and dchi2_k = 2 e^T P_sym dxi_k against the reference, with the allowances
    of xi (a_r = 1e-10 (|xi_r| + xi_scale_r)) and dxi (a_rk = 1e-10 (|dxi_rk| + dxi_scale_rk))
    carried through the two formulas, v = 2 P_sym e:
    chi2: rtol + sum_r |v_r| a_r;  dchi2_k: rtol + sum_r |v_r| a_rk + 2 sum_r (|P_sym| a)_r |dxi_rk|."""
    ngal, chi2, dngal, dchi2 = got
    n = len(ngal)
    xi = expect['xi'].reshape(n, -1)
    dxi = expect['dxi'].reshape(n, expect['dxi'].shape[1], -1)
    a_r = RTOL * (np.abs(xi) + expect['xi_scale'].reshape(n, -1))
    a_rk = RTOL * (np.abs(dxi) + expect['dxi_scale'].reshape(dxi.shape))
    p_sym = 0.5 * (precision + precision.T)
    e = xi - data
    v = 2.0 * e @ p_sym
    chi2_ref = np.einsum('nr,rs,ns->n', e, precision, e)
    dchi2_ref = np.einsum('nr,nkr->nk', v, dxi)
    chi2_allow = RTOL * np.abs(chi2_ref) + np.sum(np.abs(v) * a_r, axis=1)
    dchi2_allow = (RTOL * np.abs(dchi2_ref) + np.einsum('nr,nkr->nk', np.abs(v), a_rk) +
                   2.0 * np.einsum('nr,nkr->nk', a_r @ np.abs(p_sym), np.abs(dxi)))
    print('%s: max error / allowance = %.3g (chi2), %.3g (dchi2)' % (
        what, np.max(np.abs(chi2 - chi2_ref) / chi2_allow),
        np.max(np.abs(dchi2 - dchi2_ref) / np.maximum(dchi2_allow, 1e-300))))
    assert chi2.shape == (n, ) and dchi2.shape == dchi2_ref.shape
    assert np.all(np.abs(chi2 - chi2_ref) <= chi2_allow)
    assert np.all(np.abs(dchi2 - dchi2_ref) <= dchi2_allow)
    for name, value in (('ngal', ngal), ('dngal', dngal)):
        allowance = RTOL * np.abs(expect[name]) + RTOL * expect[name + '_scale']
        assert np.all(np.abs(value - expect[name]) <= allowance), name


CHI2_CASES = [((4, 5), 7, 2, (5, ), 'auto', False), ((4, 5), 9, 1, (3, 4), 'auto', True),
              ((4, 5), 33, 1, (3, 4), 'cross', True)]


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('entry', CHI2_CASES,
                         ids=[main_id(e + (10, )) for e in CHI2_CASES])
def test_chi2_gradient(entry, n_draws, symmetric):
    """The non-symmetric precision pins the P_sym convention."""
    grid, n_prim, n_sec, tpcf_shape, mode, modulate = entry
    case = get_case(grid, n_prim, n_sec, tpcf_shape, mode, modulate=modulate)
    data, precision = chi2_inputs(case, symmetric)
    interp = case['interp']
    theta, x = case['theta'][:n_draws], case['x'][:n_draws]
    got = interp.chi2_grad_batch(theta, x, data.reshape(tpcf_shape), precision,
                                 modulate_with_cenocc=modulate)
    check_chi2_values(got, reference.first(case['reference'], n_draws), data, precision,
                      'chi2 %s n=%d' % (main_id(entry + (10, )), n_draws))
    # the value agrees with the forward entry point to parity
    assert_rel(got[1], interp.chi2_batch(theta, x, data, precision,
                                         modulate_with_cenocc=modulate)[1], RTOL)


def device_grad(interp, theta, x, data=None, precision=None, n_gauss=10, flags=0):
    """tc_interp_predict_grad_zheng07_batch_device or, with data, the chi2 entry."""
    from tabcorr_amd import _lib
    device = interp.to_device()
    n, n_r, n_cols = len(theta), device.tables[0].n_r, 5 + x.shape[1]
    arguments = [theta, 5, x, n, n_gauss, flags]
    if data is None:
        return device_call(device, 'tc_interp_predict_grad_zheng07_batch_device', arguments,
                           [n, (n, n_r), (n, n_cols), (n, n_cols, n_r)], 'tc_interp_synchronize')
    data = _lib.contiguous(np.ravel(data))
    precision = _lib.contiguous(precision)
    return device_call(device, 'tc_interp_chi2_grad_zheng07_batch_device',
                       arguments + [_lib.as_double_p(data), _lib.as_double_p(precision)],
                       [n, n, (n, n_cols), (n, n_cols)], 'tc_interp_synchronize')


@pytest.mark.parametrize('entry', [((4, 5), 7, 2, (5, ), 'auto'), ((4, 5), 33, 1, (3, 4), 'cross'),
                                   ((4, 4, 4), 7, 1, (5, ), 'auto')],
                         ids=['auto-4x5', 'cross-4x5', 'auto-4x4x4'])
def test_batch_invariance_and_device_entries(entry):
    """The kernels have one form and every sum an order fixed by the interpolator: a draw's
    results are bit-equal in batches of 1, D + 1 and 2 D + 3 draws, alone or among others, and
    between the host-array and the device-pointer entry points -- conditions that follow from the
    design, no tolerance.  Three device-pointer calls in a row also use the interpolator's lanes
    in turn."""
    grid, n_prim, n_sec, tpcf_shape, mode = entry
    case = get_case(grid, n_prim, n_sec, tpcf_shape, mode, classes='one')
    interp, theta, x = case['interp'], case['theta'], case['x']
    data, precision = chi2_inputs(case, False)
    full = interp.predict_batch_grad(theta, x)
    full_chi2 = interp.chi2_grad_batch(theta, x, data, precision)
    assert all(np.all(np.isfinite(a)) for a in full + full_chi2)
    for n in DRAW_COUNTS:
        part = interp.predict_batch_grad(theta[:n], x[:n])
        device = device_grad(interp, theta[:n], x[:n])
        assert same_bits(part, [c[:n] for c in full]) and same_bits(device, part, reshape=True)
        part = interp.chi2_grad_batch(theta[:n], x[:n], data, precision)
        device = device_grad(interp, theta[:n], x[:n], data, precision)
        assert same_bits(part, [c[:n] for c in full_chi2]) and same_bits(device, part)
    # the last draw alone (column 0 of its workgroup instead of column 2)
    for alone, whole in ((interp.predict_batch_grad(theta[-1:], x[-1:]), full),
                         (interp.chi2_grad_batch(theta[-1:], x[-1:], data, precision), full_chi2)):
        assert same_bits(alone, [c[-1:] for c in whole])


def test_predict_grad_of_a_model():
    from tabcorr_amd import Zheng07Model
    from tabcorr_amd.models import ZHENG07_KEYS
    case = get_case((4, 5), 9, 1, (3, 4), 'auto', modulate=True)
    interp = case['interp']
    ngal, xi, dngal, dxi = call(case, 4)
    keys = tuple(ZHENG07_KEYS) + tuple(interp.keys)
    assert keys[5:] == ('log_eta', 'alpha_s')
    model = Zheng07Model(redshift=0.0, modulate_with_cenocc=True)
    for key, value in zip(keys, np.concatenate([case['theta'][3], case['x'][3]])):
        model.param_dict[key] = value
    one = interp.predict_grad(model)
    assert isinstance(one[0], float) and one[1].shape == (3, 4)
    assert tuple(one[2]) == keys and tuple(one[3]) == keys
    assert one[0] == ngal[3] and np.array_equal(one[1], xi[3])
    for k, key in enumerate(keys):
        assert one[2][key] == dngal[3, k]
        assert np.array_equal(one[3][key], dxi[3, k])


# ---- the LDS limit ------------------------------------------------------------------------------
# The documented budget of grad_interp_auto_kernel (csrc/grad.h), in rows of D doubles: the rows
# of a table (three per central bin, six per satellite bin, one of zeros), six rows of totals, the
# weights and derivative weights of every axis (2 x 32 rows per dimension) and 6 + n_dim
# accumulators per r bin; the likelihood is finished in the accumulators.


# (a restatement of grad_interp_auto_lds_bytes, which is not exported: keep it in step with
# csrc/grad.h -- the pass at the largest shape and the refusal one bin later pin the two together)
def auto_lds_bytes(n_bins, n_central, n_r, n_dim, chi2):
    rows = (3 * n_central + 6 * (n_bins - n_central) + 1) + 6 + 2 * 32 * n_dim + (6 + n_dim) * n_r
    return rows * D * 8


def test_lds_limit_auto():
    """A grid (4, ) with four r bins: 131 primary bins (262 bins) need 163 584 of the 163 840
    bytes and are served, by both calls, and match the reference; one primary bin more (164 736
    bytes) is refused by both, and the interpolator goes on serving predict_batch."""
    n_r, n_dim = 4, 1
    n_prim = largest(lambda n: auto_lds_bytes(2 * n, n, n_r, n_dim, False) <= LDS_LIMIT)
    assert n_prim == 131 and auto_lds_bytes(2 * n_prim, n_prim, n_r, n_dim, False) == 163584
    assert auto_lds_bytes(2 * n_prim + 2, n_prim + 1, n_r, n_dim, True) == 164736
    case = get_case((4, ), n_prim, 1, (n_r, ), 'auto')
    n = D + 1
    check_case(case, n, 'LDS limit auto %d bins' % (2 * n_prim))
    data, precision = chi2_inputs(case, False)
    got = case['interp'].chi2_grad_batch(case['theta'][:n], case['x'][:n], data, precision)
    check_chi2_values(got, reference.first(case['reference'], n), data, precision,
                      'LDS limit auto chi2')
    tables, keys, points = make_tables((4, ), n_prim + 1, 1, (n_r, ), 'auto', 'one')
    interp = make_interpolator(tables, keys, points)
    theta = synthetic.zheng07_draws(5, seed=2)
    x = make_x(points, None, 5, 'inside', 2)
    with pytest.raises(NotImplementedError, match='LDS'):
        interp.predict_batch_grad(theta, x)
    with pytest.raises(NotImplementedError, match='LDS'):
        interp.chi2_grad_batch(theta, x, np.zeros(n_r), np.eye(n_r))
    check_still_serves(interp, tables, points, theta, x, RTOL)


def check_still_serves(interp, tables, points, theta, x, rtol, gradients=True):
    """The interpolator serves predict_batch and its tables predict_batch_grad."""
    setup = oracle.interpolator_setup(tables, points)
    expect = oracle.interpolator_predict_zheng07_batch(tables, setup, theta, x)
    ngal, xi = interp.predict_batch(theta, x)
    assert_rel(ngal, expect[0], rtol)
    assert_rel(xi, expect[1], rtol)
    if gradients:
        ngal, xi, dngal, dxi = interp.tabcorr_list[-1].predict_batch_grad(theta)
        one = oracle.predict_zheng07_batch(tables[-1], theta)
        assert_rel(ngal, one[0], RTOL)
        assert_rel(xi, one[1], RTOL)
        assert np.all(np.isfinite(dngal)) and np.all(np.isfinite(dxi))


def test_unsupported_requests_leave_the_interpolator_usable():
    from tabcorr_amd import _lib
    tables, keys, points = make_tables((4, 5), 7, 1, (5, ), 'auto', 'two')
    theta = synthetic.zheng07_draws(5, seed=2)
    x = make_x(points, None, 5, 'inside', 2)

    single = make_interpolator(tables, keys, points, compute_dtype='float32')
    with pytest.raises(NotImplementedError, match='float64'):
        single.predict_batch_grad(theta, x)
    with pytest.raises(NotImplementedError, match='float64'):
        single.chi2_grad_batch(theta, x, np.zeros(5), np.eye(5))
    check_still_serves(single, tables, points, theta, x, 1e-5, gradients=False)

    interp = make_interpolator(tables, keys, points)
    device = interp.to_device()
    n, n_r = len(theta), 5
    outputs = [np.empty(n * 2), np.empty(n * 3 * n_r), np.empty(n * 2 * 9),
               np.empty(n * 3 * 9 * n_r)]
    for flags, columns in ((_lib.FLAG_SEPARATE_GAL_TYPE, 5), (_lib.FLAG_ASSEMBIAS, 7),
                           (_lib.FLAG_LEAUTHAUD11, 5)):
        wide = np.ascontiguousarray(np.hstack([theta, np.zeros((n, 2))])[:, :columns])
        with device.lock:
            status = device.lib.tc_interp_predict_grad_zheng07_batch(
                device.handle, _lib.as_double_p(wide), columns, _lib.as_double_p(x), n, 10, flags,
                *[_lib.as_double_p(a) for a in outputs])
        assert status == _lib.TC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            _lib.check(status)
        with device.lock:
            status = device.lib.tc_interp_chi2_grad_zheng07_batch(
                device.handle, _lib.as_double_p(wide), columns, _lib.as_double_p(x), n, 10, flags,
                _lib.as_double_p(np.zeros(n_r)), _lib.as_double_p(np.eye(n_r)),
                *[_lib.as_double_p(a) for a in outputs])
        assert status == _lib.TC_ERR_UNSUPPORTED
        check_still_serves(interp, tables, points, theta, x, RTOL)
    # and the gradient call itself still serves the interpolator
    setup = oracle.interpolator_setup(tables, points)
    nodes = np.unique(np.concatenate([grad_reference.nodes_of(t) for t in tables]))
    theta = grad_reference.centre_log_m0(theta.copy(), nodes)
    expect = reference.jacobian_batch(tables, setup, points, theta, x)
    reference.check(interp.predict_batch_grad(theta, x), expect, 'after the refused calls')
