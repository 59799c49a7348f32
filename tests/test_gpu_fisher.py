"""Fisher matrix of the likelihood on the device (TabCorr / Interpolator chi2_fisher_batch,
fisher_batch, fisher; the tc_*chi2_fisher_* entry points) against the reference of
fisher_reference.py: F[k, l] = dxi_k^T P_sym dxi_l from the reference Jacobians of the gradient
suites.  Needs an MI355X.

Allowance: the gradient suites' bar on dxi, |error| <= a = 1e-10 (|dxi| + scale), carried
through the bilinear form, plus 1e-10 of the absolute terms of the sum (fisher_reference.py) --
no new number.  Every case prints its largest error in units of that allowance.  Tables, draws
(grad_reference.stress_draws, logM0 at node midpoints, every draw usable) and reference
Jacobians are those of test_gpu_grad.py and test_gpu_interp_grad.py, made once and shared.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference  # noqa: E402
import grad_reference  # noqa: E402
import interp_grad_reference  # noqa: E402
import test_gpu_grad as table_suite  # noqa: E402
import test_gpu_interp_grad as interp_suite  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    D, LDS_LIMIT, check_refused, chi2_data, device_call, largest, same_bits)
from util import load_golden, table_from_golden  # noqa: E402

pytestmark = pytest.mark.gpu

DRAW_COUNTS = [1, D + 1, 2 * D + 3]
N_MAX = max(DRAW_COUNTS)
assert N_MAX == table_suite.N_MAX == interp_suite.N_MAX


def check_symmetric_to_the_bit(fisher):
    assert np.array_equal(fisher, fisher.transpose(0, 2, 1), equal_nan=True)


def check_positive(fisher, allow):
    """With a symmetric positive-definite precision F is positive semi-definite: the smallest
    eigenvalue of every draw's matrix is at least minus the largest allowance of that draw."""
    for matrix, bound in zip(fisher, allow):
        assert np.linalg.eigvalsh(matrix)[0] >= -np.max(bound)


# ---- tables -----------------------------------------------------------------------------------
# (n_prim, n_sec, n_r) and the axes the r bins are reported on.  Mode auto: one r bin (a rank-1
# matrix) over 4 bins and over 2, 36 bins, 32 bins (whole tiles), 132 and 66 bins with twelve r
# bins on two axes.  Mode cross: 36 bins (one slab) and 66 (two slabs), three r bins and twelve on
# two axes.
AUTO_SHAPES = [((1, 2, 1), None), ((1, 1, 1), None), ((9, 2, 5), None), ((16, 1, 3), None),
               ((33, 2, 12), (3, 4)), ((33, 1, 12), (3, 4))]
CROSS_SHAPES = [((18, 1, 3), None), ((18, 1, 12), (3, 4)), ((33, 1, 3), None),
                ((33, 1, 12), (3, 4))]
TABLE_CASES = ([(shape, 'auto', tpcf_shape) for shape, tpcf_shape in AUTO_SHAPES] +
               [(shape, 'cross', tpcf_shape) for shape, tpcf_shape in CROSS_SHAPES])


def table_id(case):
    shape, mode, tpcf_shape = case
    return '%s-%dx%dx%d%s' % ((mode, ) + shape + (
        '' if tpcf_shape is None else '-as-' + 'x'.join(map(str, tpcf_shape)), ))


def table_inputs(case, modulate, symmetric):
    """The table, all N_MAX draws, dxi and its allowance of the reference, a data vector near
    draw 3's xi (on the table's tpcf_shape) and a precision matrix."""
    shape, mode, tpcf_shape = case
    _, halotab = table_suite.get_table(shape, mode, tpcf_shape)
    theta, reference, _ = table_suite.get_reference(shape, mode, modulate, 10, tpcf_shape,
                                                    usable=True)
    # no draw is left out: every one of them has galaxies and a finite reference
    assert len(theta) == N_MAX and grad_reference.usable(reference)
    data, precision = chi2_data(reference[1][3], symmetric)
    dxi, a = fisher_reference.table_jacobian(reference)
    return halotab, theta, dxi, a, data, precision


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('case', TABLE_CASES, ids=table_id)
def test_table_fisher_matches_reference(case, n_draws, modulate, symmetric):
    """The non-symmetric precision pins the P_sym convention; with the symmetric one every
    draw's matrix is positive semi-definite within its allowance.  The other four results are
    those of chi2_grad_batch to the bit."""
    halotab, theta, dxi, a, data, precision = table_inputs(case, modulate, symmetric)
    theta = theta[:n_draws]
    got = halotab.chi2_fisher_batch(theta, data, precision, modulate_with_cenocc=modulate)
    assert [g.shape for g in got] == [(n_draws, ), (n_draws, ), (n_draws, 5), (n_draws, 5),
                                      (n_draws, 5, 5)]
    what = 'fisher %s n=%d modulate=%s symmetric=%s' % (table_id(case), n_draws, modulate,
                                                        symmetric)
    _, allow = fisher_reference.check(got[4], dxi, a, precision, what)
    check_symmetric_to_the_bit(got[4])
    if symmetric:
        check_positive(got[4], allow)
    assert same_bits(got[:4], halotab.chi2_grad_batch(theta, data, precision,
                                                      modulate_with_cenocc=modulate))


def device_chi2_fisher(halotab, theta, data, precision, flags=0):
    """tc_chi2_fisher_zheng07_batch_device (the data vector and the precision matrix are host
    arrays there too): ngal, chi2, dngal, dchi2, fisher."""
    from tabcorr_amd import _lib
    device = halotab.to_device()
    n = len(theta)
    data = _lib.contiguous(np.ravel(data))
    precision = _lib.contiguous(precision)
    assert data.shape == (device.n_r, ) and precision.shape == (device.n_r, device.n_r)
    return device_call(device, 'tc_chi2_fisher_zheng07_batch_device',
                       [theta, 5, n, 10, flags, _lib.as_double_p(data),
                        _lib.as_double_p(precision)], [n, n, (n, 5), (n, 5), (n, 5, 5)])


@pytest.mark.parametrize('case', [((16, 1, 3), 'auto', None), ((9, 2, 5), 'auto', None),
                                  ((33, 1, 12), 'cross', (3, 4))], ids=table_id)
def test_table_exact_properties(case):
    """What follows from the design, no tolerance: the matrix is symmetric to the bit; the data
    vector does not enter it (fisher_batch); a draw's matrix is the same bits alone, as draw 16
    of 17 and in 35; the host-array and the device-pointer entry return the same bits."""
    from tabcorr_amd import _lib
    halotab, theta, _, _, data, precision = table_inputs(case, False, False)
    full = halotab.chi2_fisher_batch(theta, data, precision)
    assert all(np.all(np.isfinite(a)) for a in full)
    check_symmetric_to_the_bit(full[4])
    assert same_bits(full[:4], halotab.chi2_grad_batch(theta, data, precision))
    forecast = halotab.fisher_batch(theta, precision)
    assert [f.shape for f in forecast] == [(N_MAX, ), (N_MAX, 5), (N_MAX, 5, 5)]
    assert same_bits(forecast, (full[0], full[2], full[4]))
    assert same_bits(halotab.chi2_fisher_batch(theta[D:D + 1], data, precision),
                     [c[D:D + 1] for c in full])
    assert same_bits(halotab.chi2_fisher_batch(theta[:D + 1], data, precision),
                     [c[:D + 1] for c in full])
    for n in DRAW_COUNTS:
        assert same_bits(device_chi2_fisher(halotab, theta[:n], data, precision),
                         [c[:n] for c in full])
    # modulate_with_cenocc through the flags of the device entry
    host = halotab.chi2_fisher_batch(theta[:D + 1], data, precision, modulate_with_cenocc=True)
    assert same_bits(device_chi2_fisher(halotab, theta[:D + 1], data, precision,
                                        flags=_lib.FLAG_MODULATE_WITH_CENOCC), host)
    assert not np.array_equal(host[4], full[4][:D + 1])


def test_real_table_and_the_fisher_matrix_of_a_model():
    """bolplanck_wp, 17 draws, against the reference; `fisher(model, ...)` is row 0 of the batch
    call bit for bit."""
    from tabcorr_amd import TabCorr, Zheng07Model
    from tabcorr_amd.models import ZHENG07_KEYS
    golden = load_golden('bolplanck_wp')
    table = table_from_golden(golden)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                  table['tpcf_shape'], table['attrs'])
    n = D + 1
    theta = np.resize(np.array(golden['theta'], dtype=np.float64), (n, 5)).copy()
    theta[len(golden['theta']):] += 0.01
    theta = grad_reference.centre_log_m0(theta, grad_reference.nodes_of(table))
    reference = grad_reference.jacobian_batch(table, theta)
    assert grad_reference.usable(reference)
    data, precision = chi2_data(reference[1][3], True)
    dxi, a = fisher_reference.table_jacobian(reference)
    got = halotab.chi2_fisher_batch(theta, data, precision)
    _, allow = fisher_reference.check(got[4], dxi, a, precision, 'fisher bolplanck_wp')
    check_symmetric_to_the_bit(got[4])
    check_positive(got[4], allow)
    assert same_bits(got[:4], halotab.chi2_grad_batch(theta, data, precision))
    ngal, dngal, fisher = halotab.fisher_batch(theta, precision)
    assert same_bits((ngal, dngal, fisher), (got[0], got[2], got[4]))
    model = Zheng07Model(redshift=0.0)
    for key, value in zip(ZHENG07_KEYS, theta[0]):
        model.param_dict[key] = value
    one = halotab.fisher(model, precision)
    assert isinstance(one[0], float) and one[0] == ngal[0]
    assert list(one[1]) == list(ZHENG07_KEYS)
    assert all(one[1][key] == dngal[0, k] for k, key in enumerate(ZHENG07_KEYS))
    assert one[2].shape == (5, 5) and np.array_equal(one[2], fisher[0])


# ---- interpolators ----------------------------------------------------------------------------
# Grids (4, ) and (4, 5) -- Q = 6 and 7; 7 gives 448 items, so the workgroup's strided loop runs
# twice -- of 14-bin tables in mode auto and 36-bin tables in mode cross, five r bins.
# Entries: grid, n_prim, mode.
INTERP_CASES = [((4, ), 7, 'auto'), ((4, 5), 7, 'auto'), ((4, ), 18, 'cross'),
                ((4, 5), 18, 'cross')]


def interp_id(entry):
    grid, n_prim, mode = entry
    return '%s-%s-%d' % (mode, 'x'.join(map(str, grid)), 2 * n_prim)


def interp_inputs(case, symmetric):
    expect = case['reference']
    assert len(case['theta']) == N_MAX and interp_grad_reference.usable(expect)
    data, precision = chi2_data(expect['xi'][3].ravel(), symmetric)
    dxi, a = fisher_reference.interp_jacobian(expect)
    return dxi, a, data, precision


def interp_call(case, n, data, precision):
    return case['interp'].chi2_fisher_batch(
        case['theta'][:n], case['x'][:n], data, precision, n_gauss_prim=case['n_gauss'],
        extrapolate=case['extrapolate'], modulate_with_cenocc=case['modulate'])


def check_interp_case(case, n, symmetric, what):
    dxi, a, data, precision = interp_inputs(case, symmetric)
    n_cols = 5 + len(case['interp'].keys)
    got = interp_call(case, n, data, precision)
    assert [g.shape for g in got] == [(n, ), (n, ), (n, n_cols), (n, n_cols), (n, n_cols, n_cols)]
    _, allow = fisher_reference.check(got[4], dxi, a, precision, what)
    check_symmetric_to_the_bit(got[4])
    if symmetric:
        check_positive(got[4], allow)
    assert same_bits(got[:4], case['interp'].chi2_grad_batch(
        case['theta'][:n], case['x'][:n], data, precision, n_gauss_prim=case['n_gauss'],
        extrapolate=case['extrapolate'], modulate_with_cenocc=case['modulate']))
    return got


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('entry', INTERP_CASES, ids=interp_id)
def test_interpolator_fisher_matches_reference(entry, n_draws, symmetric):
    grid, n_prim, mode = entry
    case = interp_suite.get_case(grid, n_prim, 1, (5, ), mode)
    check_interp_case(case, n_draws, symmetric, 'fisher %s n=%d symmetric=%s' % (
        interp_id(entry), n_draws, symmetric))


def test_interpolator_fisher_outside_the_grid():
    """x beyond the grid on both sides with extrapolate=True (two classes of halo tables); without
    it the call is a ValueError."""
    case = interp_suite.get_case((4, 5), 7, 1, (5, ), 'auto', classes='two', x_kind='outside')
    xp = case['setup']['xp']
    assert all(np.all((case['x'][:, d] < xp[d][0]) | (case['x'][:, d] > xp[d][-1]))
               for d in range(2))
    check_interp_case(case, N_MAX, False, 'fisher outside the grid')
    with pytest.raises(ValueError, match='extrapolation'):
        case['interp'].fisher_batch(case['theta'], case['x'], np.eye(5))


def device_interp_chi2_fisher(interp, theta, x, data, precision):
    from tabcorr_amd import _lib
    device = interp.to_device()
    n, n_cols = len(theta), 5 + x.shape[1]
    data = _lib.contiguous(np.ravel(data))
    precision = _lib.contiguous(precision)
    return device_call(device, 'tc_interp_chi2_fisher_zheng07_batch_device',
                       [theta, 5, x, n, 10, 0, _lib.as_double_p(data),
                        _lib.as_double_p(precision)],
                       [n, n, (n, n_cols), (n, n_cols), (n, n_cols, n_cols)],
                       'tc_interp_synchronize')


@pytest.mark.parametrize('entry', [((4, 5), 7, 'auto'), ((4, 5), 18, 'cross')], ids=interp_id)
def test_interpolator_exact_properties(entry):
    """As test_table_exact_properties, and `fisher(model, ...)` against row 3 of the batch."""
    from tabcorr_amd import Zheng07Model
    from tabcorr_amd.models import ZHENG07_KEYS
    grid, n_prim, mode = entry
    case = interp_suite.get_case(grid, n_prim, 1, (5, ), mode)
    interp, theta, x = case['interp'], case['theta'], case['x']
    _, _, data, precision = interp_inputs(case, False)
    full = interp.chi2_fisher_batch(theta, x, data, precision)
    assert all(np.all(np.isfinite(a)) for a in full)
    check_symmetric_to_the_bit(full[4])
    assert same_bits(full[:4], interp.chi2_grad_batch(theta, x, data, precision))
    forecast = interp.fisher_batch(theta, x, precision)
    assert same_bits(forecast, (full[0], full[2], full[4]))
    assert same_bits(interp.chi2_fisher_batch(theta[D:D + 1], x[D:D + 1], data, precision),
                     [c[D:D + 1] for c in full])
    assert same_bits(interp.chi2_fisher_batch(theta[:D + 1], x[:D + 1], data, precision),
                     [c[:D + 1] for c in full])
    for n in DRAW_COUNTS:
        assert same_bits(device_interp_chi2_fisher(interp, theta[:n], x[:n], data, precision),
                         [c[:n] for c in full])
    keys = tuple(ZHENG07_KEYS) + tuple(interp.keys)
    model = Zheng07Model(redshift=0.0)
    for key, value in zip(keys, np.concatenate([theta[3], x[3]])):
        model.param_dict[key] = value
    one = interp.fisher(model, precision)
    assert isinstance(one[0], float) and one[0] == forecast[0][3]
    assert tuple(one[1]) == keys
    assert all(one[1][key] == forecast[1][3, k] for k, key in enumerate(keys))
    assert one[2].shape == (7, 7) and np.array_equal(one[2], forecast[2][3])


# ---- refusals -----------------------------------------------------------------------------------

def test_lds_limit_auto():
    """The Fisher matrix takes no LDS of its own: with three r bins the largest table that
    chi2_grad_batch serves is served, and matches the reference; one primary bin more is refused
    by both, and the handle goes on serving predict_batch."""
    n_r = 3
    n_prim = largest(lambda n: table_suite.auto_lds_bytes(2 * n, n, n_r, True) <= LDS_LIMIT)
    table, halotab, theta, reference = table_suite.lds_limit_case((n_prim, 1, n_r), 'auto')
    data, precision = chi2_data(reference[1][3], False)
    dxi, a = fisher_reference.table_jacobian(reference)
    got = halotab.chi2_fisher_batch(theta, data, precision)
    fisher_reference.check(got[4], dxi, a, precision, 'fisher LDS limit auto %d bins' % (
        2 * n_prim))
    assert same_bits(got[:4], halotab.chi2_grad_batch(theta, data, precision))
    table, halotab = table_suite.make_table((n_prim + 1, 1, n_r), 'auto')
    operands = np.zeros(n_r), np.eye(n_r)
    check_refused(halotab, table, lambda draws: halotab.chi2_fisher_batch(draws, *operands))
    check_refused(halotab, table, lambda draws: halotab.fisher_batch(draws, operands[1]))
    check_refused(halotab, table, lambda draws: halotab.chi2_grad_batch(draws, *operands))


def test_lds_limit_cross():
    """Mode cross at the most r bins that are served, 148 reported as (4, 37): the shape where
    the n_r^2 terms of an entry are most.  One r bin more is refused."""
    n_r = largest(lambda n: table_suite.cross_lds_bytes(n) <= LDS_LIMIT)
    assert n_r == 148
    tpcf_shape = (4, n_r // 4)
    table, halotab, theta, reference = table_suite.lds_limit_case((9, 2, n_r), 'cross',
                                                                  tpcf_shape)
    data, precision = chi2_data(reference[1][3], False)
    dxi, a = fisher_reference.table_jacobian(reference)
    got = halotab.chi2_fisher_batch(theta, data, precision)
    fisher_reference.check(got[4], dxi, a, precision, 'fisher LDS limit cross %d r bins' % n_r)
    check_symmetric_to_the_bit(got[4])
    assert same_bits(got[:4], halotab.chi2_grad_batch(theta, data, precision))
    table, halotab = table_suite.make_table((9, 2, n_r + 1), 'cross')
    operands = np.zeros(n_r + 1), np.eye(n_r + 1)
    check_refused(halotab, table, lambda draws: halotab.chi2_fisher_batch(draws, *operands))
    check_refused(halotab, table, lambda draws: halotab.chi2_grad_batch(draws, *operands))


def test_lds_limit_interpolator():
    """A grid (4, ) of 262-bin tables with four r bins is the largest that chi2_grad_batch
    serves: served here too, against the reference; one primary bin more is refused."""
    n_r, n_prim = 4, 131
    case = interp_suite.get_case((4, ), n_prim, 1, (n_r, ), 'auto')
    check_interp_case(case, D + 1, False, 'fisher LDS limit interpolator')
    tables, keys, points = interp_suite.make_tables((4, ), n_prim + 1, 1, (n_r, ), 'auto', 'one')
    interp = interp_suite.make_interpolator(tables, keys, points)
    theta = synthetic.zheng07_draws(5, seed=2)
    x = interp_suite.make_x(points, None, 5, 'inside', 2)
    with pytest.raises(NotImplementedError, match='LDS'):
        interp.chi2_fisher_batch(theta, x, np.zeros(n_r), np.eye(n_r))
    with pytest.raises(NotImplementedError, match='LDS'):
        interp.chi2_grad_batch(theta, x, np.zeros(n_r), np.eye(n_r))
    interp_suite.check_still_serves(interp, tables, points, theta, x, 1e-10)


def test_float32_tables_are_refused():
    """A float32 table is refused naming float64, for a table and for an interpolator, and goes
    on serving predict_batch (1e-5: the float32 path's stated tolerance)."""
    from tabcorr_amd import TabCorr
    table = synthetic.synthetic_table(9, 2, (5, ), 'auto', seed=3)
    single = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                 table['attrs'], compute_dtype='float32')
    operands = np.zeros(5), np.eye(5)
    check_refused(single, table, lambda draws: single.chi2_fisher_batch(draws, *operands),
                  'float64', 1e-5)
    check_refused(single, table, lambda draws: single.fisher_batch(draws, operands[1]),
                  'float64', 1e-5)

    tables, keys, points = interp_suite.make_tables((4, 5), 7, 1, (5, ), 'auto', 'two')
    theta = synthetic.zheng07_draws(5, seed=2)
    x = interp_suite.make_x(points, None, 5, 'inside', 2)
    single = interp_suite.make_interpolator(tables, keys, points, compute_dtype='float32')
    with pytest.raises(NotImplementedError, match='float64'):
        single.chi2_fisher_batch(theta, x, *operands)
    interp_suite.check_still_serves(single, tables, points, theta, x, 1e-5, gradients=False)
