"""Gradients of Zheng07 decorated with assembly bias on the device (`assembias=True` of
predict_batch_grad / chi2_grad_batch / chi2_fisher_batch / fisher_batch / predict_grad / fisher of
TabCorr and Interpolator, the tc_*_grad_assembias_* entry points) against the seven-column
reference Jacobian of assembias_grad_reference.py and the oracle's values.  Needs an MI355X.

Allowance of a derivative, as in test_gpu_grad.py: 1e-10 |reference| (the project's parity bar)
plus 1e-10 of the size of the terms that cancel in it (the reference's `scale`); the likelihood
and the Fisher matrix carry it through their formulas (test_gpu_grad.check_chi2_values,
fisher_reference).  Every case prints its largest error in units of its allowance.  logM0 and
logMmin of every draw sit at node midpoints (the function has kinks where they cross a node).
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assembias_grad_reference as reference  # noqa: E402
import fisher_reference  # noqa: E402
import grad_reference  # noqa: E402
import interp_grad_reference  # noqa: E402
import test_gpu_grad as table_suite  # noqa: E402
import test_gpu_interp_grad as interp_suite  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    D, LDS_LIMIT, RTOL, check_still_serves, chi2_data, device_call, largest, same_bits)
from util import assert_rel  # noqa: E402

pytestmark = pytest.mark.gpu

DRAW_COUNTS = [1, D + 1, 2 * D + 3]
N_MAX = max(DRAW_COUNTS)

_tables = {}
_references = {}


def get_table(n_prim, n_sec, tpcf_shape, mode):
    from tabcorr_amd import TabCorr
    key = (n_prim, n_sec, tpcf_shape, mode)
    if key not in _tables:
        table = reference.synthetic_table(n_prim, n_sec, tpcf_shape, mode, seed=3)
        _tables[key] = (table, TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                                   table['tpcf_shape'], table['attrs']))
    return _tables[key]


def oracle_values(table, theta, n_gauss, modulate):
    return oracle.predict_zheng07_batch(table, theta[:, :5], n_gauss_prim=n_gauss,
                                        modulate_with_cenocc=modulate, assembias=theta[:, 5:])


def get_reference(n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss, n_draws=N_MAX):
    """Draws (n_draws, 7), their reference (ngal, xi, dngal, dxi, scale) and the oracle's values,
    computed once per combination and never modified: a batch of n draws is the first n of them.
    The seed is the first one from 5 on with which every draw has galaxies and only finite
    reference results, and with which the reference's own rounding stays below a tenth of the
    allowance (assembias_grad_reference.rounding_of_centrals) -- chosen from the reference
    alone."""
    key = (n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss, n_draws)
    if key not in _references:
        table, _ = get_table(n_prim, n_sec, tpcf_shape, mode)
        for seed in range(5, 25):
            theta = reference.stress_draws(table, n_draws, seed=seed, n_gauss_prim=n_gauss)
            with np.errstate(all='ignore'):
                expect = reference.jacobian_batch(table, theta, n_gauss, modulate)
            if reference.usable(expect) and reference.well_conditioned(table, theta, expect,
                                                                        n_gauss, modulate):
                break
        else:
            raise AssertionError('no seed gives usable draws for %s' % (key, ))
        values = oracle_values(table, theta, n_gauss, modulate)
        for array in (theta, ) + expect + values:
            array.setflags(write=False)
        _references[key] = (theta, expect, values)
    return _references[key]


def check_clipped_columns(theta, dngal, dxi):
    """A strength beyond [-1, 1] is clipped: its column is exactly zero."""
    for k in (5, 6):
        beyond = np.abs(theta[:, k]) > 1.0
        assert np.all(dngal[beyond, k] == 0.0) and np.all(dxi[beyond, k] == 0.0)


def check_gradient(halotab, theta, expect, values, n_gauss, modulate, tpcf_shape, what):
    n = len(theta)
    ngal, xi, dngal, dxi = halotab.predict_batch_grad(
        theta, n_gauss_prim=n_gauss, modulate_with_cenocc=modulate, assembias=True)
    assert ngal.shape == (n, ) and xi.shape == (n, ) + tpcf_shape
    assert dngal.shape == (n, 7) and dxi.shape == (n, 7) + tpcf_shape
    assert_rel(ngal, values[0][:n], RTOL, what + ' ngal')
    assert_rel(xi, values[1][:n], RTOL, what + ' xi')
    assert_rel(ngal, expect[0][:n], RTOL, what + ' ngal')
    table_suite.check_derivatives(dngal, dxi, tuple(a[:n] for a in expect), what)
    check_clipped_columns(theta, dngal, dxi)
    return ngal, xi, dngal, dxi


# (n_prim, n_sec, tpcf_shape).  Mode auto: 4 bins (one step of four matrix columns), 16 bins (one
# whole tile), 36 bins (padding), 18 bins that all lie below the split, 36 bins of which a third
# sit at percentile exactly 0.5 (below) with twelve r bins on two axes.  Mode cross: 36 bins (one
# slab) and 68 (a slab and four bins).
AUTO_SHAPES = [(1, 2, (1, )), (4, 2, (5, )), (9, 2, (5, )), (9, 1, (5, )), (6, 3, (3, 4))]
CROSS_SHAPES = [(9, 2, (5, )), (17, 2, (5, ))]
CASES = ([shape + ('auto', ) for shape in AUTO_SHAPES] +
         [shape + ('cross', ) for shape in CROSS_SHAPES])


def case_id(case):
    n_prim, n_sec, tpcf_shape, mode = case
    return '%s-%dx%dx%s' % (mode, n_prim, n_sec, 'x'.join(map(str, tpcf_shape)))


@pytest.mark.parametrize('n_gauss', [10, 1])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_gradient_matches_reference_jacobian(case, n_draws, modulate, n_gauss):
    n_prim, n_sec, tpcf_shape, mode = case
    table, halotab = get_table(*case)
    theta, expect, values = get_reference(n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss)
    assert len(theta) == N_MAX and np.all(values[0] > 0.0)
    if n_sec == 3:
        assert np.sum(table['gal_type']['sec_haloprop_percentile'] == 0.5) == 2 * n_prim
    check_gradient(halotab, theta[:n_draws], expect, values, n_gauss, modulate, tpcf_shape,
                   '%s n=%d modulate=%s ng=%d' % (case_id(case), n_draws, modulate, n_gauss))


def test_satellites_above_the_split_vanish_at_minus_one():
    """A_sat = -1: the satellite bins above the split hold no galaxies, yet the A_sat column is
    the plain occupation's, not zero (the derivative at the boundary faces inside)."""
    case = (9, 2, (5, ), 'auto')
    table, halotab = get_table(*case)
    theta, expect, _ = get_reference(*case, False, 10)
    rows = np.nonzero(theta[:, 6] == -1.0)[0]
    assert len(rows) >= 2
    _, _, dngal, dxi = halotab.predict_batch_grad(theta, assembias=True)
    assert np.all(np.any(expect[3][rows, 6] != 0.0, axis=-1))
    assert np.all(np.any(dxi[rows, 6] != 0.0, axis=-1))
    gal_type = table['gal_type']
    gone = ~oracle.is_centrals(gal_type) & (gal_type['sec_haloprop_percentile'] > 0.5)
    for row in rows:
        assert np.all(oracle.mean_occupation(table, reference.model(theta[row]))[gone] == 0.0)


# ---- likelihood and Fisher matrix ---------------------------------------------------------------

def flat_reference(expect, n):
    """The first n draws with the r bins on one axis."""
    ngal, xi, dngal, dxi, scale = (a[:n] for a in expect)
    return ngal, xi.reshape(n, -1), dngal, dxi.reshape(n, 7, -1), scale


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('case', [(1, 2, (1, ), 'auto'), (9, 2, (5, ), 'auto'),
                                  (6, 3, (3, 4), 'auto'), (9, 2, (5, ), 'cross'),
                                  (17, 2, (3, 4), 'cross')], ids=case_id)
def test_likelihood_and_fisher(case, n_draws, modulate, symmetric):
    """chi2, dchi2 (allowances of test_gpu_grad.test_chi2_gradient) and fisher (7, 7)
    (fisher_reference) against the reference Jacobian; the non-symmetric precision pins the
    P_sym convention.  fisher is symmetric to the bit, and the other four results of the Fisher
    call are those of the gradient call bit for bit."""
    n_prim, n_sec, tpcf_shape, mode = case
    _, halotab = get_table(*case)
    theta, expect, _ = get_reference(n_prim, n_sec, tpcf_shape, mode, modulate, 10)
    data, precision = chi2_data(expect[1][3].ravel(), symmetric)
    theta = theta[:n_draws]
    what = '%s n=%d modulate=%s symmetric=%s' % (case_id(case), n_draws, modulate, symmetric)
    got = halotab.chi2_fisher_batch(theta, data.reshape(tpcf_shape), precision,
                                    modulate_with_cenocc=modulate, assembias=True)
    assert [g.shape for g in got] == [(n_draws, ), (n_draws, ), (n_draws, 7), (n_draws, 7),
                                      (n_draws, 7, 7)]
    flat = flat_reference(expect, n_draws)
    table_suite.check_chi2_values(got[1], got[3], flat, data, precision, 'chi2 ' + what)
    assert_rel(got[0], flat[0], RTOL)
    assert_rel(got[2], flat[2], RTOL)
    dxi, a = fisher_reference.table_jacobian(expect)
    fisher_reference.check(got[4], dxi, a, precision, 'fisher ' + what)
    assert np.array_equal(got[4], got[4].transpose(0, 2, 1))
    gradient = halotab.chi2_grad_batch(theta, data.reshape(tpcf_shape), precision,
                                       modulate_with_cenocc=modulate, assembias=True)
    assert len(gradient) == 4 and same_bits(got[:4], gradient)
    forecast = halotab.fisher_batch(theta, precision, modulate_with_cenocc=modulate,
                                    assembias=True)
    assert same_bits(forecast, (got[0], got[2], got[4]))
    # the value agrees with the forward entry point to parity
    assert_rel(got[1], halotab.chi2_batch(theta, data, precision, modulate_with_cenocc=modulate,
                                          assembias=True)[1], RTOL)


# ---- interpolator ---------------------------------------------------------------------------------

_interp_cases = {}


def get_interp_case(grid, n_prim, n_sec, tpcf_shape, mode, modulate):
    """Interpolator, draws (theta (N_MAX, 7), x) and their reference: the spline-weighted sum of
    the table references."""
    key = (grid, n_prim, n_sec, tpcf_shape, mode, modulate)
    if key not in _interp_cases:
        tables, keys, points = interp_suite.make_tables(grid, n_prim, n_sec, tpcf_shape, mode,
                                                        'two')
        setup = oracle.interpolator_setup(tables, points)
        for seed in range(5, 25):
            theta = reference.stress_draws(tables[0], N_MAX, seed=seed)
            x = interp_suite.make_x(points, setup, N_MAX, 'inside', seed)
            with np.errstate(all='ignore'):
                expect = reference.interp_jacobian_batch(tables, setup, points, theta, x, 10,
                                                         modulate)
            allowance = 1e-10 * (np.abs(expect['dxi']) + expect['dxi_scale'])
            if interp_grad_reference.usable(expect) and reference.rounding_of_centrals(
                    lambda: reference.interp_jacobian_batch(tables, setup, points, theta, x, 10,
                                                            modulate)['dxi'],
                    expect['dxi'], allowance) <= 0.1:
                break
        else:
            raise AssertionError('no seed gives usable draws for %s' % (key, ))
        for array in [theta, x] + list(expect.values()):
            array.setflags(write=False)
        _interp_cases[key] = {'interp': interp_suite.make_interpolator(tables, keys, points),
                              'theta': theta, 'x': x, 'reference': expect, 'modulate': modulate}
    return _interp_cases[key]


INTERP_CASES = [((4, ), 7, 2, (5, ), 'auto', False), ((4, 5), 7, 2, (5, ), 'auto', True),
                ((4, ), 9, 2, (3, 4), 'cross', True), ((4, 5), 9, 2, (5, ), 'cross', False)]


def interp_id(entry):
    grid, n_prim, n_sec, tpcf_shape, mode, modulate = entry
    return '%s-grid%s-%dx%dx%s%s' % (mode, 'x'.join(map(str, grid)), n_prim, n_sec,
                                     'x'.join(map(str, tpcf_shape)),
                                     '-modulate' if modulate else '')


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('entry', INTERP_CASES, ids=interp_id)
def test_interpolator(entry, n_draws, symmetric):
    """Grids of one and two axes over 28-bin auto and 36-bin cross tables with two secondary bins
    (two classes of halo tables interleaved): 7 + D columns.  Prediction, likelihood and Fisher
    matrix against the spline-weighted sum of the table references, with the allowances of
    test_gpu_interp_grad.py and fisher_reference.py."""
    grid, n_prim, n_sec, tpcf_shape, mode, modulate = entry
    case = get_interp_case(*entry)
    interp, n_cols = case['interp'], 7 + len(grid)
    theta, x = case['theta'][:n_draws], case['x'][:n_draws]
    expect = interp_grad_reference.first(case['reference'], n_draws)
    what = '%s n=%d' % (interp_id(entry), n_draws)
    got = interp.predict_batch_grad(theta, x, modulate_with_cenocc=modulate, assembias=True)
    assert got[2].shape == (n_draws, n_cols) and got[3].shape == (n_draws, n_cols) + tpcf_shape
    interp_grad_reference.check(got, expect, what)
    check_clipped_columns(theta, got[2], got[3])
    forward = interp.predict_batch(theta, x, modulate_with_cenocc=modulate, assembias=True)
    assert_rel(got[0], forward[0], RTOL, what + ' ngal against predict_batch')
    assert_rel(got[1], forward[1], RTOL, what + ' xi against predict_batch')

    data, precision = chi2_data(case['reference']['xi'][3].ravel(), symmetric)
    full = interp.chi2_fisher_batch(theta, x, data.reshape(tpcf_shape), precision,
                                    modulate_with_cenocc=modulate, assembias=True)
    assert full[4].shape == (n_draws, n_cols, n_cols)
    interp_suite.check_chi2_values(full[:4], expect, data, precision, 'chi2 ' + what)
    dxi, a = fisher_reference.interp_jacobian(case['reference'])
    fisher_reference.check(full[4], dxi, a, precision, 'fisher ' + what)
    assert np.array_equal(full[4], full[4].transpose(0, 2, 1))
    gradient = interp.chi2_grad_batch(theta, x, data.reshape(tpcf_shape), precision,
                                      modulate_with_cenocc=modulate, assembias=True)
    assert len(gradient) == 4 and same_bits(full[:4], gradient)
    forecast = interp.fisher_batch(theta, x, precision, modulate_with_cenocc=modulate,
                                   assembias=True)
    assert same_bits(forecast, (full[0], full[2], full[4]))


# ---- zero strengths, batch invariance, the entry points -------------------------------------------

@pytest.mark.parametrize('case', [(9, 2, (5, ), 'auto'), (17, 2, (5, ), 'cross')], ids=case_id)
def test_zero_strengths_agree_with_the_plain_gradient(case):
    """With both strengths zero, ngal, xi and the first five columns are the plain gradient's
    within the parity bar (whether to the bit is reported, not asserted); the two strength
    columns are not zero."""
    n_prim, n_sec, tpcf_shape, mode = case
    table, halotab = get_table(*case)
    theta = np.array(get_reference(n_prim, n_sec, tpcf_shape, mode, False, 10)[0])
    theta[:, 5:] = 0.0
    plain_reference = grad_reference.jacobian_batch(table, theta[:, :5])
    plain = halotab.predict_batch_grad(theta[:, :5])
    got = halotab.predict_batch_grad(theta, assembias=True)
    assert_rel(got[0], plain[0], RTOL)
    assert_rel(got[1], plain[1], RTOL)
    assert_rel(got[2][:, :5], plain[2], RTOL)
    # (each side within the allowance of the plain reference: their difference within twice it)
    table_suite.check_derivatives(got[2][:, :5], got[3][:, :5], plain_reference,
                                  'zero strengths ' + case_id(case))
    print('zero strengths %s: first five columns bit-equal to the plain gradient: %s' % (
        case_id(case), same_bits((got[0], got[1], got[2][:, :5], got[3][:, :5]), plain)))
    # all seven columns against the decorated reference at zero strengths, whose two strength
    # columns are not zero (A_sat's is where a draw has no satellites at all)
    expect = reference.jacobian_batch(table, theta)
    table_suite.check_derivatives(got[2], got[3], expect, 'zero strengths, seven columns')
    assert np.all(np.any(expect[3][:, 5] != 0.0, axis=-1))
    assert np.sum(np.any(expect[3][:, 6] != 0.0, axis=-1)) >= N_MAX - 4
    assert np.array_equal(got[3][:, 5:] != 0.0, expect[3][:, 5:] != 0.0)


def device_grad(halotab, theta, flags=0):
    device = halotab.to_device()
    n, n_r = len(theta), device.n_r
    return device_call(device, 'tc_predict_grad_assembias_batch_device',
                       [theta, 7, n, 10, flags], [n, (n, n_r), (n, 7), (n, 7, n_r)])


def device_chi2_grad(halotab, theta, data, precision, fisher, flags=0):
    """tc_chi2_grad_assembias_batch_device with its trailing fisher, or NULL in its place."""
    from tabcorr_amd import _lib
    device = halotab.to_device()
    n = len(theta)
    data = _lib.contiguous(np.ravel(data))
    precision = _lib.contiguous(precision)
    arguments = [theta, 7, n, 10, flags, _lib.as_double_p(data), _lib.as_double_p(precision)]
    shapes = [n, n, (n, 7), (n, 7)]
    if fisher:
        return device_call(device, 'tc_chi2_grad_assembias_batch_device', arguments,
                           shapes + [(n, 7, 7)])
    # (None after the four outputs cannot be spelled through device_call: the outputs come last)
    import ctypes
    lib = device.lib
    inputs = [np.ascontiguousarray(theta)]
    outputs = [np.empty(shape) for shape in shapes]
    pointers = []
    try:
        for array in inputs + outputs:
            ptr = ctypes.c_void_p()
            _lib.check(lib.tc_device_malloc(ctypes.byref(ptr), max(array.nbytes, 8)))
            pointers.append(ptr)
        with device.lock:
            _lib.check(lib.tc_memcpy_h2d(pointers[0], inputs[0].ctypes.data_as(ctypes.c_void_p),
                                         inputs[0].nbytes))
            _lib.check(lib.tc_chi2_grad_assembias_batch_device(
                device.handle, pointers[0], *arguments[1:], *pointers[1:], None))
            _lib.check(lib.tc_table_synchronize(device.handle))
            for array, ptr in zip(outputs, pointers[1:]):
                _lib.check(lib.tc_memcpy_d2h(array.ctypes.data_as(ctypes.c_void_p), ptr,
                                             array.nbytes))
    finally:
        for ptr in pointers:
            lib.tc_device_free(ptr)
    return outputs


@pytest.mark.parametrize('case', [(9, 2, (5, ), 'auto'), (6, 3, (3, 4), 'auto'),
                                  (17, 2, (5, ), 'cross')], ids=case_id)
def test_batch_invariance_and_device_entries(case):
    """The kernels have one form: a draw's bits are the same alone, as draw 16 of 17 and in 35,
    and through the host-array and the device-pointer entry points -- for the prediction, the
    likelihood and the Fisher matrix, and with modulate_with_cenocc through the device flags."""
    from tabcorr_amd import _lib
    n_prim, n_sec, tpcf_shape, mode = case
    _, halotab = get_table(*case)
    theta, expect, _ = get_reference(n_prim, n_sec, tpcf_shape, mode, False, 10)
    data, precision = chi2_data(expect[1][3].ravel(), False)
    full = halotab.predict_batch_grad(theta, assembias=True)
    full_chi2 = halotab.chi2_fisher_batch(theta, data.reshape(tpcf_shape), precision,
                                          assembias=True)
    assert all(np.all(np.isfinite(a)) for a in full + full_chi2)

    def predict(draws):
        return halotab.predict_batch_grad(draws, assembias=True)

    def likelihood(draws):
        return halotab.chi2_fisher_batch(draws, data.reshape(tpcf_shape), precision,
                                         assembias=True)

    for call, everything in ((predict, full), (likelihood, full_chi2)):
        assert same_bits(call(theta[D:D + 1]), [b[D:D + 1] for b in everything])
        assert same_bits(call(theta[:D + 1]), [b[:D + 1] for b in everything])
    for n in DRAW_COUNTS:
        assert same_bits(device_grad(halotab, theta[:n]), [b[:n] for b in full], reshape=True)
        assert same_bits(device_chi2_grad(halotab, theta[:n], data, precision, True),
                         [b[:n] for b in full_chi2])
        assert same_bits(device_chi2_grad(halotab, theta[:n], data, precision, False),
                         [b[:n] for b in full_chi2[:4]])
    host = halotab.predict_batch_grad(theta[:D + 1], modulate_with_cenocc=True, assembias=True)
    assert same_bits(device_grad(halotab, theta[:D + 1], _lib.FLAG_MODULATE_WITH_CENOCC), host,
                     reshape=True)
    assert not np.array_equal(host[1], full[1][:D + 1])


def test_interpolator_batch_invariance_and_device_entries():
    from tabcorr_amd import _lib
    entry = ((4, 5), 7, 2, (5, ), 'auto', True)
    case = get_interp_case(*entry)
    interp, theta, x = case['interp'], case['theta'], case['x']
    data, precision = chi2_data(case['reference']['xi'][3].ravel(), False)
    full = interp.predict_batch_grad(theta, x, modulate_with_cenocc=True, assembias=True)
    full_chi2 = interp.chi2_fisher_batch(theta, x, data, precision, modulate_with_cenocc=True,
                                         assembias=True)
    for rows in (slice(D, D + 1), slice(0, D + 1)):
        assert same_bits(interp.predict_batch_grad(theta[rows], x[rows],
                                                   modulate_with_cenocc=True, assembias=True),
                         [b[rows] for b in full])
        assert same_bits(interp.chi2_fisher_batch(theta[rows], x[rows], data, precision,
                                                  modulate_with_cenocc=True, assembias=True),
                         [b[rows] for b in full_chi2])
    device = interp.to_device()
    n_r, n_cols = device.tables[0].n_r, 9
    flags = _lib.FLAG_MODULATE_WITH_CENOCC
    for n in DRAW_COUNTS:
        arguments = [theta[:n], 7, x[:n], n, 10, flags]
        got = device_call(device, 'tc_interp_predict_grad_assembias_batch_device', arguments,
                          [n, (n, n_r), (n, n_cols), (n, n_cols, n_r)], 'tc_interp_synchronize')
        assert same_bits(got, [b[:n] for b in full], reshape=True)
        got = device_call(device, 'tc_interp_chi2_grad_assembias_batch_device',
                          arguments + [_lib.as_double_p(_lib.contiguous(data)),
                                       _lib.as_double_p(_lib.contiguous(precision))],
                          [n, n, (n, n_cols), (n, n_cols), (n, n_cols, n_cols)],
                          'tc_interp_synchronize')
        assert same_bits(got, [b[:n] for b in full_chi2])


# ---- limits -----------------------------------------------------------------------------------------
# The decorated budget of grad_auto_kernel (csrc/grad.h), in rows of D doubles: four rows per
# central bin, seven per satellite bin, one row of zeros, eight rows of totals.

def auto_lds_bytes(n_bins, n_central):
    return (4 * n_central + 7 * (n_bins - n_central) + 1 + 8) * D * 8


def test_lds_limit_auto():
    """n_sec = 2, three r bins: the table with the most bins that the decorated gradient serves
    matches the reference; one more primary bin is refused naming LDS, and the handle then serves
    predict_batch and the plain predict_batch_grad."""
    from tabcorr_amd import TabCorr
    n_prim = largest(lambda n: auto_lds_bytes(4 * n, 2 * n) <= LDS_LIMIT)
    case = (n_prim, 2, (3, ), 'auto')
    _, halotab = get_table(*case)
    theta, expect, values = get_reference(*case, False, 10, n_draws=D + 1)
    check_gradient(halotab, theta, expect, values, 10, False, (3, ),
                   'LDS limit auto %d bins' % (4 * n_prim))
    table = synthetic.synthetic_table(n_prim + 1, 2, (3, ), 'auto', seed=3)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                  table['attrs'])
    draws = reference.stress_draws(table, 5, seed=5)
    with pytest.raises(NotImplementedError, match='LDS'):
        halotab.predict_batch_grad(draws, assembias=True)
    check_still_serves(halotab, table)
    plain = grad_reference.jacobian_batch(table, draws[:, :5])
    got = halotab.predict_batch_grad(draws[:, :5])
    assert_rel(got[0], plain[0], RTOL)
    table_suite.check_derivatives(got[2], got[3], plain, 'plain gradient after the refusal')


def test_unsupported_requests_leave_the_handle_usable():
    from tabcorr_amd import TabCorr, _lib
    case = (9, 2, (5, ), 'auto')
    table, halotab = get_table(*case)
    theta, expect, values = get_reference(*case, False, 10)
    single = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                 table['attrs'], compute_dtype='float32')
    with pytest.raises(NotImplementedError, match='float64'):
        single.predict_batch_grad(theta[:5], assembias=True)
    check_still_serves(single, table, 1e-5)     # (the float32 path's stated tolerance)

    device = halotab.to_device()
    n, n_r = 5, device.n_r
    draws = np.ascontiguousarray(theta[:n])
    outputs = [np.empty(n * 2), np.empty(n * 3 * n_r), np.empty(n * 14), np.empty(n * 21 * n_r)]
    for flags in (_lib.FLAG_SEPARATE_GAL_TYPE, _lib.FLAG_LEAUTHAUD11, _lib.FLAG_ASSEMBIAS,
                  _lib.FLAG_MODULATE_WITH_CENOCC | _lib.FLAG_SEPARATE_GAL_TYPE):
        with device.lock:
            status = device.lib.tc_predict_grad_assembias_batch(
                device.handle, _lib.as_double_p(draws), 7, n, 10, flags,
                *[_lib.as_double_p(a) for a in outputs])
        assert status == _lib.TC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            _lib.check(status)
        with device.lock:
            status = device.lib.tc_chi2_grad_assembias_batch(
                device.handle, _lib.as_double_p(draws), 7, n, 10, flags,
                _lib.as_double_p(np.zeros(n_r)), _lib.as_double_p(np.eye(n_r)),
                *[_lib.as_double_p(a) for a in outputs], None)
        assert status == _lib.TC_ERR_UNSUPPORTED
        check_still_serves(halotab, table)
    # five columns are not the decorated entry's
    with device.lock:
        status = device.lib.tc_predict_grad_assembias_batch(
            device.handle, _lib.as_double_p(draws), 5, n, 10, 0,
            *[_lib.as_double_p(a) for a in outputs])
    assert status == _lib.TC_ERR_INVALID
    check_gradient(halotab, theta, expect, values, 10, False, (5, ), 'after the refused calls')


def test_interpolator_refuses_other_flags():
    from tabcorr_amd import _lib
    case = get_interp_case((4, ), 7, 2, (5, ), 'auto', False)
    interp = case['interp']
    device = interp.to_device()
    n, n_r = 3, device.tables[0].n_r
    theta = np.ascontiguousarray(case['theta'][:n])
    x = np.ascontiguousarray(case['x'][:n])
    outputs = [np.empty(n), np.empty(n * n_r), np.empty(n * 8), np.empty(n * 8 * n_r)]
    for flags in (_lib.FLAG_SEPARATE_GAL_TYPE, _lib.FLAG_LEAUTHAUD11):
        with device.lock:
            status = device.lib.tc_interp_predict_grad_assembias_batch(
                device.handle, _lib.as_double_p(theta), 7, _lib.as_double_p(x), n, 10, flags,
                *[_lib.as_double_p(a) for a in outputs])
        assert status == _lib.TC_ERR_UNSUPPORTED
    got = interp.predict_batch_grad(theta, x, assembias=True)
    interp_grad_reference.check(got, interp_grad_reference.first(case['reference'], n),
                                'after the refused calls')


# ---- model objects ----------------------------------------------------------------------------------

def decorated_model(theta, modulate, extra=None):
    from tabcorr_amd import Zheng07Model
    from tabcorr_amd.models import ZHENG07_ASSEMBIAS_KEYS
    model = Zheng07Model(redshift=0.0, modulate_with_cenocc=modulate,
                         sec_haloprop_key='halo_nfw_conc')
    for key, value in zip(ZHENG07_ASSEMBIAS_KEYS, theta):
        model.param_dict[key] = value
    model.param_dict.update(extra or {})
    return model


def test_model_object_calls():
    """predict_grad(model, assembias=True) and fisher(model, P, assembias=True) return the bits of
    their row of the batch, keyed by the seven names -- of a table and of an interpolator."""
    from tabcorr_amd.models import ZHENG07_ASSEMBIAS_KEYS
    case = (9, 2, (5, ), 'auto')
    _, halotab = get_table(*case)
    theta, expect, _ = get_reference(*case, True, 10)
    _, precision = chi2_data(expect[1][3].ravel(), False)
    row = 2
    model = decorated_model(theta[row], True)
    batch = halotab.predict_batch_grad(theta, modulate_with_cenocc=True, assembias=True)
    one = halotab.predict_grad(model, assembias=True)
    assert isinstance(one[0], float) and one[0] == batch[0][row]
    assert np.array_equal(one[1], batch[1][row])
    assert list(one[2]) == list(ZHENG07_ASSEMBIAS_KEYS) == list(one[3])
    for k, key in enumerate(ZHENG07_ASSEMBIAS_KEYS):
        assert one[2][key] == batch[2][row, k] and np.array_equal(one[3][key], batch[3][row, k])
    forecast = halotab.fisher_batch(theta, precision, modulate_with_cenocc=True, assembias=True)
    ngal, dngal, fisher = halotab.fisher(model, precision, assembias=True)
    assert ngal == forecast[0][row] and np.array_equal(fisher, forecast[2][row])
    assert [dngal[key] for key in ZHENG07_ASSEMBIAS_KEYS] == list(forecast[1][row])
    # without the keyword a decorated model stays refused
    with pytest.raises(NotImplementedError, match='plain Zheng07'):
        halotab.predict_grad(model)

    entry = ((4, ), 7, 2, (5, ), 'auto', False)
    interp_case = get_interp_case(*entry)
    interp, theta, x = interp_case['interp'], interp_case['theta'], interp_case['x']
    _, precision = chi2_data(interp_case['reference']['xi'][3].ravel(), False)
    model = decorated_model(theta[row], False, {interp.keys[0]: x[row, 0]})
    keys = tuple(ZHENG07_ASSEMBIAS_KEYS) + tuple(interp.keys)
    batch = interp.predict_batch_grad(theta, x, assembias=True)
    one = interp.predict_grad(model, assembias=True)
    assert one[0] == batch[0][row] and np.array_equal(one[1], batch[1][row])
    assert tuple(one[2]) == keys == tuple(one[3])
    for k, key in enumerate(keys):
        assert one[2][key] == batch[2][row, k] and np.array_equal(one[3][key], batch[3][row, k])
    forecast = interp.fisher_batch(theta, x, precision, assembias=True)
    ngal, dngal, fisher = interp.fisher(model, precision, assembias=True)
    assert ngal == forecast[0][row] and np.array_equal(fisher, forecast[2][row])
    assert [dngal[key] for key in keys] == list(forecast[1][row])
