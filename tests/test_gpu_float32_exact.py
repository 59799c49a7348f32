"""The float32 kernels -- contract_quad_f32_kernel<U, INTERP> and contract_f32_kernel<INTERP> --
held to float64 precision on inputs for which float32 arithmetic is exact (tests/exact_tables.py:
n_h x occupation, matrix entries and spline weights are short dyadic numbers and every partial
sum stays below 2^24 units).  The 1e-5 of the other float32 tests cannot see a 4 x 4 matrix block
that is dropped, doubled or read from the wrong place on the synthetic tables
(tests/test_exact_tables_cpu.py measures it: 15 to 44 % of the blocks); here every entry carries
at least one unit, and one missing entry exceeds the allowance.  Needs an MI355X.

Tolerances, per (draw, r), with sum |terms| = sum_k |w_k| sum_ij |pre_ij n_i n_j T_ijr|:
occupation route (tables, `predict(ndarray)`): 4 eps64 sum |terms| / norm -- the one division
    and the oracle's own roundings; whether the totals are bit-equal is printed, not asserted.
theta route (tables and interpolators, Zheng07 draws with exact 0 / 1 occupations):
    4e-12 sum |terms| / norm -- the 1e-12 the float32 tests grant the device's float64
    occupations, times 4 for a ratio of two quadratic forms in them.  ngal at 1e-12.

Paths that are not exactly dyadic (read from the kernels and the table fills):
- none in fill_quad_table_f32 and the float32 table of contract_f32_kernel (table.cpp): the pair
  prefactor 1 or 2 times an integer entry, cast to float; none in either kernel's products.
- the interpolators' coefficient (float)(spline weight / pair-weight norm): the weight comes from
  the device's float64 spline matrices, a dyadic number to ~1e-15, and the norm from the device's
  float64 occupations, a power of two to ~1e-15; the cast to float removes both departures from
  every non-zero weight.  A weight that should be exactly zero (x on a node) arrives as ~1e-16
  instead: its table adds ~1e-16 sum |terms| / norm, inside the theta route's 4e-12.
- the oracle itself evaluates the splines from an inverted matrix (weights to 2e-15 on 4 nodes,
  2e-14 on 5): also inside 4e-12.

Every test prints `form: ...` lines with the largest error in units of its allowance.
"""

import ctypes

import numpy as np
import pytest

import exact_tables as ex
from util import assert_rel, load_golden, table_from_golden

pytestmark = pytest.mark.gpu

QUAD_WAVES_PER_BLOCK = 4        # (kernel_args.h: kQuadWavesPerBlock)


def make(table, dtype):
    from tabcorr_amd import TabCorr
    return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                               table['attrs'], compute_dtype=dtype)


def set_option(halotab, key, value):
    from tabcorr_amd import _lib
    _lib.check(_lib.load().tc_table_set_option(halotab.to_device().handle, key.encode(), value))


def last_launch(halotab):
    """(workgroups, waves per workgroup, slabs, LDS bytes) of the handle's last contraction."""
    from tabcorr_amd import _lib
    launch = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.load().tc_table_last_launch(halotab.to_device().handle,
                                                *[ctypes.byref(v) for v in launch]))
    return tuple(v.value for v in launch)


def assert_quad_kernel(halotab):
    launch = last_launch(halotab)
    assert launch[1] == QUAD_WAVES_PER_BLOCK and launch[2] > 0, 'not contract_quad*: %s' % (launch, )


def assert_contract_kernel(halotab):
    """(launch.hip, interp.cpp: the contract_*_kernel launches ask for LDS and count groups; the
    quadratic-form path of tables reports no LDS, a one-launch form no slabs)"""
    launch = last_launch(halotab)
    assert launch[2] > 0 and launch[3] > 0, 'not contract_f32 / contract_mfma: %s' % (launch, )


def in_allowance(got, expect, allowance, factor, what):
    """|got - expect| <= factor * allowance elementwise; the largest ratio."""
    got = np.reshape(np.asarray(got, dtype=np.float64), np.shape(expect))
    assert np.all(np.isfinite(got)), what
    error = np.abs(got - expect)
    bound = factor * allowance
    worst = float(np.max(error / np.maximum(bound, 1e-300)))
    assert np.all(error <= bound), '%s: %.3g of the allowance at %s' % (
        what, worst, np.unravel_index(np.argmax(error / np.maximum(bound, 1e-300)), error.shape))
    return worst


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v, dtype=np.float64) for v in (a, b))
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


@pytest.fixture(scope='module')
def oracle_of():
    """The oracle's (ngal, xi) of a cached case, total and separated, computed once."""
    cache = {}

    def values(case, separate, route):
        key = (id(case), separate)
        if key not in cache:
            cache[key] = (ex.oracle_occupation if route == 'occupation' else ex.oracle_theta)(
                case, separate)
        return cache[key]
    return values


def check_prediction(form, what, case, n, got, expect, factor):
    """A device result (ngal, xi), total or separated, of the first n draws against the
    oracle's `expect`; returns (largest error / allowance, totals bit-equal or None)."""
    ngal, xi = got
    if isinstance(xi, dict):
        assert sorted(xi) == sorted(expect[1])
        worst = 0.0
        for key in expect[0]:
            assert_rel(ngal[key], expect[0][key][:n], 1e-12, what + ' ngal ' + key)
        for key in xi:
            worst = max(worst, in_allowance(
                xi[key].reshape(n, -1), expect[1][key][:n].reshape(n, -1),
                case.allowance[key][:n], factor, '%s %s %s' % (form, what, key)))
        return worst, None
    assert xi.shape == (n, ) + case.tpcf_shape
    assert_rel(ngal, expect[0][:n], 1e-12, what + ' ngal')
    worst = in_allowance(xi.reshape(n, -1), expect[1][:n].reshape(n, -1),
                         case.allowance['total'][:n], factor, '%s %s total' % (form, what))
    return worst, same_bits(xi, expect[1][:n])


OCCUPATION_CASES = ([spec + ('auto', 'quad') for spec in ex.QUAD_CASES] +
                    [spec + ('contract', ) for spec in ex.CONTRACT_CASES])


@pytest.mark.parametrize('spec', OCCUPATION_CASES, ids=ex.case_id)
def test_tables_occupation_route(spec, oracle_of):
    """contract_quad_f32_kernel<U, false> (mode auto up to 304 bins) and
    contract_f32_kernel<false> (mode cross, mode auto beyond) through `predict(ndarray)`: integer
    occupations, 1, 63, 64, 65 and 130 draws, the total prediction and every component; then the
    same table in float64 (contract_quad_kernel, and contract_mfma_kernel in mode cross -- the
    occupation seam always takes the three-kernel path, option fused = 0 changes no bit) at the
    same tolerance, its totals bit-equal to the float32 ones."""
    kernel = spec[-1]
    case = ex.cached('occupation', *spec[:-1], ex.N_DRAWS)
    eps4 = 4 * ex.EPS64
    halotab = make(case.table, 'float32')
    form = 'quad f32' if kernel == 'quad' else 'contract_f32'
    worst, equal, totals = 0.0, True, {}
    for n in ex.DRAW_COUNTS:
        for separate in (False, True):
            got = halotab.predict(case.occupation[:n], separate_gal_type=separate)
            (assert_quad_kernel if kernel == 'quad' else assert_contract_kernel)(halotab)
            ratio, bits = check_prediction(form, '%d draws' % n, case, n, got,
                                           oracle_of(case, separate, 'occupation'), eps4)
            worst = max(worst, ratio)
            if not separate:
                equal, totals[n] = equal and bits, got[1]
    print('form: %s %s: largest error %.3f of 4 eps64 sum |terms| / norm; totals bit-equal to the '
          'oracle: %s' % (form, ex.case_id(spec), worst, equal))
    # float64 beside it
    halotab64 = make(case.table, 'float64')
    mode = case.mode
    worst64, equal64 = 0.0, True
    for n in (65, ex.N_DRAWS):
        for separate in (False, True):
            got = halotab64.predict(case.occupation[:n], separate_gal_type=separate)
            if mode == 'auto':
                assert_quad_kernel(halotab64)
            else:
                assert_contract_kernel(halotab64)
            ratio, bits = check_prediction('float64', '%d draws' % n, case, n, got,
                                           oracle_of(case, separate, 'occupation'), eps4)
            worst64 = max(worst64, ratio)
            if not separate:
                equal64 = equal64 and bits
                assert same_bits(got[1], totals[n]), \
                    'float32 and float64 totals differ (%d draws)' % n
    set_option(halotab64, 'fused', 0)
    again = halotab64.predict(case.occupation, separate_gal_type=False)
    assert same_bits(again[1], totals[ex.N_DRAWS])
    print('form: %s %s: largest error %.3f of the allowance; totals bit-equal to the oracle: %s, '
          'to float32: True' % ('contract_quad (f64)' if mode == 'auto' else 'contract_mfma (f64)',
                                ex.case_id(spec), worst64, equal64))


@pytest.mark.parametrize('spec', ex.SWEEP_CASES, ids=ex.case_id)
def test_same_bits_whatever_the_schedule(spec, oracle_of):
    """Exact sums do not depend on the order: every schedule of contract_quad_f32_kernel --
    workgroup-level merging on and off, 1 to 3 waves per SIMD, every order of
    build_quad_schedule (0 ... 5; those that do not apply to one table fall back to another, as
    hostmath.cpp describes) -- returns the default's bits.  The 50-bin case takes 2560 draws, so
    that the number of waves changes the shares; the other one has two r tiles and is run
    separated by galaxy type too."""
    n_prim, n_sec, tpcf_shape, n_draws = spec
    case = ex.cached('occupation', n_prim, n_sec, tpcf_shape, 'auto', n_draws, 0, False)
    halotab = make(case.table, 'float32')
    separations = (False, ) if n_draws > ex.N_DRAWS else (False, True)

    def run(separate):
        got = halotab.predict(case.occupation, separate_gal_type=separate)
        assert_quad_kernel(halotab)
        xi = got[1] if separate else {'total': got[1]}
        return {key: np.array(value) for key, value in xi.items()}, last_launch(halotab)[:3]
    default = {separate: run(separate) for separate in separations}
    worst = in_allowance(default[False][0]['total'].reshape(n_draws, -1), case.expect['total'],
                         case.allowance['total'], 4 * ex.EPS64, 'default schedule')
    if n_draws == ex.N_DRAWS:       # (the same draws: against the oracle itself as well)
        sample = ex.cached('occupation', n_prim, n_sec, tpcf_shape, 'auto', ex.N_DRAWS)
        assert np.array_equal(sample.occupation, case.occupation)
        in_allowance(default[False][0]['total'].reshape(n_draws, -1),
                     oracle_of(sample, False, 'occupation')[1].reshape(n_draws, -1),
                     case.allowance['total'], 4 * ex.EPS64, 'default schedule, oracle')
    launches = {}
    defaults = {'quad_merge': 1, 'quad_waves': 3, 'quad_order': -1}     # (internal.h: float32)
    for key, values in (('quad_merge', (0, 1)), ('quad_waves', (1, 2, 3)),
                        ('quad_order', (0, 1, 2, 3, 4, 5))):
        for value in values:
            set_option(halotab, key, value)
            for separate in separations:
                got, launch = run(separate)
                launches[key, value, separate] = launch
                for name, xi in got.items():
                    assert same_bits(xi, default[separate][0][name]), \
                        '%s = %d changes bits of %s' % (key, value, name)
        set_option(halotab, key, defaults[key])
    again, launch = run(False)
    assert same_bits(again['total'], default[False][0]['total']) and launch == default[False][1]
    distinct = {launch for (key, _, separate), launch in launches.items() if not separate}
    print('form: quad f32 sweep %s: default within %.3f of the allowance; %d distinct '
          '(workgroups, waves, slabs) among the schedules: %s'
          % (ex.case_id(spec), worst, len(distinct), sorted(distinct)))
    assert len(distinct) > 1, 'the sweep changed no schedule'
    if n_draws > ex.N_DRAWS:
        assert len({launches['quad_waves', value, False] for value in (1, 2, 3)}) > 1


def make_interpolator(case, dtype):
    from tabcorr_amd import Interpolator
    halotabs = [make(table, dtype) for table in case.tables]
    return halotabs, Interpolator(halotabs, {key: case.points[:, d]
                                             for d, key in enumerate(case.keys)})


THETA_FACTOR = 4e-12


@pytest.mark.parametrize('spec', ex.INTERP_CASES, ids=ex.case_id)
def test_interpolators_theta_route(spec, oracle_of):
    """contract_quad_f32_kernel<U, true> (mode auto) and contract_f32_kernel<true> (mode cross) on
    grids (4, ), (4, 4) and (5, ) with an integer matrix of its own per node and one or two
    classes of halo tables: 3, 64 and 130 draws, x on nodes and mid-points in turn, the total
    prediction and every component."""
    case = ex.cached('theta', *spec, ex.N_DRAWS)
    halotabs, interpolator = make_interpolator(case, 'float32')
    form = 'quad f32 INTERP' if case.mode == 'auto' else 'contract_f32 INTERP'
    worst, exact_worst, equal = 0.0, 0.0, True
    for n in ex.INTERP_DRAW_COUNTS:
        for separate in (False, True):
            got = interpolator.predict_batch(case.theta[:n], case.x[:n],
                                             separate_gal_type=separate)
            (assert_quad_kernel if case.mode == 'auto' else assert_contract_kernel)(halotabs[0])
            ratio, _ = check_prediction(form, '%d draws' % n, case, n, got,
                                        oracle_of(case, separate, 'theta'), THETA_FACTOR)
            worst = max(worst, ratio)
            xi = got[1] if separate else {'total': got[1]}
            for key, value in xi.items():   # (against the exact rational result, for the record)
                error = np.abs(value.reshape(n, -1) - case.expect[key][:n])
                exact_worst = max(exact_worst, float(np.max(
                    error / np.maximum(ex.EPS64 * case.allowance[key][:n], 1e-300))))
            if not separate:
                equal = equal and same_bits(got[1].reshape(n, -1), case.expect['total'][:n])
    print('form: %s %s: largest error %.3g of 4e-12 sum |terms| / norm against the oracle, '
          '%.3g eps64 sum |terms| / norm against the exact result; totals bit-equal to the exact '
          'result: %s' % (form, ex.case_id(spec), worst, exact_worst, equal))


@pytest.mark.parametrize('spec', ex.THETA_TABLE_CASES, ids=ex.case_id)
def test_tables_theta_route(spec, oracle_of):
    """One table from Zheng07 draws: the occupation kernel writes the float copy of the densities
    that the float32 kernels read (the occupation route goes through occ_from_array_kernel)."""
    case = ex.cached('theta', *spec, ex.N_DRAWS)
    worst, equal = {}, {}
    for dtype in ('float32', 'float64'):
        halotab = make(case.table, dtype)
        if dtype == 'float64':
            # the three-kernel path (contract_quad / contract_mfma), for three draws too: neither
            # the one-launch forms nor the un-batched kernel (tests/golden/make_quad_walk_parent.py)
            set_option(halotab, 'fused', 0)
            set_option(halotab, 'single_draw', 0)
        worst[dtype], equal[dtype] = 0.0, True
        for n in ex.INTERP_DRAW_COUNTS:
            for separate in (False, True):
                got = halotab.predict_batch(case.theta[:n], separate_gal_type=separate)
                (assert_quad_kernel if case.mode == 'auto' else assert_contract_kernel)(halotab)
                ratio, _ = check_prediction(dtype, '%d draws' % n, case, n, got,
                                            oracle_of(case, separate, 'theta'), THETA_FACTOR)
                worst[dtype] = max(worst[dtype], ratio)
                if not separate:
                    equal[dtype] = equal[dtype] and same_bits(got[1].reshape(n, -1),
                                                              case.expect['total'][:n])
    print('form: %s theta route %s: largest error %.3g (float32), %.3g (float64) of 4e-12 '
          'sum |terms| / norm; totals bit-equal to the exact result: %s, %s'
          % ('quad f32' if case.mode == 'auto' else 'contract_f32', ex.case_id(spec),
             worst['float32'], worst['float64'], equal['float32'], equal['float64']))


def integer_likelihood(n_r, seed):
    """An integer data vector and an integer (asymmetric) precision matrix."""
    rng = np.random.default_rng([seed, n_r])
    data = rng.integers(-2, 3, size=n_r).astype(np.float64)
    precision = rng.integers(-2, 3, size=(n_r, n_r)).astype(np.float64)
    precision += np.diag(np.full(n_r, 5.0))
    return data, precision


@pytest.mark.parametrize('spec', [((), 50, (19, ), 'auto', 1), ((4, ), 14, (12, ), 'auto', 1)],
                         ids=ex.case_id)
def test_chi2(spec, oracle_of):
    """`chi2_batch` of one float32 table and one float32 interpolator with integer data and an
    integer precision matrix, against chi2 of the oracle's xi at the bound the suite derives
    for it (test_gpu_call_paths.check_against_oracle): first order in the tolerance of xi,
    |chi2 - expected| <= sum_j |(P d)_j + (P^T d)_j| tol_j with d = xi - data and tol_j the theta
    route's 4e-12 sum |terms| / norm."""
    case = ex.cached('theta', *spec, ex.N_DRAWS)
    n_r = int(np.prod(case.tpcf_shape))
    data, precision = integer_likelihood(n_r, 3)
    if case.grid:
        halotabs, interpolator = make_interpolator(case, 'float32')
        ngal, chi2 = interpolator.chi2_batch(case.theta, case.x, data, precision)
        assert_quad_kernel(halotabs[0])
    else:
        halotab = make(case.table, 'float32')
        ngal, chi2 = halotab.chi2_batch(case.theta, data, precision)
        assert_quad_kernel(halotab)
    expect_ngal, expect_xi = oracle_of(case, False, 'theta')
    assert_rel(ngal, expect_ngal, 1e-12, 'ngal')
    delta = expect_xi.reshape(len(case.theta), -1) - data
    slope = np.abs(delta @ precision.T + delta @ precision)
    bound = np.sum(slope * THETA_FACTOR * case.allowance['total'], axis=-1)
    expect = np.einsum('bi,ij,bj->b', delta, precision, delta)
    worst = float(np.max(np.abs(chi2 - expect) / bound))
    print('form: quad f32%s chi2 %s: largest error %.3g of the bound inherited from xi'
          % (' INTERP' if case.grid else '', ex.case_id(spec), worst))
    assert worst <= 1.0


def test_realistic_table_per_element_bound():
    """bolplanck_wp (60 bins, 19 r_p bins, wp spanning orders of magnitude across r) as a float32
    table, 64 prior draws, every (draw, r) against the oracle at k 2^-24 sum |terms| / norm -- per
    element, not the array's maximum.

    k counts the float32 roundings on the longest path of a term T_ijr n_i n_j through
    contract_quad_f32_kernel, from the kernel and the schedule:
      3   the inputs: the table entry, n_i and n_j cast to float;
      8   per matrix unit of the wave: v_mfma_f32_16x16x4_f32 adds four products to the chain D,
          counted as a rounding of each product and of each addition;
      4   per unit for the outer factor: a block row ends with four fmaf F += D e per sum, and a
          wave has at most as many block rows as units;
      11  the workgroup's merge adds at most 12 LDS slots (launch.hip: merge_quad_schedule(...,
          12, ...)); the slabs are then added in float64.
    A wave's sums F run through all its units of an output group, at most `units_max` of
    tc_debug_quad_schedule: 64 draws are one tile, two r tiles of 10 values and 120 units of the
    unpadded 15-row triangle (30 centrals do not fill 4-bin blocks) make 240 units, 8 per wave
    on any device with at least 30 wave slots.  So k = 3 + 12 * 8 + 11 = 110; the count is an
    upper bound (the hardware may round less often), derived, not tuned."""
    from tabcorr_amd import _lib, synthetic
    from oracle import tabcorr_oracle as oracle
    table = table_from_golden(load_golden('bolplanck_wp'))
    central = oracle.is_centrals(table['gal_type'])
    n_bins, n_central = len(central), int(central.sum())
    assert (n_bins, n_central, table['tpcf_shape']) == (60, 30, (19, ))
    sizes = [ctypes.c_int() for _ in range(3)]
    units = [ctypes.c_int64(), ctypes.c_int64()]
    _lib.check(_lib.load().tc_debug_quad_schedule(
        n_bins, n_central, 0, 1, 2, 1, 0, 256 * 4 * 3, 8, 0,
        *[ctypes.byref(v) for v in sizes + units]))
    units_max = units[1].value
    k = 3 + 12 * units_max + 11
    print('schedule: %d waves, %d runs, %d slabs, %d to %d units per wave; k = %d'
          % tuple([v.value for v in sizes] + [units[0].value, units_max, k]))
    assert units_max == 8 and k == 110
    theta = synthetic.zheng07_draws(64, seed=77)
    halotab = make(table, 'float32')
    ngal, xi = halotab.predict_batch(theta)
    assert_quad_kernel(halotab)
    launch = last_launch(halotab)
    assert launch[0] * QUAD_WAVES_PER_BLOCK >= sizes[0].value > (launch[0] - 1) * QUAD_WAVES_PER_BLOCK
    expect_ngal, expect_xi = oracle.predict_zheng07_batch(table, theta)
    assert_rel(ngal, expect_ngal, 1e-12, 'ngal')
    index_1, index_2, prefactor = oracle.pair_indices(n_bins)
    allowance = np.empty_like(expect_xi)
    for d, t in enumerate(theta):
        density = oracle.mean_occupation(table, oracle.Zheng07(t)) * table['gal_type']['n_h']
        weights = prefactor * density[index_1] * density[index_2]
        allowance[d] = np.abs(table['tpcf_matrix']) @ weights / np.sum(weights)
    worst = in_allowance(xi, expect_xi, allowance, k * 2.0**-24, 'bolplanck_wp float32')
    cancellation = np.max(allowance / np.abs(expect_xi))
    print('form: quad f32 bolplanck_wp: k = %d, largest error %.4f of k 2^-24 sum |terms| / norm '
          '(sum |terms| / |xi| up to %.1f; |xi| from %.3g to %.3g)'
          % (k, worst, cancellation, np.min(np.abs(expect_xi)), np.max(np.abs(expect_xi))))
