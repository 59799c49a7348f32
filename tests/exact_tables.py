"""Tables on which float32 arithmetic is exact, so that the float32 kernels can be held to
float64 precision (no GPU needed here; tests/test_exact_tables_cpu.py, test_gpu_float32_exact.py).

The float32 tests of the suite compare with the oracle at 1e-5, which is right for float32
rounding but blind to the walk: `synthetic.synthetic_table` gives n_h ~ 10^(-0.9 log M), so the
pair weights span nine orders of magnitude, and a large share of the 4 x 4 matrix blocks adds
less than 1e-5 to xi in every r bin.  Here n_h x occupation, the matrix entries and the spline
weights are short dyadic numbers.  Written as integers times a power of two (the product of the
units, `lsb`), every product and every partial sum a kernel can form -- n_i n_j, the chains of
the matrix instructions, F += D e, slabs, merges -- is an integer multiple of `lsb`, and if

    sum_k |w_k| sum_ij |pre_ij n_i n_j T_ijr|  <  2^24 lsb

for a draw and an r bin, each is below 2^24 lsb and therefore a float: whatever the order or
the factorisation, the float32 result is the exact sum.  `assert_representable` states that from
the inputs alone, in integer arithmetic; a case that violates it is a mistake in the test.

Two routes lead to the densities:

occupation route (`occupation_case`): an integer occupation array for `halotab.predict(ndarray)`;
    every draw has its own pattern (all bins, runs of empty bins, no centrals, no satellites, a
    single bin).
theta route (`theta_case`, tables and interpolators): Zheng07 draws whose occupations are exactly
    0 or 1 -- alpha = 0, sigma_logM = 0.1, logMmin = 8 (centrals on) or 20 (off), logM0 below all
    bins, above all bins or exactly on a bin edge.  The interpolator kernels multiply the densities
    by (float)(spline weight / pair-weight norm), which is dyadic only for a power-of-two norm:
    n_h is chosen so that ngal of every pattern used is a power of two (centrals 1/2, all
    satellites 1, satellites from the two chosen edges 1/2 and 1/4, centrals with the satellites
    from the first edge 1), and the grids have 4 or 5 uniform integer nodes with x on nodes and
    mid-points (weights in sixteenths, 64ths; 256ths on a (4, 4) grid).
"""

import itertools

import numpy as np

from tabcorr_amd import synthetic
from oracle import tabcorr_oracle as oracle

LIMIT = 1 << 24           # float32: integers below 2^24 are exact
EPS64 = float(np.finfo(np.float64).eps)
N_H_VALUES = (1, 2, 3)
OCCUPATION_MAX = 3
ENTRY_MAX = 3
AUTO_KEYS = ['centrals-centrals', 'centrals-satellites', 'satellites-satellites']
CROSS_KEYS = ['centrals', 'satellites']


def integer_matrix(shape, rng):
    """Entries in {-3, ..., 3}."""
    return rng.integers(-ENTRY_MAX, ENTRY_MAX + 1, size=shape).astype(np.float64)


def exact_table(n_prim, n_sec=1, tpcf_shape=(19, ), mode='auto', seed=0):
    """`synthetic.synthetic_table` with n_h in {1, 2, 3} (the centrals' and the satellites' rows
    of a bin drawn separately) and integer matrix entries."""
    table = synthetic.synthetic_table(n_prim, n_sec, tpcf_shape, mode, seed)
    rng = np.random.default_rng([seed, 77])
    table['gal_type']['n_h'] = rng.choice(N_H_VALUES, size=len(table['gal_type']))
    table['tpcf_matrix'] = integer_matrix(table['tpcf_matrix'].shape, rng)
    return table


def occupation_patterns(table, n_draws, seed=0):
    """(n_draws, n_bins) integers in {0, ..., 3}, a pattern per draw in turn: every bin drawn;
    runs of empty bins (whole 4-bin blocks among them); no centrals; no satellites; one bin."""
    n_bins = len(table['gal_type'])
    central = oracle.is_centrals(table['gal_type'])
    rng = np.random.default_rng([seed, n_bins, n_draws])
    occupation = rng.integers(0, OCCUPATION_MAX + 1, size=(n_draws, n_bins))
    for d in range(n_draws):
        kind = d % 5
        if kind == 1:
            for _ in range(1 + n_bins // 12):
                start = 4 * int(rng.integers(0, n_bins // 4 + 1))
                occupation[d, start:start + int(rng.integers(1, 10))] = 0
        elif kind == 2:
            occupation[d, central] = 0
        elif kind == 3:
            occupation[d, ~central] = 0
        elif kind == 4:
            occupation[d] = 0
            occupation[d, int(rng.integers(0, n_bins))] = int(rng.integers(1, OCCUPATION_MAX + 1))
        if not occupation[d].any():     # (ngal = 0 is another test's subject)
            occupation[d, int(rng.integers(0, n_bins))] = 1
    return occupation


def as_integers(values, what, unit=1.0):
    """`values / unit` as int64, or an AssertionError if they are not integers."""
    scaled = np.asarray(values, dtype=np.float64) / unit
    rounded = np.rint(scaled)
    assert np.array_equal(scaled, rounded), '%s: not integer multiples of %g' % (what, unit)
    return rounded.astype(np.int64)


def component_masks(table):
    """{key: boolean mask over the matrix columns} as `oracle.predict` separates them."""
    central = oracle.is_centrals(table['gal_type'])
    if table['attrs']['mode'] == 'cross':
        return {'centrals': central, 'satellites': ~central}
    index_1, index_2, _ = oracle.pair_indices(len(central))
    c_1, c_2 = central[index_1], central[index_2]
    return {'centrals-centrals': c_1 & c_2, 'centrals-satellites': c_1 != c_2,
            'satellites-satellites': ~c_1 & ~c_2}


def integer_sums(table, density, n_h_unit=1.0, components=True):
    """The contraction in int64 for densities `density` (n_draws, n_bins), integers in units of
    `n_h_unit`: a dict with `norm` (n_draws, ) the sum of the pair weights pre_ij n_i n_j (mode
    cross: n_i), and per key ('total' and, with `components`, the components) `sums`
    (n_draws, R) = sum_p weights T and `abs_sums` = sum_p weights |T|."""
    n = as_integers(density, 'densities', n_h_unit)
    assert n.min() >= 0
    matrix = as_integers(table['tpcf_matrix'], 'matrix entries')
    if table['attrs']['mode'] == 'auto':
        index_1, index_2, prefactor = oracle.pair_indices(n.shape[1])
        weights = prefactor.astype(np.int64) * n[:, index_1] * n[:, index_2]
    else:
        weights = n
    masks = {'total': slice(None)}
    if components:
        masks.update(component_masks(table))
    sums, abs_sums = {}, {}
    for key, mask in masks.items():
        sums[key] = weights[:, mask] @ matrix[:, mask].T
        abs_sums[key] = weights[:, mask] @ np.abs(matrix[:, mask]).T
    return {'norm': weights.sum(axis=1), 'sums': sums, 'abs_sums': abs_sums}


def assert_representable(abs_sums, what=''):
    """sum |terms| < 2^24 in units of lsb, for every draw and r bin (integers in, no rounding)."""
    abs_sums = np.asarray(abs_sums)
    assert abs_sums.dtype == np.int64, what
    worst = int(abs_sums.max())
    assert worst < LIMIT, ('%s: sum |terms| = %d lsb is not below 2^24: float32 sums of this '
                           'case need not be exact (a mistake in the test\'s construction)'
                           % (what, worst))
    return worst


class ExactCase:
    """What a test needs of one exact case.

    table(s), the inputs of the device call (`occupation`, or `theta` and `x`), and per key
    ('total' and the components), all (n_draws, R) float64:
    expect[key]     the exact result (one division of two exactly represented numbers)
    allowance[key]  sum |terms| / norm, the quantity the tolerances multiply
    abs_lsb[key]    sum |terms| in units of `lsb` (int64), what `assert_representable` checked
    `lsb` is the real value of one unit of the sums before the normalisation."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def occupation_case(n_prim, n_sec, tpcf_shape, mode, n_draws, seed=0, components=True):
    """Occupation route: an exact table and an integer occupation array."""
    table = exact_table(n_prim, n_sec, tpcf_shape, mode, seed)
    occupation = occupation_patterns(table, n_draws, seed)
    density = occupation * as_integers(table['gal_type']['n_h'], 'n_h')
    exact = integer_sums(table, density, components=components)
    assert exact['norm'].min() > 0
    what = 'occupation %s %dx%dx%s' % (mode, n_prim, n_sec, tpcf_shape)
    assert_representable(exact['abs_sums']['total'], what)
    norm = exact['norm'].astype(np.float64)[:, np.newaxis]
    return ExactCase(
        table=table, tpcf_shape=tuple(tpcf_shape), mode=mode, lsb=1.0,
        occupation=occupation.astype(np.float64), ngal=density.sum(axis=1).astype(np.float64),
        ngal_parts={'centrals': density[:, oracle.is_centrals(table['gal_type'])].sum(axis=1),
                    'satellites': density[:, ~oracle.is_centrals(table['gal_type'])].sum(axis=1)},
        abs_lsb=exact['abs_sums'],
        expect={key: value.astype(np.float64) / norm for key, value in exact['sums'].items()},
        allowance={key: value.astype(np.float64) / norm
                   for key, value in exact['abs_sums'].items()})


def oracle_occupation(case, separate=False):
    """`oracle.predict` draw by draw for an occupation-route case: (ngal, xi), stacked."""
    cache = {}
    results = [oracle.predict(case.table, occupation, separate, cache)
               for occupation in case.occupation]
    return oracle._stack(results, separate)


def float32_emulation(table, density, mask, order):
    """What a float32 kernel computes for one draw, in numpy: the inputs cast to float32, the terms
    pre_ij n_i n_j T_ijr of the columns `mask` formed in float32 and added one by one in the
    order `order` (a permutation of the masked columns) with a float32 accumulator.  (R, )
    float32."""
    n = np.asarray(density, dtype=np.float32)
    matrix = np.asarray(table['tpcf_matrix'], dtype=np.float32)[:, mask][:, order]
    if table['attrs']['mode'] == 'auto':
        index_1, index_2, prefactor = oracle.pair_indices(len(n))
        weights = (prefactor.astype(np.float32) * n[index_1] * n[index_2])[mask][order]
    else:
        weights = n[mask][order]
    assert weights.dtype == np.float32 and matrix.dtype == np.float32
    terms = matrix * weights                      # float32 products
    # (a cumulative sum in float32 rounds after every addition, in the order given)
    return np.cumsum(terms, axis=1, dtype=np.float32)[:, -1]


# -- theta route --------------------------------------------------------------------------------

PATTERNS = ('centrals', 'all satellites', 'satellites from edge 1', 'satellites from edge 2',
            'centrals and satellites from edge 1')


def fill_to_sum(length, total, rng):
    """`length` integers in {1, ..., 4} that add up to `total`."""
    assert length <= total <= 4 * length, (length, total)
    values = np.ones(length, dtype=np.int64)
    while values.sum() < total:
        i = int(rng.integers(0, length))
        if values[i] < 4:
            values[i] += 1
    return values


def power_of_two_n_h(n_prim, seed):
    """n_h of the centrals' and the satellites' bins (n_sec = 1) and the two edges, such that
    ngal of every pattern of `PATTERNS` is a power of two: with L = 2 n_prim // 7 and S the
    smallest power of two >= 2 L, the satellites of the last L bins add up to S integers, those
    of the L bins before them to S and the rest to 2 S; the centrals to 2 S; in units of
    1 / (4 S).  So centrals = 1/2, all satellites = 1, from edge 1 = 1/2, from edge 2 = 1/4 and
    centrals with the satellites from edge 1 = 1."""
    rng = np.random.default_rng([seed, n_prim, 99])
    length = 2 * n_prim // 7
    part = 1
    while part < 2 * length:
        part *= 2
    edge_1, edge_2 = n_prim - 2 * length, n_prim - length
    satellites = np.concatenate([fill_to_sum(edge_1, 2 * part, rng),
                                 fill_to_sum(length, part, rng), fill_to_sum(length, part, rng)])
    centrals = fill_to_sum(n_prim, 2 * part, rng)
    unit = 1.0 / (4 * part)
    return centrals, satellites, (edge_1, edge_2), unit


def is_power_of_two(value):
    mantissa, _ = np.frexp(np.asarray(value, dtype=np.float64))
    return np.all(mantissa == 0.5)


def theta_draws(table, edges, n_draws):
    """Zheng07 draws (logMmin, sigma_logM, logM0, logM1, alpha) whose occupations are exactly 0
    or 1, pattern d % 5 of `PATTERNS` for draw d, and the patterns' indices."""
    log_min = table['gal_type']['log_prim_haloprop_min']
    n_prim = len(log_min) // 2
    assert np.array_equal(log_min[1:n_prim], table['gal_type']['log_prim_haloprop_max'][:n_prim - 1])
    log_m0 = {0: 16.0, 1: 9.0, 2: log_min[edges[0]], 3: log_min[edges[1]], 4: log_min[edges[0]]}
    pattern = np.arange(n_draws) % len(PATTERNS)
    theta = np.empty((n_draws, 5))
    theta[:, 0] = np.where((pattern == 0) | (pattern == 4), 8.0, 20.0)
    theta[:, 1] = 0.1
    theta[:, 2] = [log_m0[p] for p in pattern]
    theta[:, 3] = 13.0
    theta[:, 4] = 0.0
    return theta, pattern


def pattern_occupation(n_prim, edges, pattern):
    """(n_draws, 2 n_prim) exact 0 / 1 occupations of the patterns."""
    occupation = np.zeros((len(pattern), 2 * n_prim), dtype=np.int64)
    bins = np.arange(n_prim)
    for d, p in enumerate(pattern):
        if p in (0, 4):
            occupation[d, :n_prim] = 1
        if p == 1:
            occupation[d, n_prim:] = 1
        if p in (2, 4):
            occupation[d, n_prim:] = bins >= edges[0]
        if p == 3:
            occupation[d, n_prim:] = bins >= edges[1]
    return occupation


def axis_weights(nodes, x):
    """The oracle's spline weights of the nodes at `x` as integers over a power-of-two
    denominator: (numerators int64, denominator)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    a = oracle.spline_interpolation_matrix(nodes)
    weights = oracle.spline_interpolate([x], [nodes], [a], np.eye(len(nodes)))
    for denominator in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        scaled = weights * denominator
        if np.max(np.abs(scaled - np.rint(scaled))) < 1e-9:
            return np.rint(scaled).astype(np.int64), denominator
    raise AssertionError('the spline weights %s at x = %g are not short dyadic numbers'
                         % (weights, x))


def grid_x(grid, n_draws):
    """x per draw: nodes and mid-points in turn (the second axis at half the pace, so that all
    four combinations occur), another node or interval each time."""
    x = np.empty((n_draws, len(grid)))
    for d in range(n_draws):
        for axis, n_nodes in enumerate(grid):
            step = d // (2 << axis) + 3 * axis
            on_node = (d >> axis) % 2 == 0
            x[d, axis] = step % n_nodes if on_node else step % (n_nodes - 1) + 0.5
    return x


def theta_case(grid, n_prim, tpcf_shape, mode, n_classes, n_draws, seed=0):
    """Theta route.  `grid` = () gives a single table; (4, ), (4, 4), (5, ) an interpolator on
    integer nodes 0, 1, ... with its own integer matrix per node and `n_classes` (1 or 2)
    different n_h columns (nodes alternate)."""
    n_tables = int(np.prod(grid)) if grid else 1
    base = synthetic.synthetic_table(n_prim, 1, tpcf_shape, mode, seed)
    rng = np.random.default_rng([seed, n_tables, 55])
    classes = [power_of_two_n_h(n_prim, seed + 10 * c) for c in range(n_classes)]
    # (the same edges and unit for every class: the draws and lsb are shared)
    edges, unit = classes[0][2], classes[0][3]
    assert all(c[2] == edges and c[3] == unit for c in classes)
    tables = []
    for k in range(n_tables):
        # (the second class twice as dense: ngal and the norms differ between the classes)
        centrals, satellites = classes[k % n_classes][:2]
        table = dict(base)
        table['gal_type'] = base['gal_type'].copy()
        table['gal_type']['n_h'] = (np.concatenate([centrals, satellites]) * unit *
                                    2**(k % n_classes))
        table['tpcf_matrix'] = integer_matrix(base['tpcf_matrix'].shape, rng)
        tables.append(table)
    theta, pattern = theta_draws(base, edges, n_draws)
    occupation = pattern_occupation(n_prim, edges, pattern)
    keys, points = None, None
    if grid:
        keys = ('log_eta', 'alpha_s', 'alpha_c')[:len(grid)]
        mesh = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in grid], indexing='ij')
        points = np.stack([m.ravel() for m in mesh], axis=-1)
        x = grid_x(grid, n_draws)
    else:
        x = None
    # spline weights of every table: numerators (n_draws, K) over one denominator
    numerators = np.ones((n_draws, n_tables), dtype=np.int64)
    denominator = 1
    if grid:
        per_axis = [[axis_weights(np.arange(n), x[d, axis]) for d in range(n_draws)]
                    for axis, n in enumerate(grid)]
        axis_denominator = [max(w[1] for w in draws) for draws in per_axis]
        for d in range(n_draws):
            vectors = [per_axis[axis][d][0] * (axis_denominator[axis] // per_axis[axis][d][1])
                       for axis in range(len(grid))]
            numerators[d] = [int(np.prod(c)) for c in itertools.product(*vectors)]
        denominator = int(np.prod(axis_denominator))
        assert np.all(numerators.sum(axis=1) == denominator)
    # per table: the integer sums, and its norm (a power of two, asserted) relative to the largest
    keys_out = ['total'] + (AUTO_KEYS if mode == 'auto' else CROSS_KEYS)
    per_table = []
    for table in tables:
        density = occupation * table['gal_type']['n_h']
        exact = integer_sums(table, density, unit)
        assert exact['norm'].min() > 0
        assert is_power_of_two(exact['norm']), 'norm of a pattern is not a power of two'
        assert is_power_of_two(density.sum(axis=1)), 'ngal of a pattern is not a power of two'
        per_table.append(exact)
    norm_max = np.max([e['norm'] for e in per_table], axis=0)               # (n_draws, )
    expect, allowance, abs_lsb = {}, {}, {}
    for key in keys_out:
        total = np.zeros((n_draws, base['tpcf_matrix'].shape[0]), dtype=np.int64)
        total_abs = np.zeros_like(total)
        for k, exact in enumerate(per_table):
            shift = norm_max // exact['norm']
            assert np.array_equal(shift * exact['norm'], norm_max)
            factor = (numerators[:, k] * shift)[:, np.newaxis]
            total += factor * exact['sums'][key]
            total_abs += np.abs(factor) * exact['abs_sums'][key]
        scale = (denominator * norm_max).astype(np.float64)[:, np.newaxis]
        abs_lsb[key] = total_abs
        expect[key] = total.astype(np.float64) / scale
        allowance[key] = total_abs.astype(np.float64) / scale
    what = 'theta %s grid %s %dx%s' % (mode, grid, n_prim, tpcf_shape)
    assert_representable(abs_lsb['total'], what)
    ngal_tables = np.array([(occupation * t['gal_type']['n_h']).sum(axis=1) for t in tables])
    central = oracle.is_centrals(base['gal_type'])
    parts_tables = {
        'centrals': np.array([(occupation * t['gal_type']['n_h'])[:, central].sum(axis=1)
                              for t in tables]),
        'satellites': np.array([(occupation * t['gal_type']['n_h'])[:, ~central].sum(axis=1)
                                for t in tables])}
    weights = numerators.T / float(denominator)
    return ExactCase(
        tables=tables, table=tables[0], keys=keys, points=points, grid=tuple(grid),
        tpcf_shape=tuple(tpcf_shape), mode=mode, theta=theta, x=x, pattern=pattern,
        occupation=occupation, lsb=unit * unit if mode == 'auto' else unit,
        ngal=np.sum(weights * ngal_tables, axis=0),
        ngal_parts={key: np.sum(weights * value, axis=0) for key, value in parts_tables.items()},
        abs_lsb=abs_lsb, expect=expect, allowance=allowance)


def oracle_theta_direct(case, separate=False):
    """The oracle's (ngal, xi) of a theta-route case, draw by draw."""
    if case.grid:
        setup = oracle.interpolator_setup(case.tables, case.points)
        return oracle.interpolator_predict_zheng07_batch(case.tables, setup, case.theta, case.x,
                                                         separate_gal_type=separate)
    return oracle.predict_zheng07_batch(case.table, case.theta, separate_gal_type=separate)


def oracle_theta(case, separate=False):
    """`oracle_theta_direct`, bit for bit (tests/test_exact_tables_cpu.py compares them), at a
    fraction of its cost: the draws repeat five parameter vectors, so the tables' predictions --
    `oracle.interpolator_predict` up to its spline step, the same calls in the same order -- are
    formed once per vector, and only `oracle.spline_interpolate` runs per draw."""
    n_patterns = len(PATTERNS)
    assert np.array_equal(case.theta, case.theta[case.pattern])      # (draw d repeats d % 5)
    if not case.grid:
        cache = {}
        results = [oracle.predict_zheng07(case.table, theta, separate, cache=cache)
                   for theta in case.theta[:n_patterns]]
        return oracle._stack([results[p] for p in case.pattern], separate)
    setup = oracle.interpolator_setup(case.tables, case.points)
    shape = [len(xp) for xp in setup['xp']]
    data = []           # per parameter vector: (ngal, xi) on the grid, dicts if separated
    for theta in case.theta[:n_patterns]:
        model = oracle.Zheng07(theta)
        occupation = [oracle.mean_occupation(case.tables[i], model)
                      for i in setup['unique_index']]
        results = [oracle.predict(case.tables[k], occupation[setup['unique_inverse'][k]], separate)
                   for k in setup['order']]
        on_grid = []
        for i in range(2):
            if separate:
                on_grid.append({})
                for key in results[0][i]:
                    values = np.array([r[i][key] for r in results])
                    on_grid[-1][key] = values.reshape(shape + list(values.shape[1:]))
            else:
                values = np.array([r[i] for r in results])
                on_grid.append(values.reshape(shape + list(values.shape[1:])))
        data.append(on_grid)
    outputs = []
    for p, x in zip(case.pattern, case.x):
        def interpolate(values):
            return oracle.spline_interpolate(x, setup['xp'], setup['a'], values)
        outputs.append(tuple(
            {key: interpolate(values) for key, values in part.items()} if separate
            else interpolate(part) for part in data[p]))
    return oracle._stack(outputs, separate)


# -- how much of a table the 1e-5 bar cannot see ---------------------------------------------------

def block_of_column(n_bins):
    """The 4 x 4 block (unit) of the pair triangle that every packed column lies in, numbered
    bI (bI + 1) / 2 + bJ for block row bI >= block column bJ."""
    index_1, index_2, _ = oracle.pair_indices(n_bins)
    return (index_1 // 4) * (index_1 // 4 + 1) // 2 + index_2 // 4


def block_contributions(table, occupation):
    """xi of one draw as the oracle forms it, split by 4 x 4 block: (xi (R, ), per block
    (R, n_blocks)) with xi = the blocks' sum."""
    n_bins = len(table['gal_type'])
    index_1, index_2, prefactor = oracle.pair_indices(n_bins)
    block = block_of_column(n_bins)
    ngal = occupation * table['gal_type']['n_h']
    ngal_sq = prefactor * ngal[index_1] * ngal[index_2]
    terms = table['tpcf_matrix'] * ngal_sq / np.sum(ngal_sq)                          # (R, P)
    per_block = np.stack([np.bincount(block, weights=row, minlength=int(block.max()) + 1)
                          for row in terms])
    return terms.sum(axis=1), per_block


# -- the cases of tests/test_gpu_float32_exact.py (their construction is checked on the CPU too) ---

N_DRAWS = 130                       # 1, 63, 64, 65 and 130 draws are its leading rows
DRAW_COUNTS = (1, 63, 64, 65, 130)
# contract_quad_f32_kernel, tables (mode auto): (n_prim, n_sec, tpcf_shape).  Centrals that fill
# 4-bin blocks (4, 16, 32, 152 of them) and centrals that do not; U = 1 ... 4 sub-tiles, one to
# three r tiles and their tails; 2 * 152 = 304 bins: 3003 KB per r tile, the last size below the
# kernel's 3 MB limit (table.cpp)
QUAD_CASES = [(1, 1, (1, )), (1, 2, (3, )), (2, 1, (4, )), (2, 2, (7, )), (3, 1, (12, )),
              (3, 2, (3, 4)), (5, 1, (16, )), (5, 2, (17, )), (16, 1, (19, )), (16, 2, (40, )),
              (50, 1, (19, )), (50, 1, (7, )), (152, 1, (3, ))]
# contract_f32_kernel, tables: mode cross with 2, 16, 18, 36, 64 and 66 bins (= entries: multiples
# of its 8-entry step and not), 40 r values = two r tiles of 32; mode auto beyond the quad limit,
# 320 bins (51360 entries, a multiple of 8) and 322 bins (52003 entries)
CONTRACT_CASES = [(1, 1, (3, ), 'cross'), (4, 2, (19, ), 'cross'), (9, 1, (7, ), 'cross'),
                  (9, 2, (40, ), 'cross'), (16, 2, (12, ), 'cross'), (33, 1, (19, ), 'cross'),
                  (160, 1, (3, ), 'auto'), (161, 1, (3, ), 'auto')]
# interpolators (theta route): (grid, n_prim, tpcf_shape, mode, classes of halo tables).  Mode
# auto on a (4, 4) grid takes 14 bins: with 50 the sums of 16 tables weighted in 256ths pass 2^24.
INTERP_DRAW_COUNTS = (3, 64, 130)
INTERP_CASES = [((4, ), 14, (12, ), 'auto', 1), ((4, ), 50, (19, ), 'auto', 2),
                ((4, 4), 14, (19, ), 'auto', 2), ((5, ), 50, (12, ), 'auto', 1),
                ((5, ), 14, (19, ), 'auto', 2),
                ((4, ), 14, (19, ), 'cross', 2), ((4, ), 50, (12, ), 'cross', 1),
                ((4, 4), 50, (12, ), 'cross', 2), ((5, ), 50, (19, ), 'cross', 2)]
# single tables from Zheng07 draws (theta route, grid ())
THETA_TABLE_CASES = [((), 50, (19, ), 'auto', 1), ((), 14, (12, ), 'auto', 1),
                     ((), 50, (12, ), 'cross', 1)]
# the schedule sweeps: enough draws for the number of waves per SIMD to change the shares
SWEEP_CASES = [(50, 1, (19, ), 2560), (16, 2, (19, ), 130)]

_cache = {}


def cached(kind, *args):
    """A case built once per process: kind 'occupation' -> `occupation_case(*args)`, 'theta' ->
    `theta_case(*args)`.  The cases are read, never changed."""
    key = (kind, ) + args
    if key not in _cache:
        _cache[key] = (occupation_case if kind == 'occupation' else theta_case)(*args)
    return _cache[key]


def case_id(spec):
    return '-'.join(('x'.join(str(v) for v in part) or 'table') if isinstance(part, tuple)
                    else str(part) for part in spec)
