"""The construction behind tests/test_gpu_float32_exact.py, checked without a GPU
(tests/exact_tables.py): the cases are representable, float32 arithmetic on them is exact and
independent of the order, the theta-route draws give exact 0 / 1 occupations and power-of-two
number densities, the exact comparison notices every missing 4 x 4 block -- and the 1e-5
comparison of the synthetic tables does not, which is why that file exists."""

import numpy as np
import pytest

import exact_tables as ex
from oracle import tabcorr_oracle as oracle
from tabcorr_amd import synthetic

OCCUPATION_SPECS = ([spec + ('auto', ) for spec in ex.QUAD_CASES] + list(ex.CONTRACT_CASES))


@pytest.mark.parametrize('spec', OCCUPATION_SPECS, ids=ex.case_id)
def test_occupation_cases_are_representable(spec):
    """sum |terms| < 2^24 lsb for every draw and r bin (asserted by the helper in int64), every
    pattern occurs, and the exact result is the oracle's within 4 eps64 sum |terms| / norm."""
    case = ex.cached('occupation', *spec, ex.N_DRAWS)
    worst = ex.assert_representable(case.abs_lsb['total'], ex.case_id(spec))
    for key, value in case.abs_lsb.items():
        assert np.all(value <= case.abs_lsb['total']), key
    occupation = case.occupation
    central = oracle.is_centrals(case.table['gal_type'])
    assert occupation.min() == 0 and occupation.max() == ex.OCCUPATION_MAX
    assert np.array_equal(occupation, np.rint(occupation))
    assert np.any(~occupation[:, central].any(axis=1)) and np.any(~occupation[:, ~central].any(axis=1))
    assert np.all(occupation.any(axis=1))
    if len(central) >= 8:       # (a whole 4-bin block of zeros beside occupied bins)
        blocks = occupation[:, :len(central) // 4 * 4].reshape(len(occupation), -1, 4)
        has_empty_block = (~blocks.any(axis=2)).any(axis=1)
        assert np.any(has_empty_block & ((occupation != 0).sum(axis=1) >= 4))
    ngal, xi = ex.oracle_occupation(case)
    assert np.array_equal(ngal, case.ngal)
    xi = xi.reshape(len(ngal), -1)
    excess = np.max(np.abs(xi - case.expect['total']) /
                    np.maximum(4 * ex.EPS64 * case.allowance['total'], 1e-300))
    print('%s: sum |terms| up to %d lsb (2^24 = %d), oracle - exact up to %.2f of the allowance'
          % (ex.case_id(spec), worst, ex.LIMIT, excess))
    assert excess <= 1.0


@pytest.mark.parametrize('spec', [spec[:3] + ('auto', spec[3]) for spec in ex.SWEEP_CASES],
                         ids=ex.case_id)
def test_sweep_cases_are_representable(spec):
    case = ex.cached('occupation', *spec, 0, False)
    ex.assert_representable(case.abs_lsb['total'], ex.case_id(spec))


@pytest.mark.parametrize('spec', ex.INTERP_CASES + ex.THETA_TABLE_CASES, ids=ex.case_id)
def test_theta_cases_are_representable(spec):
    """The same for the interpolators, spline weights and per-table norms included; the oracle
    gives exact 0 / 1 occupations and a power-of-two ngal for every table and draw, reproduces the
    dyadic spline weights, and agrees with the exact result within the theta route's
    4e-12 sum |terms| / norm."""
    case = ex.cached('theta', *spec, ex.N_DRAWS)
    ex.assert_representable(case.abs_lsb['total'], ex.case_id(spec))
    assert sorted(set(case.pattern)) == list(range(len(ex.PATTERNS)))
    for table in case.tables:
        for theta, expected in zip(case.theta[:len(ex.PATTERNS)], case.occupation):
            occupation = oracle.mean_occupation(table, oracle.Zheng07(theta))
            assert np.array_equal(occupation, expected)          # (departure 0.0)
            ngal = np.sum(occupation * table['gal_type']['n_h'])
            assert ex.is_power_of_two(ngal), ngal
    grid = spec[0]
    for axis, n_nodes in enumerate(grid):       # nodes and mid-points, every node and interval
        on_node = case.x[:, axis] == np.rint(case.x[:, axis])
        assert set(case.x[on_node, axis]) == set(range(n_nodes))
        assert set(case.x[~on_node, axis]) == {i + 0.5 for i in range(n_nodes - 1)}
    if grid:
        assert np.any(np.all(case.x == np.rint(case.x), axis=1))
        assert np.any(np.all(case.x != np.rint(case.x), axis=1))
    n_h = np.array([table['gal_type']['n_h'] for table in case.tables])
    assert len(np.unique(n_h, axis=0)) == spec[4]
    matrices = np.array([table['tpcf_matrix'] for table in case.tables])
    assert len(np.unique(matrices, axis=0)) == len(case.tables)
    for separate in (False, True):
        ngal, xi = ex.oracle_theta_direct(case, separate)
        quick_ngal, quick_xi = ex.oracle_theta(case, separate)    # (what the GPU tests call)
        if not separate:
            ngal, xi = {'total': ngal}, {'total': xi}
            quick_ngal, quick_xi = {'total': quick_ngal}, {'total': quick_xi}
        for quick, direct in ((quick_ngal, ngal), (quick_xi, xi)):
            assert sorted(quick) == sorted(direct)
            for key in direct:
                assert quick[key].shape == direct[key].shape
                assert np.array_equal(quick[key].view(np.uint64), direct[key].view(np.uint64)), key
        if separate:
            for key in ngal:
                np.testing.assert_allclose(ngal[key], case.ngal_parts[key], rtol=1e-12,
                                           atol=1e-12 * np.max(case.ngal))
        for key in xi:
            got = xi[key].reshape(len(case.theta), -1)
            excess = np.max(np.abs(got - case.expect[key]) /
                            np.maximum(4e-12 * case.allowance[key], 1e-300))
            assert excess <= 1.0, (key, excess)
    np.testing.assert_allclose(ngal['centrals'] + ngal['satellites'], case.ngal, rtol=1e-12)


def test_spline_weights_are_dyadic():
    """4 uniform nodes: (-1, 9, 9, -1) / 16 and (5, 15, -5, 1) / 16 at the mid-points; 5 nodes:
    64ths.  The oracle (an inverted matrix times powers of x) reproduces the former to 2e-15 and
    the latter to 2e-14 -- what the theta route's 4e-12 has to cover on the oracle's side."""
    numerators, denominator = ex.axis_weights(np.arange(4), 1.5)
    assert denominator == 16 and list(numerators) == [-1, 9, 9, -1]
    numerators, denominator = ex.axis_weights(np.arange(4), 0.5)
    assert denominator == 16 and list(numerators) == [5, 15, -5, 1]
    numerators, denominator = ex.axis_weights(np.arange(4), 2.0)
    assert list(numerators * (16 // denominator)) == [0, 0, 16, 0]
    nodes = np.arange(4.0)
    a = oracle.spline_interpolation_matrix(nodes)
    for x, expected in ((0.5, [5, 15, -5, 1]), (1.5, [-1, 9, 9, -1]), (2.5, [1, -5, 15, 5])):
        weights = oracle.spline_interpolate([x], [nodes], [a], np.eye(4))
        assert np.max(np.abs(weights - np.array(expected) / 16)) < 2e-15
    for x in (0.5, 1.5, 2.5, 3.5):
        numerators, denominator = ex.axis_weights(np.arange(5), x)
        assert denominator <= 64 and numerators.sum() == denominator
        nodes = np.arange(5.0)
        a = oracle.spline_interpolation_matrix(nodes)
        weights = oracle.spline_interpolate([x], [nodes], [a], np.eye(5))
        assert np.max(np.abs(weights - numerators / denominator)) < 2e-14


# (table spec, mode, draws emulated): small tables, every pattern, and the 50-bin case
EMULATED = [((3, 2, (3, 4)), 'auto', 10), ((16, 1, (19, )), 'auto', 10), ((50, 1, (19, )), 'auto', 5),
            ((9, 2, (40, )), 'cross', 10)]


@pytest.mark.parametrize('spec, mode, n_emulated', EMULATED,
                         ids=[ex.case_id(spec) + '-' + mode for spec, mode, _ in EMULATED])
def test_float32_sums_are_exact_in_any_order(spec, mode, n_emulated):
    """A numpy float32 emulation -- inputs cast to float32, the terms added one by one in two
    different random orders -- gives identical bits, the integer sum, and after the one division
    the float64 oracle within 4 eps64 sum |terms| / norm; total and every component."""
    case = ex.cached('occupation', *spec, mode, ex.N_DRAWS)
    masks = dict(ex.component_masks(case.table), total=np.ones(case.table['tpcf_matrix'].shape[1],
                                                               dtype=bool))
    ngal_sep, xi_sep = ex.oracle_occupation(case, separate=True)
    _, xi_total = ex.oracle_occupation(case)
    expect = dict(xi_sep, total=xi_total)
    rng = np.random.default_rng(5)
    density = case.occupation * case.table['gal_type']['n_h']
    for d in range(n_emulated):
        norm = np.sum(density[d])**2 if mode == 'auto' else np.sum(density[d])
        for key, mask in masks.items():
            count = int(mask.sum())
            first = ex.float32_emulation(case.table, density[d], mask, rng.permutation(count))
            second = ex.float32_emulation(case.table, density[d], mask, rng.permutation(count))
            assert first.dtype == np.float32
            assert np.array_equal(first.view(np.uint32), second.view(np.uint32)), (d, key)
            got = first.astype(np.float64) / norm
            assert np.array_equal(got, case.expect[key][d]), (d, key)
            bound = 4 * ex.EPS64 * case.allowance[key][d]
            assert np.all(np.abs(got - expect[key][d].ravel()) <= bound), (d, key)


def emulated_block_breaks(case, block, draws):
    """Whether the float32 emulation with 4 x 4 block `block` of the matrix zeroed leaves the
    exact comparison's allowance for one of `draws` (total prediction)."""
    table = dict(case.table)
    columns = ex.block_of_column(len(table['gal_type'])) == block
    table['tpcf_matrix'] = np.where(columns, 0.0, case.table['tpcf_matrix'])
    density = case.occupation * case.table['gal_type']['n_h']
    everything = np.ones(len(columns), dtype=bool)
    order = np.arange(len(columns))
    for d in draws:
        got = ex.float32_emulation(table, density[d], everything, order).astype(np.float64)
        got /= np.sum(density[d])**2
        if np.any(np.abs(got - case.expect['total'][d]) >
                  4 * ex.EPS64 * case.allowance['total'][d]):
            return True
    return False


@pytest.mark.parametrize('which', ['first', 'middle', 'last'])
@pytest.mark.parametrize('spec', [(16, 1, (19, )), (50, 1, (19, )), (5, 2, (17, ))], ids=ex.case_id)
def test_a_missing_block_breaks_the_exact_comparison(spec, which):
    case = ex.cached('occupation', *spec, 'auto', ex.N_DRAWS)
    n_blocks = int(ex.block_of_column(len(case.table['gal_type'])).max()) + 1
    block = {'first': 0, 'middle': n_blocks // 2, 'last': n_blocks - 1}[which]
    assert emulated_block_breaks(case, block, range(ex.N_DRAWS))


def test_every_block_of_the_50_bin_case_breaks_it():
    case = ex.cached('occupation', 50, 1, (19, ), 'auto', ex.N_DRAWS)
    n_blocks = int(ex.block_of_column(100).max()) + 1
    assert n_blocks == 325
    unseen = [block for block in range(n_blocks)
              if not emulated_block_breaks(case, block, range(ex.N_DRAWS))]
    assert unseen == []


@pytest.fixture(scope='module')
def synthetic_blocks():
    """Per existing float32 shape of test_gpu_full_size.test_float32_variant_small: xi of its 40
    oracle draws (40, R) and the 4 x 4 blocks' contributions (40, R, n_blocks)."""
    out = {}
    for name, spec, seed in (('50x1x19', (50, 1, (19, )), 0), ('12x1x(7, 9)', (12, 1, (7, 9)), 41)):
        table = synthetic.synthetic_table(*spec, mode='auto', seed=seed)
        theta = synthetic.zheng07_draws(200, seed=seed + 1)[:40]
        parts = [ex.block_contributions(table, oracle.mean_occupation(table, oracle.Zheng07(t)))
                 for t in theta]
        out[name] = (np.array([p[0] for p in parts]), np.array([p[1] for p in parts]))
    return out


def test_the_float32_bar_of_the_suite_cannot_see_many_blocks(synthetic_blocks):
    """The measurement behind this file, from the oracle alone: the share of 4 x 4 blocks that add
    less than 1e-5 of xi in every r bin, per draw."""
    for name, (xi, blocks) in synthetic_blocks.items():
        invisible = np.all(np.abs(blocks) < 1e-5 * np.abs(xi)[:, :, np.newaxis], axis=1)
        share = invisible.mean(axis=1)
        print('%s: %d blocks; below 1e-5 of xi in every r bin: %.0f %% on average, %.0f %% at the '
              'least' % (name, blocks.shape[2], 100 * share.mean(), 100 * share.min()))
        if name == '50x1x19':
            assert blocks.shape[2] == 325
            assert share.mean() > 0.10 and share.min() > 0.10


def test_a_missing_block_passes_the_float32_bar_of_the_suite(synthetic_blocks):
    """The gap: at the suite's float32 tolerance (test_gpu_full_size.py: relative 1e-5 with a floor
    of 1e-5 of the largest element) the 50-bin synthetic case does not notice that a block is
    missing, on any of its 40 draws, for at least a tenth of the blocks."""
    xi, blocks = synthetic_blocks['50x1x19']
    tolerance = 1e-5 * np.abs(xi) + 1e-14 * np.max(np.abs(xi))      # (util.assert_rel)
    passes = np.all(np.abs(blocks) <= tolerance[:, :, np.newaxis], axis=(0, 1))
    print('50x1x19: %d of %d blocks can go missing at 1e-5' % (passes.sum(), passes.size))
    assert passes.mean() >= 0.10
