"""GPU pair counts (tabcorr_amd/csrc/paircount.hip) against the brute-force oracle
(oracle/paircount_oracle.py) on the plans the other pair-count tests never produce: several
label blocks on the side of sample 1, partial last blocks, blocks of one label, two labelled
samples, the 27-neighbour grids with real load, cells streamed in several tiles, the wrap
shortcut with 5, 6 and 7 cells along every axis, and the sizes at which the LDS counters
reach their limits.  Integer counts: the bar is np.array_equal on uint64.

Every test first asserts, through tc_debug_pair_plan (no device involved) and with NumPy on
its own positions, that its inputs produce the grid, the label blocks and the cell occupancy
it is there for: a test that drifts off its branch fails.  The plans themselves are pinned in
tests/test_paircount_plan_cpu.py."""

import ctypes
import functools
import sys

import numpy as np
import pytest

from util import REPO, cell_occupancy, pair_plan

sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu

BOX = np.array([100.0, 100.0, 100.0])


def around(occupancy, neighbours):
    """Points in the cells around every cell: `neighbours` cells to each side, periodic."""
    total = np.zeros_like(occupancy)
    for ox in range(-neighbours[0], neighbours[0] + 1):
        for oy in range(-neighbours[1], neighbours[1] + 1):
            for oz in range(-neighbours[2], neighbours[2] + 1):
                total += np.roll(occupancy, (ox, oy, oz), axis=(0, 1, 2))
    return total


def split_by_label(pos, label, n_labels):
    """The per-bin position arrays TabCorr.tabulate hands to corrfunc.pair_count_matrix."""
    order = np.argsort(label, kind='stable')
    return np.split(pos[order], np.cumsum(np.bincount(label, minlength=n_labels))[:-1])


@functools.lru_cache(maxsize=None)
def labelled_set(n, n_labels, seed=1):
    """n points in a box of 100^3: about 12 clumps (sigma 2) over a uniform background.  The
    last label holds a single point (it is the whole of a partial last block where the labels
    are no multiple of the block), one label in the middle is empty (three labels or more),
    and one clump of 300 points carries a single label of the upper half."""
    rng = np.random.default_rng(seed)
    heavy_count = min(300, n // 3)
    centres = rng.uniform(10.0, 90.0, (12, 3))
    n_clumped = (n - heavy_count) // 2
    pos = np.vstack([
        centres[rng.integers(0, 12, n_clumped)] + rng.normal(0.0, 2.0, (n_clumped, 3)),
        rng.uniform(0.0, 1.0, (n - heavy_count - n_clumped, 3)) * BOX,
        np.array([50.0, 50.0, 50.0]) + rng.normal(0.0, 2.0, (heavy_count, 3))])
    pos = np.ascontiguousarray(np.mod(pos, BOX))
    lonely = n_labels - 1
    empty = n_labels // 2 if n_labels >= 3 else -1
    heavy = n_labels - 3 if n_labels >= 4 else 0
    usable = np.array([k for k in range(n_labels) if k not in (lonely, empty)])
    label = usable[rng.integers(0, len(usable), n)]
    label[n - heavy_count:] = heavy
    label[0] = lonely
    counts = np.bincount(label, minlength=n_labels)
    assert counts[lonely] == 1 and (empty < 0 or counts[empty] == 0)
    pos.setflags(write=False)
    label.setflags(write=False)
    return pos, label, heavy


@functools.lru_cache(maxsize=None)
def plain_set(n, seed=2):
    """An unlabelled second sample: half in clumps around the centre of the box."""
    rng = np.random.default_rng(seed)
    pos = np.vstack([np.array([50.0, 50.0, 50.0]) + rng.normal(0.0, 6.0, (n // 2, 3)),
                     rng.uniform(0.0, 1.0, (n - n // 2, 3)) * BOX])
    pos = np.ascontiguousarray(np.mod(pos, BOX))
    pos.setflags(write=False)
    return pos


# case: (kind, bins, labels, (labels per block 1, 2, blocks 1, 2), points)
LABELLED_CASES = {
    'L1': ('rp', (19, ), 50, (50, 8, 1, 7), 3500),          # last block of side 2: 2 labels
    'L2': ('rp', (64, ), 70, (35, 2, 2, 35), 3500),
    'L3': ('rp', (64, ), 71, (36, 2, 2, 36), 3500),         # both last blocks partial
    'S1': ('smu', (8, 10), 51, (26, 2, 2, 26), 3500),
    'S2': ('smu', (60, 64), 3, (1, 2, 3, 2), 1000),
    'S3': ('smu', (60, 120), 3, (1, 2, 3, 2), 1000),        # 14 400 counters: 56.25 KB
    'S4': ('smu', (64, 121), 3, (1, 1, 3, 3), 1000),
    'S5': ('smu', (64, 240), 2, (1, 1, 2, 2), 1000),        # the documented maximum: 60 KB
}
REACH = 20.0


def edges(n_bins, first=0.1):
    out = np.concatenate([[first], np.logspace(-0.7, np.log10(REACH), n_bins)])
    out[-1] = REACH
    return out


@pytest.mark.parametrize('case', sorted(LABELLED_CASES))
def test_label_block_plans_against_the_oracle(case):
    """Auto, and cross against an unlabelled second sample, through
    corrfunc.pair_count_matrix[_smu] -- the way the tabulation counts."""
    from tabcorr_amd import corrfunc
    from oracle import paircount_oracle as oracle
    kind, bins, n_labels, expect_plan, n = LABELLED_CASES[case]
    pos, label, heavy = labelled_set(n, n_labels)
    other = plain_set(n - 500)
    n_bin = int(np.prod(bins))
    plan = pair_plan(BOX, REACH, REACH, n, n_bin, n_labels)
    print('PLAN', case, kind, bins, n_labels, plan)
    assert plan['plan'] == expect_plan, plan
    assert plan['lds_bytes'] == 4 * n_bin * expect_plan[0] * expect_plan[1]
    assert plan['neighbours'] == (2, 2, 2)
    b1, b2 = expect_plan[:2]
    # the cell of the one-label clump: its points see more than 256 points of that label's
    # block around them (the kernel walks them in more than one pass of 256 lanes) ...
    in_block = label // b2 == heavy // b2
    seen = around(cell_occupancy(pos[in_block], BOX, plan['cells']), plan['neighbours'])
    have = cell_occupancy(pos[label // b1 == heavy // b1], BOX, plan['cells']) > 0
    if n >= 3000:
        assert seen[have].max() > 256
        # ... and the clump's label lies in the second block of side 1 where there is one
        assert expect_plan[2] == 1 or heavy // b1 >= 1
    groups = split_by_label(pos, label, n_labels)
    zeros = np.zeros(len(other), dtype=np.int64)
    if kind == 'rp':
        rp_bins = edges(bins[0])
        got = corrfunc.pair_count_matrix(groups, rp_bins, REACH, BOX)
        expect = oracle.pair_count_rppi(pos, None, BOX, rp_bins, REACH, label1=label,
                                        n_labels=n_labels)
        cross = corrfunc.pair_count_matrix(groups, rp_bins, REACH, BOX, sample2=other)
        expect_cross = oracle.pair_count_rppi(pos, other, BOX, rp_bins, REACH, label1=label,
                                              label2=zeros, n_labels=n_labels)[..., 0]
    else:
        s_bins = edges(bins[0])
        got = corrfunc.pair_count_matrix_smu(groups, s_bins, bins[1], BOX)
        expect = oracle.pair_count_smu(pos, None, BOX, s_bins, bins[1], label1=label,
                                       n_labels=n_labels)
        cross = corrfunc.pair_count_matrix_smu(groups, s_bins, bins[1], BOX, sample2=other)
        expect_cross = oracle.pair_count_smu(pos, other, BOX, s_bins, bins[1], label1=label,
                                             label2=zeros, n_labels=n_labels)[..., 0]
    print('PLAN', case, 'served: %d pairs auto, %d cross' % (got.sum(), cross.sum()))
    assert got.dtype == np.uint64 and got.shape == bins + (n_labels, n_labels)
    assert expect.sum() > 10000 and expect_cross.sum() > 10000
    assert np.array_equal(got, expect), int(np.sum(got != expect))
    assert np.array_equal(cross, expect_cross), int(np.sum(cross != expect_cross))


def test_one_bin_beyond_the_labelled_maximum_is_refused_and_the_library_keeps_serving():
    """S6: 64 x 241 bins are one row more than the counters of a workgroup take."""
    from tabcorr_amd import corrfunc
    from oracle import paircount_oracle as oracle
    pos, label, _ = labelled_set(1000, 2)
    groups = split_by_label(pos, label, 2)
    with pytest.raises(ValueError, match=r'at most 15360 \(separation, mu\) bins'):
        pair_plan(BOX, REACH, REACH, 1000, 64 * 241, 2)
    with pytest.raises(ValueError, match=r'at most 15360 \(separation, mu\) bins'):
        corrfunc.pair_count_matrix_smu(groups, edges(64), 241, BOX)
    s_bins = edges(5)
    assert np.array_equal(
        corrfunc.pair_count_matrix_smu(groups, s_bins, 7, BOX),
        oracle.pair_count_smu(pos, None, BOX, s_bins, 7, label1=label, n_labels=2))


def labelled_call(kind, pos1, label1, pos2, label2, n_labels, box, bins, second):
    """tc_pair_count_rppi_labelled (second = pi_max) / tc_pair_count_smu_labelled (second =
    n_mu) as tabcorr_amd/corrfunc.py calls them, with labels on both samples."""
    from tabcorr_amd import _lib
    lib = _lib.load()
    _lib.require_device()
    pos1 = _lib.contiguous(pos1)
    pos2 = _lib.contiguous(pos2)
    label1 = np.ascontiguousarray(label1, dtype=np.int32)
    label2 = np.ascontiguousarray(label2, dtype=np.int32)
    box = _lib.contiguous(np.broadcast_to(np.asarray(box, dtype=np.float64), (3, )))
    bins = _lib.contiguous(bins)
    n_bins = len(bins) - 1
    int32_p, uint64_p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)
    points = (_lib.as_double_p(pos1), label1.ctypes.data_as(int32_p), len(pos1),
              _lib.as_double_p(pos2), label2.ctypes.data_as(int32_p), len(pos2), n_labels,
              _lib.as_double_p(box), _lib.as_double_p(bins), n_bins)
    if kind == 'rp':
        counts = np.zeros((n_bins, n_labels, n_labels), dtype=np.uint64)
        _lib.check(lib.tc_pair_count_rppi_labelled(*points, float(second),
                                                   counts.ctypes.data_as(uint64_p)))
    else:
        counts = np.zeros((n_bins, int(second), n_labels, n_labels), dtype=np.uint64)
        _lib.check(lib.tc_pair_count_smu_labelled(*points, int(second),
                                                  counts.ctypes.data_as(uint64_p)))
    return counts


@pytest.mark.parametrize('case', ['L3', 'S1'])
def test_two_labelled_samples(case):
    """The C entry points take labels on both samples (the Python wrappers always label the
    second sample 0): the full (..., L, L) array against the oracle, the samples swapped
    (the transpose), and points in arbitrary order instead of grouped by label."""
    from oracle import paircount_oracle as oracle
    kind, bins, n_labels, expect_plan, n = LABELLED_CASES[case]
    pos1, label1, _ = labelled_set(n, n_labels)
    rng = np.random.default_rng(7)
    pos2 = plain_set(1500, seed=3)
    label2 = rng.integers(0, n_labels, len(pos2))
    label2[:200] = n_labels - 1           # the partial last block of side 2 carries load
    assert pair_plan(BOX, REACH, REACH, n, int(np.prod(bins)), n_labels)['plan'] == expect_plan
    # (neither sample arrives grouped by label: both are in the order they were drawn in)
    assert np.any(np.diff(label1) < 0) and np.any(np.diff(label2) < 0)
    bin_edges = edges(bins[0])
    second = REACH if kind == 'rp' else bins[1]
    got = labelled_call(kind, pos1, label1, pos2, label2, n_labels, BOX, bin_edges, second)
    if kind == 'rp':
        expect = oracle.pair_count_rppi(pos1, pos2, BOX, bin_edges, REACH, label1=label1,
                                        label2=label2, n_labels=n_labels)
    else:
        expect = oracle.pair_count_smu(pos1, pos2, BOX, bin_edges, bins[1], label1=label1,
                                       label2=label2, n_labels=n_labels)
    assert expect.sum() > 10000 and np.count_nonzero(expect[..., n_labels - 1]) > 10
    assert np.array_equal(got, expect), int(np.sum(got != expect))
    swapped = labelled_call(kind, pos2, label2, pos1, label1, n_labels, BOX, bin_edges, second)
    assert np.array_equal(swapped, np.swapaxes(expect, -1, -2))
    order1, order2 = np.argsort(label1, kind='stable'), np.argsort(label2, kind='stable')
    grouped = labelled_call(kind, pos1[order1], label1[order1], pos2[order2], label2[order2],
                            n_labels, BOX, bin_edges, second)
    assert np.array_equal(grouped, expect)


def with_clump(rng, n, box, centre, n_clump, sigma):
    """n points: a tight clump of n_clump around `centre`, the rest uniform."""
    box = np.asarray(box, dtype=np.float64)
    pos = np.vstack([np.asarray(centre) + rng.normal(0.0, sigma, (n_clump, 3)),
                     rng.uniform(0.0, 1.0, (n - n_clump, 3)) * box])
    return np.ascontiguousarray(np.mod(pos, box))


def check_all_counts(pos1, pos2, box, first_edges=(0.0, 0.3), n_labels=5, smu=True, seed=5):
    """Unlabelled r_p-pi and s-mu counts and the labelled r_p count, auto and cross, for
    every first bin edge, against the oracle."""
    from tabcorr_amd import corrfunc
    from oracle import paircount_oracle as oracle
    label = np.random.default_rng(seed).integers(0, n_labels, len(pos1))
    groups = split_by_label(pos1, label, n_labels)
    zeros = np.zeros(len(pos2), dtype=np.int64)
    for first in first_edges:
        bins = np.array([first, 0.7, 1.5, 4.0, 9.0, 14.0, REACH])
        for other in (None, pos2):
            got = corrfunc.pair_count_rppi(pos1, bins, REACH, other, box)
            expect = oracle.pair_count_rppi(pos1, other, box, bins, REACH)
            assert got.shape == (6, 20) and expect.sum() > 10000
            assert np.array_equal(got, expect), ('rp', first, other is None)
            if smu:
                got = corrfunc.pair_count_smu(pos1, bins, 7, other, box)
                expect = oracle.pair_count_smu(pos1, other, box, bins, 7)
                assert np.array_equal(got, expect), ('smu', first, other is None)
            got = corrfunc.pair_count_matrix(groups, bins, REACH, box, sample2=other)
            expect = oracle.pair_count_rppi(
                pos1, other, box, bins, REACH, label1=label,
                label2=None if other is None else zeros, n_labels=n_labels)
            assert np.array_equal(got, expect if other is None else expect[..., 0]), \
                ('labelled', first, other is None)


# grid: (box, points, clump, cells, neighbours)
COARSE_GRIDS = {
    '4x4x4': ((100.0, 100.0, 100.0), 900, 600, (4, 4, 4), (1, 1, 1)),
    # (512 points or more in this box give four cells per axis: a clump of 600 is not possible
    # on 3 x 3 x 3 cells of it; the smaller box below has one)
    '3x3x3 of 200 points': ((100.0, 100.0, 100.0), 200, 150, (3, 3, 3), (1, 1, 1)),
    '3x3x3': ((70.0, 70.0, 70.0), 900, 600, (3, 3, 3), (1, 1, 1)),
    '4x4x1': ((100.0, 100.0, 45.0), 900, 600, (4, 4, 1), (1, 1, 0)),
}


@pytest.mark.parametrize('grid', sorted(COARSE_GRIDS))
def test_27_neighbour_grids_with_a_cell_of_three_tiles(grid):
    """Cells a full reach wide with one neighbour per side (boxes of three or four reaches, or
    fewer than ~1000 points), and one cell along z: a clump of 600 points in one cell is three
    work items of the unlabelled kernel and three LDS tiles of its neighbours."""
    box, n, n_clump, cells, neighbours = COARSE_GRIDS[grid]
    plan = pair_plan(box, REACH, REACH, n, 6 * 20)
    assert plan['cells'] == cells and plan['neighbours'] == neighbours, plan
    assert pair_plan(box, REACH, REACH, n, 6, 5)['plan'] == (5, 5, 1, 1)
    rng = np.random.default_rng(41)
    width = np.array(box) / np.array(cells)
    centre = width * np.minimum(1, np.array(cells) - 1) + 0.5 * width    # the middle of a cell
    pos1 = with_clump(rng, n, box, centre, n_clump, 1.0)
    pos2 = with_clump(rng, n, box, centre + 1.0, n_clump - 40, 1.0)
    if n_clump == 600:
        assert cell_occupancy(pos1, box, cells).max() > 512
        assert cell_occupancy(pos2, box, cells).max() > 512
    check_all_counts(pos1, pos2, box)


@pytest.mark.parametrize('kind', ['rp', 'smu'])
def test_cells_of_several_tiles_in_a_125_neighbour_grid(kind):
    """8 x 8 x 8 cells with two neighbours per side (the wrap shortcut on): clumps of 700, 513
    and 257 points in one cell each are 3, 3 and 2 work items (the last of one point) and as
    many tiles; the second sample has 300 points (two tiles) where the first clump is."""
    from tabcorr_amd import corrfunc
    from oracle import paircount_oracle as oracle
    box = np.array([120.0, 120.0, 120.0])
    reach = 25.0
    rng = np.random.default_rng(43)
    centres = np.array([[37.5, 52.5, 67.5], [112.5, 7.5, 52.5], [7.5, 112.5, 112.5]])
    pos1 = np.vstack([with_clump(rng, 5000 - 513 - 257, box, centres[0], 700, 0.4),
                      centres[1] + rng.normal(0.0, 0.4, (513, 3)),
                      centres[2] + rng.normal(0.0, 0.4, (257, 3))])
    pos2 = with_clump(rng, 3000, box, centres[0], 300, 0.4)
    plan = pair_plan(box, reach, reach, 5000, 12 * 25)
    assert plan['cells'] == (8, 8, 8) and plan['neighbours'] == (2, 2, 2), plan
    filled = np.sort(cell_occupancy(pos1, box, plan['cells']).ravel())[::-1]
    assert filled[0] >= 700 and 513 <= filled[1] < 700 and 257 <= filled[2] < 512
    assert 300 <= cell_occupancy(pos2, box, plan['cells']).max() <= 512
    bins = np.logspace(-1, np.log10(reach), 13)
    bins[-1] = reach
    for a, b in ((pos1, None), (pos1, pos2), (pos2, pos1)):
        if kind == 'rp':
            got = corrfunc.pair_count_rppi(a, bins, reach, b, box)
            expect = oracle.pair_count_rppi(a, b, box, bins, reach)
        else:
            got = corrfunc.pair_count_smu(a, bins, 9, b, box)
            expect = oracle.pair_count_smu(a, b, box, bins, 9)
        assert expect.sum() > 100000
        assert np.array_equal(got, expect), (kind, b is None, int(np.sum(got != expect)))


@pytest.mark.parametrize('box', [(50.0, 60.0, 70.0), (70.0, 50.0, 60.0), (60.0, 70.0, 50.0)])
def test_wrap_shortcut_with_5_6_and_7_cells_along_every_axis(box):
    """With fewer than seven cells along an axis the 5-cell neighbourhood reaches across half
    the box and every separation takes the minimum image; with seven, only the neighbours on
    the other side of a face do.  5, 6 and 7 cells on every axis in turn, points exactly on
    all six faces, and pairs that straddle every face just inside the reach."""
    box = np.array(box)
    rng = np.random.default_rng(47)

    def sample(n):
        pos = rng.uniform(0.0, 1.0, (n, 3)) * box
        extra = []
        for axis in range(3):
            for face in (0.0, box[axis]):
                on_face = rng.uniform(0.0, 1.0, (50, 3)) * box
                on_face[:, axis] = face
                extra.append(on_face)
            # pairs across the face: the same point but for this axis, `reach` minus a little
            # apart through the boundary, in all splits of that distance
            left = rng.uniform(0.0, 1.0, (30, 3)) * box
            right = left.copy()
            split = rng.uniform(0.0, 1.0, 30) * (REACH - 1e-7)
            split[:3] = [0.0, REACH - 1e-7, 0.5 * (REACH - 1e-7)]
            left[:, axis] = box[axis] - split
            right[:, axis] = (REACH - 1e-7) - split
            extra += [left, right]
        return np.ascontiguousarray(np.vstack([pos] + extra))

    pos1, pos2 = sample(3000), sample(2000)
    cells = tuple(int(v) for v in box // 10)
    assert sorted(cells) == [5, 6, 7]
    plan = pair_plan(box, REACH, REACH, len(pos1), 6 * 20)
    assert plan['cells'] == cells and plan['neighbours'] == (2, 2, 2), plan
    occupancy = cell_occupancy(pos1, box, cells)
    for axis in range(3):       # points in the first and in the last layer of cells
        layers = np.moveaxis(occupancy, axis, 0)
        assert layers[0].sum() > 50 and layers[-1].sum() > 50
    check_all_counts(pos1, pos2, box, first_edges=(0.0, ))


def test_bin_limits_of_the_unlabelled_count():
    """64 r_p bins (the most) x 192 pi bins are exactly the 48 KB of counters a workgroup
    takes, with a pi_max that is no whole number; one bin; and the refusals one past either
    limit, after which the library keeps serving."""
    from tabcorr_amd import corrfunc
    from oracle import paircount_oracle as oracle
    pos1, _, _ = labelled_set(3500, 50)
    pos2 = plain_set(3000)
    rp_bins = edges(64)
    pi_max = 19.3
    assert pair_plan(BOX, REACH, pi_max, 3500, 64 * 192)['lds_bytes'] == 48 * 1024
    for other in (None, pos2):
        got = corrfunc.pair_count_rppi(pos1, rp_bins, pi_max, other, BOX, n_pi=192)
        expect = oracle.pair_count_rppi(pos1, other, BOX, rp_bins, pi_max, n_pi=192)
        assert got.shape == (64, 192) and expect.sum() > 100000
        assert np.array_equal(got, expect), int(np.sum(got != expect))
        one = np.array([0.5, REACH])
        got = corrfunc.pair_count_rppi(pos1, one, pi_max, other, BOX, n_pi=1)
        assert got.shape == (1, 1)
        assert np.array_equal(got, oracle.pair_count_rppi(pos1, other, BOX, one, pi_max, n_pi=1))
    with pytest.raises(ValueError, match='between 1 and 64 r_p bins'):
        corrfunc.pair_count_rppi(pos1, edges(65), pi_max, None, BOX, n_pi=2)
    with pytest.raises(ValueError, match='at most 12288 two-dimensional bins'):
        pair_plan(BOX, REACH, pi_max, 3500, 64 * 193)
    with pytest.raises(ValueError, match='at most 12288 two-dimensional bins'):
        corrfunc.pair_count_rppi(pos1, rp_bins, pi_max, None, BOX, n_pi=193)
    few = edges(7)
    assert np.array_equal(corrfunc.pair_count_rppi(pos1, few, pi_max, pos2, BOX),
                          oracle.pair_count_rppi(pos1, pos2, BOX, few, pi_max))


def test_cylinders_beyond_48_kb_of_lds():
    """mass_in_cylinders keeps (radii, 256) doubles in LDS: 24 radii are exactly the 48 KB
    every kernel may ask for, from 25 on the kernel's limit is raised first, 65 (the most)
    take 133 KB; then 25 again with the limit already raised.  600 objects, more than 256 of
    them in one cell column (two work items), 4000 particles.  Equal masses are counts
    (exact); per-particle masses are sums in another order than the oracle's (1e-12, as
    test_mass_in_cylinders_and_mean_delta_sigma)."""
    from tabcorr_amd import corrfunc
    from oracle import paircount_oracle as oracle
    rng = np.random.default_rng(53)
    objects = with_clump(rng, 600, BOX, [50.0, 50.0, 50.0], 300, 1.0)
    particles = np.vstack([with_clump(rng, 3950, BOX, [50.0, 50.0, 20.0], 1500, 4.0),
                           objects[:50]])                     # separation exactly 0
    weights = rng.uniform(0.5, 2.0, len(particles))
    plan = pair_plan(BOX, REACH, BOX[2], 4000, 1)
    assert plan['cells'] == (7, 7, 1) and plan['neighbours'] == (2, 2, 0), plan
    assert cell_occupancy(objects, BOX, plan['cells']).max() > 256
    for n_edges in (1, 24, 25, 65, 25):
        radii = np.linspace(REACH / n_edges, REACH, n_edges)
        got = corrfunc.mass_in_cylinders(objects, particles, 2.5e9, radii, BOX)
        expect = oracle.mass_in_cylinders(objects, particles, 2.5e9, radii, BOX)
        assert got.shape == (600, n_edges) and expect[:, -1].min() > 0
        assert np.array_equal(got, expect), n_edges
        got = corrfunc.mass_in_cylinders(objects, particles, weights, radii, BOX)
        expect = oracle.mass_in_cylinders(objects, particles, weights, radii, BOX)
        np.testing.assert_allclose(got, expect, rtol=1e-12, atol=0, err_msg=str(n_edges))
    with pytest.raises(ValueError, match='between 1 and 65 radii'):
        corrfunc.mass_in_cylinders(objects, particles, 1.0, np.linspace(0.3, REACH, 66), BOX)
