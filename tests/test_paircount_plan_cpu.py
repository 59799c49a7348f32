"""CPU tests of what the pair counter plans before it launches (tabcorr_amd/csrc/hostmath.h:
make_cell_grid, plan_label_blocks, through tc_debug_pair_plan -- no device needed): the cell
grid of a box and the cut of the labels into blocks whose (bin, label 1, label 2) counters fit
a workgroup's LDS.  tests/test_gpu_paircount_plans.py runs these plans on the GPU; here the
plans themselves are pinned, so that a change of the sizing shows up as such."""

import sys

import numpy as np
import pytest

from util import REPO, pair_plan

sys.path.insert(0, REPO)

BUDGET = 30 * 1024 // 4       # counters a workgroup should stay within (hostmath.h)
LIMIT = 60 * 1024 // 4        # ... and must stay within: the documented 15 360 bins

# name: (n_bin, n_labels, (labels per block 1, 2, blocks 1, 2)); the labelled cases of
# tests/test_gpu_paircount_plans.py
LABELLED_PLANS = {
    'L1': (19, 50, (50, 8, 1, 7)),            # last block of sample 2: 2 labels
    'L2': (64, 70, (35, 2, 2, 35)),
    'L3': (64, 71, (36, 2, 2, 36)),           # both last blocks partial (35 and 1 labels)
    'S1': (8 * 10, 51, (26, 2, 2, 26)),
    'S2': (60 * 64, 3, (1, 2, 3, 2)),         # exactly the budget
    'S3': (60 * 120, 3, (1, 2, 3, 2)),        # over the budget, nothing left to shrink
    'S4': (64 * 121, 3, (1, 1, 3, 3)),        # the third loop: over the limit with two labels
    'S5': (64 * 240, 2, (1, 1, 2, 2)),        # the documented maximum
}
# the plans the existing labelled tests produce (tests/test_gpu_paircount.py): one block on
# the side of sample 1, every one of them
OLD_PLANS = {(10, 6): (6, 6, 1, 1), (48, 6): (6, 6, 1, 1), (7, 4): (4, 4, 1, 1),
             (12, 3): (3, 3, 1, 1), (5, 8): (8, 8, 1, 1), (19, 100): (100, 4, 1, 25)}


@pytest.fixture(scope='module', autouse=True)
def library():
    from tabcorr_amd import build
    build.build()


@pytest.mark.parametrize('case', sorted(LABELLED_PLANS))
def test_label_block_plans_of_the_gpu_cases(case):
    n_bin, n_labels, expect = LABELLED_PLANS[case]
    got = pair_plan(100.0, 20.0, 20.0, 3500, n_bin, n_labels)
    assert got['plan'] == expect, (case, got)
    assert got['lds_bytes'] == 4 * n_bin * expect[0] * expect[1]
    assert got['lds_bytes'] <= 4 * LIMIT
    # 3500 points in a box of 100^3 with a reach of 20: 7 cells of 14.3, two neighbours
    assert got['cells'] == (7, 7, 7) and got['neighbours'] == (2, 2, 2)


def test_label_block_plans_of_the_older_tests_have_one_block_on_side_one():
    for (n_bin, n_labels), expect in OLD_PLANS.items():
        assert pair_plan(100.0, 20.0, 20.0, 5000, n_bin, n_labels)['plan'] == expect
        assert expect[2] == 1


def test_bins_beyond_the_counters_are_refused():
    assert pair_plan(100.0, 20.0, 20.0, 1000, LIMIT, 2)['lds_bytes'] == 4 * LIMIT
    with pytest.raises(ValueError, match=r'at most 15360 \(separation, mu\) bins'):
        pair_plan(100.0, 20.0, 20.0, 1000, 64 * 241, 2)
    # unlabelled: 48 KB of counters
    plan = pair_plan(100.0, 20.0, 20.0, 1000, 64 * 192)
    assert plan['lds_bytes'] == 48 * 1024 and plan['plan'] == (0, 0, 0, 0)
    with pytest.raises(ValueError, match='at most 12288 two-dimensional bins'):
        pair_plan(100.0, 20.0, 20.0, 1000, 64 * 193)
    assert pair_plan(100.0, 20.0, 20.0, 1000, 1)['lds_bytes'] == 4
    with pytest.raises(ValueError):
        pair_plan(100.0, 20.0, 20.0, 1000, 0)
    with pytest.raises(ValueError):
        pair_plan(100.0, 20.0, 20.0, 1000, 10, 4097)


def test_label_block_plans_cover_the_labels_and_fit_the_lds():
    named = [19, 64, 80, 3840, 6782, 6783, 7200, 7680, 7681, 7744, 13564, 13565, 15359, 15360,
             1, 2, 12288]
    sweep = sorted(set(np.unique(np.geomspace(1, LIMIT, 120).astype(int)).tolist() + named))
    seen_third_loop = seen_over_budget = 0
    for n_bin in sweep:
        for n_labels in (1, 2, 3, 7, 8, 9, 50, 51, 70, 71, 100, 4096):
            got = pair_plan(100.0, 20.0, 20.0, 3000, n_bin, n_labels)
            b1, b2, blocks1, blocks2 = got['plan']
            what = (n_bin, n_labels, got['plan'])
            assert 1 <= b1 <= n_labels and 1 <= b2 <= min(n_labels, 8), what
            # both block counts cover all labels, with no block left empty
            assert (blocks1 - 1) * b1 < n_labels <= blocks1 * b1, what
            assert (blocks2 - 1) * b2 < n_labels <= blocks2 * b2, what
            counters = n_bin * b1 * b2
            assert got['lds_bytes'] == 4 * counters
            assert counters <= LIMIT, what
            assert counters <= BUDGET or (b1 == 1 and b2 <= 2), what
            # nothing is cut finer than the budget asks for: sample 1 keeps all its labels
            # unless sample 2 is down to blocks of 2, and blocks of one label on side 2 only
            # where two would not fit at all
            if b1 < n_labels:
                assert b2 <= 2 and n_bin * min(2 * b1, n_labels) * 2 > BUDGET, what
            if b2 == 1 and n_labels > 1:
                assert b1 == 1 and n_bin * 2 > LIMIT, what
                seen_third_loop += 1
            seen_over_budget += counters > BUDGET
    assert seen_third_loop > 10 and seen_over_budget > 10


# (box, reach in the plane, reach along z, points): cells, neighbours -- the grids of
# tests/test_gpu_paircount_plans.py
GRIDS = [
    ((100.0, 100.0, 100.0), 20.0, 20.0, 900, (4, 4, 4), (1, 1, 1)),
    ((100.0, 100.0, 100.0), 20.0, 20.0, 200, (3, 3, 3), (1, 1, 1)),
    ((100.0, 100.0, 45.0), 20.0, 20.0, 900, (4, 4, 1), (1, 1, 0)),
    ((50.0, 60.0, 70.0), 20.0, 20.0, 3000, (5, 6, 7), (2, 2, 2)),
    ((70.0, 50.0, 60.0), 20.0, 20.0, 3000, (7, 5, 6), (2, 2, 2)),
    ((60.0, 70.0, 50.0), 20.0, 20.0, 3000, (6, 7, 5), (2, 2, 2)),
    ((120.0, 120.0, 120.0), 25.0, 25.0, 5000, (8, 8, 8), (2, 2, 2)),
    # the existing tests' grids: 3-D cases 8 x 8 x 6 and the flat box 7 x 1 x 1
    ((120.0, 120.0, 120.0), 25.0, 40.0, 5000, (8, 8, 6), (2, 2, 2)),
    ((200.0, 60.0, 90.0), 25.0, 40.0, 4000, (7, 1, 1), (2, 0, 0)),
]


@pytest.mark.parametrize('box, reach_xy, reach_z, n, cells, neighbours', GRIDS)
def test_cell_grids_of_the_gpu_cases(box, reach_xy, reach_z, n, cells, neighbours):
    got = pair_plan(box, reach_xy, reach_z, n, 10)
    assert got['cells'] == cells and got['neighbours'] == neighbours, got


def test_cell_grids_hold_the_partners_in_the_neighbour_cells():
    """Along an axis: cells at least reach / neighbours wide (reach / 2 with two neighbour
    cells per side, reach with one), one cell exactly where there are no neighbour offsets,
    neighbours that are distinct cells, and no more cells than the points warrant."""
    rng = np.random.default_rng(1)
    boxes = [(100.0, 100.0, 100.0), (50.0, 60.0, 70.0), (200.0, 60.0, 90.0), (41.0, 1000.0, 45.0)]
    boxes += [tuple(rng.uniform(30.0, 400.0, 3)) for _ in range(20)]
    taken = set()
    for box in boxes:
        for reach_xy, reach_z in ((20.0, 20.0), (25.0, 40.0), (3.0, 7.5), (14.9, 12.0)):
            if reach_xy >= 0.5 * min(box[:2]) or reach_z >= 0.5 * box[2]:
                continue
            for n in (1, 2, 200, 900, 1000, 3000, 4096, 10**5, 10**8, 10**9):
                got = pair_plan(box, reach_xy, reach_z, n, 10)
                cap = max(3, int(np.cbrt(n / 8.0) + 1e-9))
                for axis in range(3):
                    reach = reach_z if axis == 2 else reach_xy
                    cells, nb = got['cells'][axis], got['neighbours'][axis]
                    what = (box, reach, n, axis, cells, nb)
                    assert nb in (0, 1, 2) and (cells == 1) == (nb == 0), what
                    assert cells >= 2 * nb + 1 and cells <= min(cap, 256), what
                    if nb:
                        assert box[axis] / cells >= reach / nb, what
                    taken.add(nb)
    assert taken == {0, 1, 2}
