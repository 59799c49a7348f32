"""csrc/fused_skip.h -- where predict_fused_kernel places a workgroup's draws in its density array,
which blocks of densities count as all zero for a group of 16 draws, and which matrix products
of a part's walk that leaves out -- stepped through on the host: tests/fused_skip_host.cpp
compiles the header the kernel includes (and csrc/fused_walk.h) into a program.  No device.

(The program stands alone: `c++ -std=c++17 -fsanitize=address,undefined -I tabcorr_amd/csrc
tests/fused_skip_host.cpp` and the commands on its standard input check it under the sanitizers.)
"""

import os
import subprocess

import numpy as np
import pytest

from test_fused_walk_cpu import CSRC, compiler, triangle_parts
from util import REPO


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    target = str(tmp_path_factory.mktemp('fused_skip') / 'fused_skip_host')
    subprocess.run([compiler(), '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC,
                    os.path.join(REPO, 'tests', 'fused_skip_host.cpp'), '-o', target], check=True)
    return target


def run(program, text):
    return subprocess.run([program], input=text, capture_output=True, text=True,
                          check=True).stdout.splitlines()


def number(value):
    return repr(float(value))          # 'nan', 'inf', '-inf', '-0.0', '1e+300'


def column_of_rank(rank):
    """Ranks 16 g ... 16 g + 15 share group g: tile g // 2, the even (g % 2 == 0) or odd columns."""
    return 32 * (rank // 32) + 2 * (rank % 16) + (rank // 16) % 2


def key_sets():
    rng = np.random.default_rng(3)
    sets = {
        'random': rng.uniform(11.0, 13.0, 64),
        'ties': rng.integers(0, 4, 64) * 0.5 + 11.0,
        'all equal': np.full(64, 12.25),
        'sorted': np.linspace(10.0, 14.0, 64),
        'reversed': np.linspace(14.0, 10.0, 64),
        'linear masses': 10.0 ** rng.uniform(11.0, 13.0, 64),
    }
    special = rng.uniform(11.0, 13.0, 64)
    special[[3, 17, 40]] = np.nan
    special[[5, 41]] = np.inf
    special[[6, 63]] = -np.inf
    special[[0, 9]] = 0.0
    special[10] = -0.0
    special[11] = 1e300
    special[12] = -300.0
    sets['nan and inf'] = special
    sets['all nan'] = np.full(64, np.nan)
    return sets


def test_perm_is_a_bijection_that_groups_by_key(program):
    sets = key_sets()
    text = ''.join('perm ' + ' '.join(number(k) for k in keys) + '\n' for keys in sets.values())
    lines = run(program, text)
    assert len(lines) == len(sets)
    for (name, keys), line in zip(sets.items(), lines):
        words = line.split()
        assert words[0] == 'perm'
        columns = [int(w) for w in words[1:]]
        assert sorted(columns) == list(range(64)), name
        rank_of_column = {column_of_rank(r): r for r in range(64)}
        rank = np.array([rank_of_column[c] for c in columns])
        # NaN below everything, then by value; the key is the double's high dword without its
        # six lowest bits, so values closer than 2^-14 relative may come out in index order
        order = np.where(np.isnan(keys), -np.inf, keys)
        for i in range(64):
            for j in range(64):
                if np.isnan(keys[i]) and not np.isnan(keys[j]):
                    assert rank[i] < rank[j], name
                elif order[i] < order[j] and (
                        abs(order[j] - order[i]) > 2.0 ** -13 * max(abs(order[i]), abs(order[j]))
                        or np.isinf(order[i]) != np.isinf(order[j])):
                    assert rank[i] < rank[j], (name, i, j)
                elif keys[i] == keys[j] and i < j:
                    assert rank[i] < rank[j], 'ties break by index: %s' % name
    # what the order is for: draws of similar key share a group of 16
    columns = [int(w) for w in lines[list(sets).index('sorted')].split()[1:]]
    groups = [2 * (c // 32) + c % 2 for c in columns]
    assert groups == [d // 16 for d in range(64)]


def mask_of(dens, row0, n_blocks, tile):
    mask = 0
    for block in range(n_blocks):
        for parity in range(2):
            values = dens[row0 + 4 * block:row0 + 4 * block + 4, 32 * tile + parity:32 * tile + 32:2]
            assert values.shape == (4, 16)
            if np.all(values == 0.0):
                mask |= 1 << (2 * block + parity)
    return mask


def test_masks_mark_the_blocks_that_are_zero_for_a_whole_group(program):
    rng = np.random.default_rng(4)
    rows, n_blocks = 22, 5
    cases = []
    dens = rng.uniform(0.1, 1.0, (rows, 64))
    dens[0:4] = 0.0                       # a block zero for every group
    dens[4:8, 0:32:2] = 0.0               # ... for tile 0's even draws only
    dens[8:12, 33:64:2] = 0.0             # ... for tile 1's odd draws
    dens[12:16, 1:32:2] = 0.0             # zero for 15 of the 16 draws of a group
    dens[13, 7] = 1e-300
    dens[16:20, 32:64:2] = -0.0           # -0 counts as zero
    cases.append((dens, 0, n_blocks, {0: 0b0000000111, 1: 0b0100100011}))
    other = np.zeros((rows, 64))
    other[5, 2] = np.nan                  # NaN does not
    other[9, 35] = 1e300
    other[14, 4] = -1e-320                # nor does a subnormal
    cases.append((other, 0, n_blocks, None))
    cases.append((other, 2, n_blocks, None))      # blocks that start at another row
    cases.append((dens, 4, 4, None))
    cases.append((np.zeros((8, 64)), 0, 2, {0: 0b1111, 1: 0b1111}))
    text = ''
    for d, row0, blocks, _ in cases:
        text += 'mask %d %d %d ' % (d.shape[0], row0, blocks)
        text += ' '.join(number(v) for v in d.ravel()) + '\n'
    lines = run(program, text)
    assert len(lines) == len(cases)
    for (d, row0, blocks, known), line in zip(cases, lines):
        words = line.split()
        got = [int(words[1], 16), int(words[2], 16)]
        assert got == [mask_of(d, row0, blocks, 0), mask_of(d, row0, blocks, 1)]
        if known is not None:
            assert got == [known[0], known[1]]
    # the NaN's and the 1e300's blocks are not zero, the blocks around them are
    got = [int(w, 16) for w in lines[1].split()[1:]]
    assert got[0] == 0b1111111111 & ~(1 << 2) & ~(1 << 6) and got[1] == 0b1111111111 & ~(1 << 5)


def tile_densities(n_blocks, pattern, rng):
    """(4 n_blocks, 32) integers: `pattern` (n_blocks, 2) says which (block, group) is all zero;
    every other block has a zero here and there but not everywhere."""
    dens = rng.integers(-3, 8, (4 * n_blocks, 32))
    dens[dens == 0] = 1
    dens[rng.random(dens.shape) < 0.1] = 0
    for block in range(n_blocks):
        for g in range(2):
            view = dens[4 * block:4 * block + 4, g::2]
            if pattern[block, g]:
                view[:] = 0
            elif np.all(view == 0):
                view[0, 0] = 2
    return dens


def patterns(n_blocks, rng):
    """Zero blocks as the satellites make them (the first blocks behind the centrals', further
    for one group than for the other), at random, none, all, and the part's first blocks."""
    out = [np.zeros((n_blocks, 2), bool), np.ones((n_blocks, 2), bool)]
    zheng = np.zeros((n_blocks, 2), bool)
    first_sat = n_blocks // 2
    zheng[first_sat:first_sat + (n_blocks - first_sat + 1) // 2, 0] = True
    zheng[first_sat:n_blocks, 1] = True
    out.append(zheng)
    out.append(rng.random((n_blocks, 2)) < 0.4)
    head = np.zeros((n_blocks, 2), bool)
    head[0:max(1, n_blocks // 3), 0] = True          # the part's first rows
    head[1:2, 1] = True
    out.append(head)
    return out


def test_walk_leaves_out_the_zero_products_and_keeps_the_sums(program):
    rng = np.random.default_rng(5)
    cases, text = [], []
    for n_rb in range(1, 26):
        for index, pattern in enumerate(patterns(n_rb, rng)):
            dens = tile_densities(n_rb, pattern, rng)
            for rb0, cb0, count in triangle_parts(n_rb, 4):
                # (the whole set of patterns for the small triangles and the benchmark's 25 rows,
                # the satellites' and the first-unit pattern for all)
                if not (n_rb <= 6 or n_rb == 25 or index in (2, 4)):
                    continue
                cases.append((n_rb, rb0, cb0, count, pattern))
                text.append('walk %d %d %d 1 %d %d ' % (rb0, cb0, count, n_rb, n_rb) +
                            ' '.join(str(v) for v in dens.ravel()) + '\n')
    lines = run(program, ''.join(text))
    logs, current = [], []
    for line in lines:
        if line == 'done':
            logs.append(current)
            current = []
        else:
            current.append(line.split())
    assert len(logs) == len(cases)
    seen_first_left_out = False
    for (n_rb, rb0, cb0, count, pattern), log in zip(cases, logs):
        units, rb, cb = [], rb0, cb0
        for _ in range(count):
            units.append((rb, cb))
            cb += 1
            if cb == rb + 1:
                rb, cb = rb + 1, 0
        issued = [(int(e[1]), int(e[2]), int(e[3])) for e in log if e[0] == 'P']
        assert len(set(issued)) == len(issued), 'no product twice'
        expected = {(rb, cb, g) for rb, cb in units for g in range(2)
                    if not pattern[rb, g] and not pattern[cb, g]}
        assert set(issued) == expected, \
            'left out: exactly the products whose B block or row block is all zero'
        assert [e[:2] for e in issued] == [e[:2] for e in sorted(issued, key=lambda e: (
            units.index(e[:2]), e[2]))], 'in the walk\'s order'
        with_skips = {(e[1], e[2]): int(e[3]) for e in log if e[0] == 'F'}
        dense = {(e[1], e[2]): int(e[3]) for e in log if e[0] == 'G'}
        assert len(dense) == 32 and with_skips == dense, 'the sums of every draw'
        for g in range(2):
            for row in {rb for rb, _ in units}:
                first = min(cb for rb, cb in units if rb == row)
                later = [cb for rb, cb in units if rb == row and cb > first]
                if (not pattern[row, g] and pattern[first, g] and
                        any(not pattern[cb, g] for cb in later)):
                    seen_first_left_out = True
    assert seen_first_left_out, 'a row whose first unit is left out and a later one is not'
