"""csrc/fused_skip.h, the sharing rules -- the list of items from which the waves of
predict_fused_kernel take their last r pass (option "fused_share"), and the mask bits by which an
item of one group leaves the other group out of a part's walk -- stepped through on the host:
tests/fused_share_host.cpp compiles the header the kernel includes (and csrc/fused_walk.h) into a
program.  No device.

(The program stands alone; test_program_is_clean_under_the_sanitizers builds it with
`-fsanitize=address,undefined` and runs it directly on the same commands.)
"""

import os
import subprocess

import numpy as np
import pytest

from test_fused_skip_cpu import patterns, tile_densities
from test_fused_walk_cpu import CSRC, compiler, triangle_parts
from util import REPO

SOURCE = os.path.join(REPO, 'tests', 'fused_share_host.cpp')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    target = str(tmp_path_factory.mktemp('fused_share') / 'fused_share_host')
    subprocess.run([compiler(), '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, SOURCE,
                    '-o', target], check=True)
    return target


def run(program, text):
    return subprocess.run([program], input=text, capture_output=True, text=True,
                          check=True).stdout.splitlines()


def items_of(lines):
    """lines of one `items` command -> (count, [(index, tile, part, select)])."""
    assert lines[0].split()[0] == 'count'
    count = int(lines[0].split()[1])
    items = [tuple(int(w) for w in line.split()[1:]) for line in lines[1:1 + count]]
    assert all(line.split()[0] == 'item' for line in lines[1:1 + count])
    return count, items


def test_every_tile_part_and_group_is_covered_exactly_once(program):
    for share, count in ((0, 0), (1, 8), (2, 16)):
        lines = run(program, 'items %d\n' % share)
        got, items = items_of(lines)
        assert got == count and len(lines) == 1 + count
        assert [item[0] for item in items] == list(range(count))
        if share == 0:
            continue
        covered = []
        for _, tile, part, select in items:
            assert tile in (0, 1) and 0 <= part < 4
            assert select == 0 if share == 1 else select in (1, 2)
            covered += [(tile, part, g) for g in range(2) if select in (0, 1 + g)]
        assert sorted(covered) == [(tile, part, g) for tile in range(2) for part in range(4)
                                   for g in range(2)], 'share %d' % share
        # the heaviest expected first: the first part of both tiles, then the parts 3, 2 and 1
        parts = [part for _, _, part, _ in items]
        per_job = count // 8
        assert parts == [p for p in (0, 3, 2, 1) for _ in range(2 * per_job)]
        assert [tile for _, tile, _, _ in items] == [t for _ in range(4) for t in (0, 1)
                                                     for _ in range(per_job)]
    # any other value of the option shares nothing
    assert items_of(run(program, 'items 3\n'))[0] == 0
    assert items_of(run(program, 'items -1\n'))[0] == 0


def walk_cases():
    rng = np.random.default_rng(11)
    cases, text = [], []
    for n_rb in (1, 2, 3, 6, 25):
        for index, pattern in enumerate(patterns(n_rb, rng)):
            dens = tile_densities(n_rb, pattern, rng)
            for rb0, cb0, count in triangle_parts(n_rb, 4):
                for select in (0, 1, 2):
                    for guard in (1, 0):
                        cases.append((n_rb, rb0, cb0, count, pattern, select, guard))
                        text.append('walk %d %d %d %d %d 1 %d %d ' %
                                    (select, guard, rb0, cb0, count, n_rb, n_rb) +
                                    ' '.join(str(v) for v in dens.ravel()) + '\n')
    return cases, ''.join(text)


def logs_of(lines):
    logs, current = [], []
    for line in lines:
        if line == 'done':
            logs.append(current)
            current = []
        else:
            current.append(line.split())
    assert not current
    return logs


def test_selection_bits_leave_the_other_group_out(program):
    cases, text = walk_cases()
    logs = logs_of(run(program, text))
    assert len(logs) == len(cases)
    for (n_rb, rb0, cb0, count, pattern, select, guard), log in zip(cases, logs):
        units, rb, cb = [], rb0, cb0
        for _ in range(count):
            units.append((rb, cb))
            cb += 1
            if cb == rb + 1:
                rb, cb = rb + 1, 0
        own = [g for g in range(2) if select in (0, 1 + g)]
        other = [g for g in range(2) if g not in own]
        issued = [(int(e[1]), int(e[2]), int(e[3])) for e in log if e[0] == 'P']
        assert len(set(issued)) == len(issued), 'no product twice'
        expected = {(rb, cb, g) for rb, cb in units for g in own
                    if not (guard and (pattern[rb, g] or pattern[cb, g]))}
        assert set(issued) == expected, 'the item\'s own groups, less the zero blocks if guarded'
        # the other group: no product, no cleared accumulator, no row end
        for kind in 'PCE':
            assert not [e for e in log if e[0] == kind and int(e[-1]) in other], (kind, select)
        sums = {(int(e[1]), int(e[2])): int(e[3]) for e in log if e[0] == 'F'}
        dense = {(int(e[1]), int(e[2])): int(e[3]) for e in log if e[0] == 'G'}
        assert len(sums) == 32 and len(dense) == 32
        for g in own:
            assert all(sums[g, c] == dense[g, c] for c in range(16)), 'the sums of its own draws'
        for g in other:
            assert all(sums[g, c] == 0 for c in range(16)), 'the other group\'s are not touched'
    # the two items of a job together are the job: every product once, every draw's sum once
    by_job = {}
    for case, log in zip(cases, logs):
        key = (case[0], case[1], case[2], case[3], id(case[4]), case[6])
        by_job.setdefault(key, {})[case[5]] = sorted(tuple(e) for e in log if e[0] == 'P')
    for halves in by_job.values():
        assert sorted(halves[1] + halves[2]) == halves[0]


def test_program_is_clean_under_the_sanitizers(tmp_path):
    target = str(tmp_path / 'fused_share_host_sanitized')
    built = subprocess.run([compiler(), '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=all', '-I', CSRC, SOURCE, '-o', target],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _, text = walk_cases()
    text = 'items 0\nitems 1\nitems 2\n' + text
    out = subprocess.run([target], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == '', out.stderr[-2000:]
    assert out.stdout.count('done') == text.count('walk')
