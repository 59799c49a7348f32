"""csrc/fused_walk.h -- the walk of a wave of predict_fused_kernel, contract_quad_kernel or
contract_quad_f32_kernel over its part of the matrix units, and the ring of operand stages it
keeps ahead of itself -- stepped through on the host: tests/fused_walk_host.cpp compiles the
header the kernels include into a program that prints the callbacks' calls.  No device.

(The program stands alone: `c++ -std=c++17 -fsanitize=address,undefined -I tabcorr_amd/csrc
tests/fused_walk_host.cpp` and the parts on its standard input check it under the sanitizers.)
"""

import os
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, 'tabcorr_amd', 'csrc')


def compiler():
    for candidate in (os.environ.get('CXX'), 'c++', 'g++', 'clang++',
                      '/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++'):
        path = shutil.which(candidate) if candidate else None
        if path:
            return path
    raise RuntimeError('no C++ compiler')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    target = str(tmp_path_factory.mktemp('fused_walk') / 'fused_walk_host')
    subprocess.run([compiler(), '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC,
                    os.path.join(REPO, 'tests', 'fused_walk_host.cpp'), '-o', target], check=True)
    return target


def triangle_parts(n_rb, n_parts):
    """hostmath.cpp: triangle_parts -- equal shares of the units, in row-major order."""
    n_units = n_rb * (n_rb + 1) // 2
    parts = []
    for part in range(n_parts):
        begin, end = n_units * part // n_parts, n_units * (part + 1) // n_parts
        rb = 0
        while (rb + 1) * (rb + 2) // 2 <= begin:
            rb += 1
        parts.append((rb, begin - rb * (rb + 1) // 2, end - begin))
    return parts


def rectangle_parts(n_rb, n_cb, n_parts):
    """launch.hip: run_fused -- the cen-sat rectangle's shares."""
    n_units = n_rb * n_cb
    parts = []
    for part in range(n_parts):
        begin, end = n_units * part // n_parts, n_units * (part + 1) // n_parts
        parts.append((begin // n_cb, begin % n_cb, end - begin))
    return parts


def every_cut(triangular, n_rb, n_cb):
    """hostmath.h: QuadSchedule gives every resident wave an equal contiguous range of the unit
    space, so a run of contract_quad_kernel starts and ends anywhere in a row and can span a
    whole component: every (first unit, count >= 1) of the component."""
    blocks = [(rb, cb) for rb in range(n_rb) for cb in range(rb + 1 if triangular else n_cb)]
    return [blocks[first] + (count, ) for first in range(len(blocks))
            for count in range(1, len(blocks) - first + 1)]


BASES = ((0, 0), (7, 0), (3, 40))         # (unit_base, units behind the component)


def all_parts():
    """(rb0, cb0, count, triangular, n_cb, unit_base, table_units) of every case: the component
    alone in its table, last in a longer one, and followed by others."""
    out = []
    shapes = [(1, n_rb, n_rb, n_rb * (n_rb + 1) // 2, every_cut(1, n_rb, n_rb))
              for n_rb in (1, 2, 3, 4, 5)]
    shapes += [(0, n_rb, n_cb, n_rb * n_cb, every_cut(0, n_rb, n_cb))
               for n_rb, n_cb in ((3, 1), (2, 7), (3, 4))]
    for triangular, n_rb, n_cb, n_units, parts in shapes:
        for unit_base, behind in BASES:
            for rb0, cb0, count in parts:
                out.append((rb0, cb0, count, triangular, n_cb, unit_base,
                            unit_base + n_units + behind))
    for n_parts in (4, 8, 16):
        shapes = [(1, n_rb, n_rb, n_rb * (n_rb + 1) // 2, triangle_parts(n_rb, n_parts))
                  for n_rb in (1, 2, 3, 5, 9, 25)]
        shapes += [(0, n_rb, n_cb, n_rb * n_cb, rectangle_parts(n_rb, n_cb, n_parts))
                   for n_rb, n_cb in ((1, 1), (1, 13), (13, 12))]
        for triangular, n_rb, n_cb, n_units, parts in shapes:
            for unit_base, behind in BASES:
                for rb0, cb0, count in parts:
                    out.append((rb0, cb0, count, triangular, n_cb, unit_base,
                                unit_base + n_units + behind))
    return out


def expected_units(part):
    """The parent's order: (rb, cb, unit) of the part's units, row by row."""
    rb, cb, count, triangular, n_cb, unit_base, _ = part
    units = []
    for _ in range(count):
        units.append((rb, cb, unit_base + (rb * (rb + 1) // 2 + cb if triangular else rb * n_cb + cb)))
        cb += 1
        if cb == (rb + 1 if triangular else n_cb):
            rb, cb = rb + 1, 0
    return units


def run(program, parts):
    """(ring depth, the calls of every part)."""
    text = ''.join(' '.join(str(v) for v in part[:6]) + '\n' for part in parts)
    out = subprocess.run([program], input=text, capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert out[0].split()[0] == 'depth'
    logs, current = [], []
    for line in out[1:]:
        if line == 'done':
            logs.append(current)
            current = []
        else:
            current.append(line.split())
    assert len(logs) == len(parts)
    return int(out[0].split()[1]), logs


def check_part(part, log, depth):
    count, table_units = part[2], part[6]
    units = expected_units(part)
    if count == 0:
        assert log == [], 'a part without units touches nothing'
        return
    stages = {}             # stage -> (unit, column, inside) requested and not yet consumed
    requested = []          # units asked for, in order
    consumed = 0
    row_open = None         # block row between its row_begin and row_end
    first_of_row = True
    for entry in log:
        kind, values = entry[0], [int(v) for v in entry[1:]]
        if kind == 'R':
            stage, unit, column, inside = values
            assert 0 <= stage < depth
            assert stage not in stages, 'stage %d requested twice' % stage
            # (one unit behind the table at most: the bounds check of the buffer resource, whose
            # size is the table's, answers a whole unit behind it with zeros)
            assert unit <= table_units, 'a request beyond what the bounds check absorbs'
            index = len(requested)
            assert unit == units[0][2] + index, 'consecutive units'
            if index < count:
                assert inside and column == units[index][1]
            else:
                # nobody consumes it: the unit behind the part, block column 0
                assert not inside and column == 0 and index == count
            stages[stage] = (unit, column, inside)
            requested.append(unit)
        elif kind == 'B':
            assert row_open is None and values[0] == units[consumed][0]
            assert first_of_row
            row_open = values[0]
        elif kind == 'C':
            stage, first, rb, cb = values
            assert (rb, cb) == units[consumed][:2], 'the parent\'s order'
            assert stage in stages, 'stage %d consumed before it was requested' % stage
            unit, column, inside = stages.pop(stage)
            assert inside and (unit, column) == (units[consumed][2], cb)
            assert row_open == rb
            assert bool(first) == first_of_row
            if first:
                assert stage == 0, 'every row begins in stage 0'
            # the ring's depth: the next unit is asked for before this one is consumed
            assert len(requested) >= min(count, consumed + depth)
            first_of_row = False
            consumed += 1
        elif kind == 'M':
            assert 0 not in stages and 1 in stages, 'a move of what was requested into a free stage'
            stages[0] = stages.pop(1)
        elif kind == 'E':
            assert row_open == values[0] == units[consumed - 1][0]
            # ... at the last unit the part has in the row
            assert consumed == count or units[consumed][0] == values[0] + 1
            row_open = None
            first_of_row = True
        else:
            raise AssertionError(entry)
    assert consumed == count, 'every unit once'
    assert row_open is None, 'the last row is closed'
    assert len(requested) == count + depth - 1
    assert all(not inside for _, _, inside in stages.values())
    # row ends: one per block row the part touches
    rows = sorted({rb for rb, _, _ in units})
    assert [int(e[1]) for e in log if e[0] == 'E'] == rows
    assert [int(e[1]) for e in log if e[0] == 'B'] == rows


def test_walk_visits_the_parents_units_through_the_ring(program):
    parts = all_parts()
    # the cases the walk's corners need are among them
    assert {0, 1, 2, 3} <= {p[2] for p in parts}
    assert any(p[1] > 0 and p[2] > 1 for p in parts), 'a part that starts inside a row'
    assert any(p[3] and p[0] == 0 and p[2] >= 3 for p in parts), 'rows of one unit'
    # ... and every cut of the quadratic-form schedule's small components
    assert {(0, 0, 15, 1, 5), (4, 4, 1, 1, 5), (1, 6, 1, 0, 7), (0, 3, 9, 0, 4)} <= {
        p[:5] for p in parts}
    depth, logs = run(program, parts)
    assert depth == 2
    for part, log in zip(parts, logs):
        check_part(part, log, depth)


def test_parts_cover_their_component_once(program):
    """The parts of a component, one after the other, are its units in table order."""
    for n_parts in (4, 8, 16):
        for n_rb in (1, 2, 3, 5, 9, 25):
            parts = [(rb0, cb0, count, 1, n_rb, 0, n_rb * (n_rb + 1) // 2)
                     for rb0, cb0, count in triangle_parts(n_rb, n_parts)]
            seen = []
            for log in run(program, parts)[1]:
                seen += [(int(e[3]), int(e[4])) for e in log if e[0] == 'C']
            assert seen == [(rb, cb) for rb in range(n_rb) for cb in range(rb + 1)]
