"""The walk of the one-launch kernel's matrix units (csrc/fused_walk.h: the operand stages across
row ends; the two tiles' waves half a turn apart in the parts, no scheduling barriers) only moves
instructions: every form that shares fused_quad_pass returns, bit for bit, what the commit
before the change returned on an MI355X (tests/golden/fused_walk_parent.npz, recorded by
tests/golden/make_fused_walk_parent.py with that commit's library), and those recorded values
agree with the oracle at the tolerance of test_gpu_fused.py.  Needs an MI355X."""

import importlib.util
import os

import numpy as np
import pytest

from util import GOLDEN, assert_rel

pytestmark = pytest.mark.gpu

RTOL = 1e-10          # (test_gpu_fused.py)


def load_recorder():
    spec = importlib.util.spec_from_file_location(
        'make_fused_walk_parent', os.path.join(GOLDEN, 'make_fused_walk_parent.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


recorder = load_recorder()
CASES = recorder.cases()


@pytest.fixture(scope='module')
def parent():
    return recorder.unpack(np.load(recorder.FILE))


@pytest.fixture(scope='module')
def oracle_values():
    """The oracle's values per (table, draws, separated), computed once."""
    cache = {}

    def values(case):
        from oracle import tabcorr_oracle as oracle
        key = (case['n_prim'], case['n_r'], case['separate'], case['degenerate'])
        if key not in cache:
            with np.errstate(all='ignore'):
                cache[key] = oracle.predict_zheng07_batch(
                    recorder.table_of(case), recorder.theta_of(case),
                    separate_gal_type=case['separate'])
        return cache[key]
    return values


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize('name, case', CASES, ids=[name for name, _ in CASES])
def test_same_bits_as_the_parent_commit(name, case, parent, oracle_values):
    want = parent[name]
    got = recorder.run_case(case)           # (asserts that the form asked for ran)
    assert sorted(got) == sorted(want)
    assert tuple(got['launch']) == tuple(want['launch'])
    for key in want:
        if key != 'launch':
            differing = int(np.sum(got[key].view(np.uint64) != want[key].view(np.uint64)))
            assert same_bits(got[key], want[key]), '%s: %d of %d values differ from the parent\'s' % (
                key, differing, want[key].size)
    # the recorded values themselves against the oracle
    expect_ngal, expect_xi = oracle_values(case)
    # (degenerate draws: test_gpu_fused.py compares them with the three-kernel path; here the
    # regular draws beside them, in the same workgroups)
    rows = np.ones(recorder.N_DRAWS, dtype=bool)
    if case['degenerate']:
        rows[list(recorder.DEGENERATE_ROWS)] = False

    def check(got, expect, what, **kwargs):
        assert_rel(got[rows], expect[rows], RTOL, what, **kwargs)
    if case['kind'] == 'chi2':
        vector, precision = recorder.likelihood_of(case)
        delta = expect_xi - vector
        check(want['ngal'], expect_ngal, 'ngal')
        assert_rel(want['chi2'], np.einsum('bi,ij,bj->b', delta, precision, delta), 1e-9, 'chi2')
    elif case['separate']:
        for key in expect_ngal:
            check(want['ngal_' + key], expect_ngal[key], 'ngal ' + key)
        for key in expect_xi:
            check(want['xi_' + key], expect_xi[key], 'xi ' + key, floor=1e-13)
    else:
        check(want['ngal'], expect_ngal, 'ngal')
        check(want['xi'], expect_xi, 'xi')


def test_the_recorded_cases_are_the_ones_asked_for(parent):
    """81 draws; n_prim 4, 5, 10, 18 with 19 r bins and 50 with 3, 8, 12, 19 (U = 1, 2, 3, 5), each
    as 64 x 8, 32 x 8 and 64 x 16, total and separated; the likelihood; degenerate draws."""
    names = set(parent)
    assert names == {name for name, _ in CASES}
    for n_prim, n_r in [(4, 19), (5, 19), (10, 19), (18, 19), (50, 3), (50, 8), (50, 12), (50, 19)]:
        for form in ('64x8', '32x8', '64x16'):
            for kind in ('tot', 'sep'):
                assert 'p%d_r%d_%s_%s' % (n_prim, n_r, form, kind) in names
    assert recorder.N_DRAWS == 81
    assert any(name.startswith('chi2_') for name in names)
    assert any(name.startswith('degenerate_') for name in names)
    for name, result in parent.items():
        draws, waves = recorder.FORMS[dict(CASES)[name]['form']]
        assert tuple(result['launch']) == ((81 + draws - 1) // draws, waves, 0), name
