"""contract_quad_kernel and contract_quad_f32_kernel walk their matrix units through
csrc/fused_walk.h, as fused_quad_pass does, and the latency form's fused_quad_pass40 keeps the
same schedule written out by hand: moving the two kernels there changed neither the order of a
sum nor a launch shape, and the next change to the walk must not either, so every case returns,
bit for bit, what the commit before the move returned on an MI355X
(tests/golden/quad_walk_parent.npz, recorded by
tests/golden/make_quad_walk_parent.py with that commit's library), and those recorded values
agree with the oracle: float64 at the tolerance of test_gpu_fused.py, float32 at the one
test_gpu_full_size.py applies to its float32 cases.  Needs an MI355X."""

import importlib.util
import os

import numpy as np
import pytest

from util import GOLDEN, assert_rel

pytestmark = pytest.mark.gpu

RTOL = 1e-10          # (test_gpu_fused.py)
RTOL_F32 = 1e-5       # (test_gpu_full_size.py: the float32 path's stated tolerance)


def load_recorder():
    spec = importlib.util.spec_from_file_location(
        'make_quad_walk_parent', os.path.join(GOLDEN, 'make_quad_walk_parent.py'))
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
    """The oracle's (ngal, xi) per table, draws and separation, computed once."""
    cache = {}

    def values(case):
        from oracle import tabcorr_oracle as oracle
        key = (case['kind'] == 'interp', case['n_prim'], case['n_r'], case['separate'],
               case['degenerate'])
        if key not in cache:
            with np.errstate(all='ignore'):
                if case['kind'] == 'interp':
                    tables, _, points = recorder.interpolator_of(case)
                    cache[key] = oracle.interpolator_predict_zheng07_batch(
                        tables, oracle.interpolator_setup(tables, points),
                        recorder.theta_of(case), recorder.x_of(case, points))
                else:
                    cache[key] = oracle.predict_zheng07_batch(
                        recorder.table_of(case), recorder.theta_of(case),
                        separate_gal_type=case['separate'])
        return cache[key]
    return values


@pytest.mark.parametrize('name, case', CASES, ids=[name for name, _ in CASES])
def test_same_bits_as_the_parent_commit(name, case, parent, oracle_values):
    want = parent[name]
    got = recorder.run_case(case)           # (asserts that the form asked for ran)
    assert sorted(got) == sorted(want)
    assert tuple(got['launch']) == tuple(want['launch'])
    for key in want:
        if key != 'launch':
            assert got[key].shape == want[key].shape
            differing = int(np.sum(got[key].view(np.uint64) != want[key].view(np.uint64)))
            assert differing == 0, '%s: %d of %d values differ from the parent\'s' % (
                key, differing, want[key].size)
    # the recorded values themselves against the oracle
    expect_ngal, expect_xi = oracle_values(case)
    rows = np.ones(recorder.N_DRAWS, dtype=bool)
    if case['degenerate']:      # (the regular draws beside the degenerate ones)
        rows[list(recorder.DEGENERATE_ROWS)] = False
    f32 = case['dtype'] == 'float32'

    def check_xi(got, expect, what, floor):
        if f32:     # (test_gpu_full_size.py: relative, with the array's scale as the floor)
            np.testing.assert_allclose(got[rows], expect[rows], rtol=RTOL_F32,
                                       atol=RTOL_F32 * np.max(np.abs(expect[rows])), err_msg=what)
        else:
            assert_rel(got[rows], expect[rows], RTOL, what, floor=floor)
    # (the occupations stay float64 on float32 tables; the interpolator's ngal: 1e-11 there)
    rtol_ngal = RTOL if not f32 else 1e-11 if case['kind'] == 'interp' else 1e-12
    if case['kind'] == 'latency_chi2':
        vector, precision = recorder.likelihood_of(case)
        delta = expect_xi - vector
        assert_rel(want['ngal'], expect_ngal, RTOL, 'ngal')
        assert_rel(want['chi2'], np.einsum('bi,ij,bj->b', delta, precision, delta), 1e-9, 'chi2')
    elif case['separate']:
        for key in expect_ngal:
            assert_rel(want['ngal_' + key], expect_ngal[key], rtol_ngal, 'ngal ' + key)
        for key in expect_xi:
            check_xi(want['xi_' + key], expect_xi[key], 'xi ' + key, 1e-13)
    else:
        assert_rel(want['ngal'][rows], expect_ngal[rows], rtol_ngal, 'ngal')
        # (test_gpu_full_size.py: the float64 interpolator's floor)
        check_xi(want['xi'], expect_xi, 'xi', 1e-12 if case['kind'] == 'interp' else 1e-14)


def test_the_recorded_cases_are_the_ones_asked_for(parent):
    """81 draws.  Three kernels, float64: U = 1 ... 5, 2 ... 25 block rows, two r tiles, total, and
    separated for every U; float32: U = 1 ... 4 and two r tiles with n_prim 10 and 50, separated
    for every U; the interpolator's per-table weight in float64 and float32; the latency form's
    five load patterns with n_prim 4, 10, 50, its likelihood, degenerate draws."""
    names = set(parent)
    assert names == {name for name, _ in CASES}
    assert recorder.N_DRAWS == 81
    for n_prim, n_r in [(4, 19), (5, 19), (10, 19), (50, 3), (50, 8), (50, 12), (50, 16), (50, 19),
                        (10, 40)]:
        assert 'three_f64_p%d_r%d_tot' % (n_prim, n_r) in names
    for n_r in (3, 8, 12, 16, 19):          # U = 1 ... 5
        assert any(name.startswith('three_f64_') and name.endswith('_r%d_sep' % n_r)
                   for name in names)
    for n_r in (3, 7, 12, 16, 19):
        for n_prim in (10, 50):
            assert 'three_f32_p%d_r%d_tot' % (n_prim, n_r) in names
    for n_r in (3, 7, 12, 16):              # U = 1 ... 4
        assert any(name.startswith('three_f32_') and name.endswith('_r%d_sep' % n_r)
                   for name in names)
    assert {'interp_f64_p10_r19', 'interp_f32_p10_r12'} <= names
    for n_prim in (4, 10, 50):
        for n_r in (3, 8, 12, 16, 19):
            assert 'latency_p%d_r%d' % (n_prim, n_r) in names
    assert {'latency_chi2_p50_r19', 'latency_degenerate_p10_r19'} <= names
    for name, result in parent.items():
        workgroups, waves, slabs = (int(v) for v in result['launch'])
        if name.startswith('latency_'):
            assert (workgroups, waves, slabs) == (3, 8, 0), name
        else:
            assert waves == 4 and slabs > 0, name
