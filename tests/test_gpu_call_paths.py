"""What a call needs on its way from an entry point to a launch -- its lane, whether it is pinned
to lane 0 or asynchronous, where the likelihood may go, the hints of a chunked synchronous call --
travels as an argument (csrc/internal.h: Call), not as fields of the handle.  That changed no bit:
every entry point of the prediction path returns, bit for bit (NaN words included), what the
commit before returned on an MI355X (tests/golden/call_paths_parent.npz, recorded by
tests/golden/make_call_paths_parent.py with that commit's library) and launches the same
(workgroups, waves, slabs, LDS bytes); the recorded values agree with the oracle; and a handle
that has served one kind of call after another returns what a fresh handle returns, so nothing
a call set outlives it.  Needs an MI355X."""

import copy
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from util import GOLDEN, assert_rel

pytestmark = pytest.mark.gpu

RTOL = 1e-10          # the suite's parity bar, with a floor of
FLOOR = 1e-14         # ... this times the largest element
RTOL_F32 = 1e-5       # (test_gpu_full_size.py: the float32 path's stated tolerance)


def load_recorder():
    spec = importlib.util.spec_from_file_location(
        'make_call_paths_parent', os.path.join(GOLDEN, 'make_call_paths_parent.py'))
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
    """The oracle's (ngal, xi) of a case's (kept) draws, per call, computed once per table,
    draws and separation."""
    cache = {}

    def values(case, call=0):
        from oracle import tabcorr_oracle as oracle
        key = (case['target'], case['n_draws'], case['degenerate'], case['separate'], call)
        if key not in cache:
            tables, _, points = recorder.tables_of(case['target'])
            theta = recorder.theta_of(case, call)
            x = recorder.x_of(case, points, call) if points is not None else None
            if recorder.is_digest(case):
                theta = recorder.edges_of(theta)
                x = recorder.edges_of(x) if x is not None else None
            with np.errstate(all='ignore'):
                if points is not None:
                    cache[key] = oracle.interpolator_predict_zheng07_batch(
                        tables, oracle.interpolator_setup(tables, points), theta, x,
                        separate_gal_type=case['separate'], extrapolate=True)
                else:
                    cache[key] = oracle.predict_zheng07_batch(tables[0], theta,
                                                              separate_gal_type=case['separate'])
        return cache[key]
    return values


def assert_same_bits(case, got, want, what):
    """A run's result against a recorded one."""
    got = recorder.stored_form(case, got)
    assert sorted(got) == sorted(want), what
    assert tuple(got['launch']) == tuple(want['launch']), what
    for key in want:
        if key == 'launch':
            continue
        assert got[key].shape == want[key].shape, (what, key)
        if key.endswith('#'):
            assert got[key].tobytes() == want[key].tobytes(), \
                '%s: %s differs from the parent\'s digest' % (what, key)
            continue
        differing = int(np.sum(got[key].view(np.uint64) != want[key].view(np.uint64)))
        assert differing == 0, '%s: %d of %d words of %s differ from the parent\'s' % (
            what, differing, want[key].size, key)


def check_against_oracle(case, want, oracle_values):
    """The recorded values `want` of a case against the oracle: relative 1e-10 with a floor of
    1e-14 of the largest element (float32 tables: what test_gpu_full_size.py states for them).
    The likelihood chi2 = d^T P d of d = xi - data inherits the bound of xi to first order:
    |chi2 - expected| <= 2 sum_j |(P d)_j + (P^T d)_j| / 2 * tol_j with tol_j the bound of xi_j
    above (the cancellation in d is why a plain relative bound does not carry over)."""
    f32 = recorder.dtype_of(case['target']) == 'float32'
    n_kept = 2 * recorder.N_EDGE if recorder.is_digest(case) else case['n_draws']
    rows = np.ones(n_kept, dtype=bool)
    if case['degenerate']:      # (the regular draws beside the degenerate ones)
        rows[[r for r in recorder.DEGENERATE_ROWS if r < n_kept]] = False

    def check_xi(got, expect, what):
        got = np.reshape(got, np.shape(expect))
        if f32:
            np.testing.assert_allclose(got[rows], expect[rows], rtol=RTOL_F32,
                                       atol=RTOL_F32 * np.max(np.abs(expect[rows])), err_msg=what)
        else:
            assert_rel(got[rows], expect[rows], RTOL, what, floor=FLOOR)
        if case['degenerate']:
            # the degenerate draws themselves: NaN for NaN, infinite for infinite, the finite
            # values as everywhere
            assert np.array_equal(np.isnan(got), np.isnan(expect)), what
            assert np.array_equal(np.isinf(got), np.isinf(expect)), what
            finite = np.isfinite(expect)
            if not f32:
                assert_rel(got[finite], expect[finite], RTOL, what, floor=FLOOR)

    def check_ngal(got, expect, what):
        got = np.reshape(got, np.shape(expect))
        assert_rel(got[rows], expect[rows], RTOL_F32 if f32 else RTOL, what)
        if case['degenerate']:
            assert np.array_equal(np.isnan(got), np.isnan(expect)), what

    n_calls = sum(key.startswith('ngal_call') for key in want) or 1
    for call in range(n_calls):
        tag = '_call%d' % call if 'ngal_call0' in want else ''
        expect_ngal, expect_xi = oracle_values(case, call)
        if case['separate']:
            for key in expect_ngal:
                check_ngal(want['ngal_' + key + tag], expect_ngal[key], 'ngal ' + key)
            for key in expect_xi:
                check_xi(want['xi_' + key + tag], expect_xi[key], 'xi ' + key)
        elif case['chi2']:
            check_ngal(want['ngal' + tag], expect_ngal, 'ngal')
            vector, precision = recorder.likelihood_of(expect_xi.shape[-1])
            delta = (expect_xi - vector)[rows]
            tol = (RTOL_F32 if f32 else RTOL) * np.abs(expect_xi[rows]) + \
                (RTOL_F32 if f32 else FLOOR) * np.max(np.abs(expect_xi[rows]))
            slope = np.abs(delta @ precision.T + delta @ precision)
            bound = np.sum(slope * tol, axis=-1)
            expect = np.einsum('bi,ij,bj->b', delta, precision, delta)
            got = np.reshape(want['chi2' + tag], -1)[rows]
            worst = np.max(np.abs(got - expect) / bound)
            assert worst <= 1.0, 'chi2: %.3g of the bound inherited from xi' % worst
        else:
            check_ngal(want['ngal' + tag], expect_ngal, 'ngal')
            check_xi(want['xi' + tag], expect_xi, 'xi')


@pytest.mark.parametrize('name, case', CASES, ids=[name for name, _ in CASES])
def test_same_bits_as_the_parent_commit(name, case, parent, oracle_values):
    recorded, unrepeatable = parent
    want = recorded[name]
    got = recorder.run_case(case)
    if name in unrepeatable:    # (the parent's own two runs differed: the oracle alone judges)
        check_against_oracle(case, recorder.stored_form(case, got), oracle_values)
    else:
        assert_same_bits(case, got, want, name)
    check_against_oracle(case, want, oracle_values)


def test_the_recorded_cases_are_the_ones_asked_for(parent):
    recorded, unrepeatable = parent
    cases = dict(CASES)
    assert set(recorded) == set(cases)
    assert len(unrepeatable) <= 2 and unrepeatable <= set(cases)
    assert recorder.N_DRAWS == 81 and recorder.N_LARGE == 4096
    assert recorder.TABLES['auto19'][0] == recorder.TABLES['cross19'][0] == (9, 2, 19)
    assert recorder.TABLES['auto34'][0] == (12, 2, 34)
    assert recorder.TABLES['auto40'][0] == (30, 2, 40)
    assert recorder.TABLES['f32'][2] == 'float32'
    assert cases['auto19_slabs_chi2']['n_draws'] == (1 << 18) + 17
    # every entry point sees degenerate draws, and they left their mark: NaN results, not only NaN
    for name, case in CASES:
        if case['degenerate'] and not case['chi2']:
            bad = np.isnan(recorded[name]['xi']).any(axis=-1)
            assert bad.any() and not bad.all(), name
    # the likelihood: fused into the one launch or the finalisation up to 32 rows (the launch
    # is the prediction's), a kernel of its own behind 34 rows and behind more than one slab
    for target in recorder.TABLES:
        assert 'chi2' in recorded[target + '_host_chi2']
    # the chunks of a large call took the copy and chunk paths: one launch per chunk, smaller
    # than the whole call's
    for target in ('auto19', 'cross19'):
        whole = recorded[target + '_large_predict_chunks-1']['launch'][0]
        for chunks in (2, 3):
            assert recorded['%s_large_predict_chunks%d' % (target, chunks)]['launch'][0] < whole
    # n_lanes + 1 pipelined calls, each recorded
    for name in ('auto19_ordered_on', 'cross19_ordered_off', 'interp_cross_ordered_on'):
        assert sum(key.startswith('xi_call') for key in recorded[name]) == 5


@pytest.mark.parametrize('mode', ['auto', 'cross'])
def test_nothing_a_call_set_outlives_it(mode, parent):
    """One table handle, and an interpolator that shares it, through every kind of call in turn:
    each returns what the same call returned on a fresh handle."""
    from tabcorr_amd import _lib
    recorded, unrepeatable = parent
    cases = dict(CASES)
    whole = recorder.Target('interp_' + mode)
    table = copy.copy(whole)                # the interpolator's first table, called directly
    table.interpolator, table.halotabs, table.points = None, whole.halotabs[:1], None
    name_of = {table: mode + '19', whole: 'interp_' + mode}
    lib = whole.lib

    def step(handles, suffix, options=()):
        name = name_of[handles] + suffix
        handles.set_options(options)
        got = handles.call(cases[name])
        got['launch'] = handles.last_launch()
        handles.set_options([(key, 0) for key, _ in options])
        if name not in unrepeatable:
            assert_same_bits(cases[name], got, recorded[name], name)

    step(table, '_host_chi2')
    step(table, '_host_predict')
    # rejected calls (argument errors): a likelihood separated by galaxy type, an asynchronous
    # call with pageable buffers
    handle = table.halotab.to_device().handle
    theta = recorder.theta_of(cases[mode + '19_host_chi2'])
    vector, precision = (np.ascontiguousarray(a) for a in recorder.likelihood_of(table.n_r))
    ngal, chi2 = np.empty(len(theta)), np.empty(len(theta))
    xi = np.empty((len(theta), table.n_r))
    p = _lib.as_double_p
    assert lib.tc_chi2_zheng07_batch(handle, p(theta), 5, len(theta), 10,
                                     _lib.FLAG_SEPARATE_GAL_TYPE, p(vector), p(precision), p(ngal),
                                     p(chi2)) == _lib.TC_ERR_INVALID
    ticket = ctypes.c_int64(-1)
    assert lib.tc_predict_zheng07_batch_async(handle, p(theta), 5, len(theta), 10, 0, p(ngal),
                                              p(xi), ctypes.byref(ticket)) == _lib.TC_ERR_INVALID
    step(table, '_async_chi2')
    step(table, '_ordered_off')             # n_lanes + 1 pipelined _device predictions
    step(table, '_large_predict_chunks2', options=(('sync_chunks', 2), ))
    step(whole, '_host_chi2')
    step(table, '_host_predict')
