"""The forward calls share one request (csrc/predict_call.h: PredictRequest), one chunk plan
(hostmath.h: plan_sync_chunks), one chunk loop and one ticket ring.  That changed no bit on the
paths tests/test_gpu_call_paths.py does not reach: staggered chunks -- the plan with an empty chunk
in the parent's arithmetic among them --, the direct loads and stores of asynchronous calls and of
a synchronous call's chunks, an interpolator's chunks separated by galaxy type, and a ticket ring
that has gone round.  Each returns, bit for bit, what the commit before returned on an MI355X
(tests/golden/forward_paths_parent.npz, recorded by tests/golden/make_forward_paths_parent.py with
that commit's library) and launches the same (workgroups, waves, slabs, LDS bytes); the recorded
values agree with the oracle.  Needs an MI355X."""

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
        'make_forward_paths_parent', os.path.join(GOLDEN, 'make_forward_paths_parent.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


recorder = load_recorder()
base = recorder.base
CASES = recorder.cases()


@pytest.fixture(scope='module')
def parent():
    return recorder.unpack(np.load(recorder.FILE))


@pytest.fixture(scope='module')
def oracle_values():
    """The oracle's (ngal, xi) of a case's (kept) draws, computed once per table, draws and
    separation."""
    cache = {}

    def values(case):
        from oracle import tabcorr_oracle as oracle
        key = (case['target'], case['n_draws'], case['separate'])
        if key not in cache:
            tables, _, points = recorder.tables_of(case['target'])
            theta = base.theta_of(case)
            x = base.x_of(case, points) if points is not None else None
            if base.is_digest(case):
                theta = base.edges_of(theta)
                x = base.edges_of(x) if x is not None else None
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
    got = base.stored_form(case, got)
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
    """The recorded values `want` of a case (predictions, regular draws) against the oracle:
    relative 1e-10 with a floor of 1e-14 of the largest element; float32 tables: what
    test_gpu_full_size.py states for them."""
    f32 = recorder.dtype_of(case['target']) == 'float32'

    def check_xi(got, expect, what):
        got = np.reshape(got, np.shape(expect))
        if f32:
            np.testing.assert_allclose(got, expect, rtol=RTOL_F32,
                                       atol=RTOL_F32 * np.max(np.abs(expect)), err_msg=what)
        else:
            assert_rel(got, expect, RTOL, what, floor=FLOOR)

    def check_ngal(got, expect, what):
        assert_rel(np.reshape(got, np.shape(expect)), expect, RTOL_F32 if f32 else RTOL, what)

    expect_ngal, expect_xi = oracle_values(case)
    if case['separate']:
        for key in expect_ngal:
            check_ngal(want['ngal_' + key], expect_ngal[key], 'ngal ' + key)
        for key in expect_xi:
            check_xi(want['xi_' + key], expect_xi[key], 'xi ' + key)
    else:
        check_ngal(want['ngal'], expect_ngal, 'ngal')
        check_xi(want['xi'], expect_xi, 'xi')


@pytest.mark.parametrize('name, case', CASES, ids=[name for name, _ in CASES])
def test_same_bits_as_the_parent_commit(name, case, parent, oracle_values):
    recorded, unrepeatable = parent
    assert unrepeatable == set()    # (every case repeated bit for bit on the parent)
    assert_same_bits(case, recorder.run_case(case), recorded[name], name)
    check_against_oracle(case, recorded[name], oracle_values)


@pytest.mark.parametrize('target', ['auto19', 'interp_cross'])
def test_a_ticket_ring_that_has_gone_round(target, parent):
    """kMaxTickets + 3 asynchronous predictions in flight, none waited for: every one returns
    the bits of the recorded single asynchronous call; ticket 0, whose slot was reused, and the
    last ticket can be queried and waited for and are done afterwards; a ticket that was never
    issued is still refused."""
    from tabcorr_amd import _lib
    recorded, unrepeatable = parent
    name = target + '_ring'
    calls, report = recorder.ring(target)
    assert recorder.N_RING == recorder.MAX_TICKETS + 3 == 67 and len(calls) == recorder.N_RING
    assert report['tickets'] == list(range(recorder.N_RING))
    assert report['done_after_wait'] == {0: 1, recorder.N_RING - 1: 1}
    assert report['never_issued'] == (_lib.TC_ERR_INVALID, _lib.TC_ERR_INVALID)
    for number, call in enumerate(calls):
        for key in ('ngal', 'xi'):
            assert base.same_words(call[key], recorded[name][key]), (number, key)


def test_the_recorded_cases_are_the_ones_asked_for(parent):
    recorded, unrepeatable = parent
    cases = dict(CASES)
    assert set(recorded) == set(cases) and unrepeatable == set()
    # the staggered table: float32, n_r = 256, results past 16 MB and 2048 bytes per draw
    s = recorder.STAGGER
    n_r = int(np.prod(s['tpcf_shape']))
    assert (s['dtype'], s['mode'], s['n_prim'] * s['n_sec'], n_r) == ('float32', 'auto', 6, 256)
    assert recorder.N_STAGGER * (n_r + 1) * 8 >= 16 << 20 and (n_r + 1) * 8 >= 2048
    assert cases['stagger_6_1']['options'] == (('sync_chunks', 6), ('sync_stagger', 1))
    assert cases['stagger_4_50']['options'] == (('sync_chunks', 4), ('sync_stagger', 50))
    # the chunks shrink: the last launch of the staggered calls is a small chunk's, and smaller
    # with a ratio of 1 % than with 50 %
    launches = {name: recorded[name]['launch'][0] for name in recorded}
    assert launches['stagger_6_1'] < launches['stagger_default'] < launches['stagger_4_50']
    # every combination of the direct loads and stores, on the (9, 2, 19) float64 table
    assert base.TABLES['auto19'] == ((9, 2, 19), 'auto', 'float64')
    assert {cases[name]['options'] for name in cases if name.startswith('auto19_async_in')} == {
        (('async_direct_in', i), ('async_direct_out', o)) for i in (0, 1) for o in (0, 1, 2)}
    assert {cases[name]['options'] for name in cases if name.startswith('auto19_chunks2')} == {
        (('sync_chunks', 2), ('sync_direct_out', o)) for o in (0, 1, 2)}
    for target in ('interp_auto', 'interp_cross'):
        case = cases[target + '_separate_chunks3']
        assert case['separate'] and case['n_draws'] == 4096
        assert case['options'] == (('sync_chunks', 3), )
    assert os.path.getsize(recorder.FILE) < 500 * 1000
