"""The chunk plan of the synchronous host-array calls without a GPU (csrc/hostmath.h:
plan_sync_chunks through tc_debug_sync_chunks; the chunk arithmetic of csrc/predict_call.h,
PredictRequest::chunk, is checked by tools/sanitize/host_driver.cpp, which
tests/test_host_cpu.py builds and runs under the sanitizers).  The expected
boundaries are the arithmetic of the commit before the planner existed -- sync_chunks() and the
boundary loops of predict_chunked in table.cpp, the inline rule of tc_interp_predict_zheng07_batch
-- transcribed below, with the one deliberate difference on top: a boundary equal to its
predecessor is dropped, so that no chunk is empty."""

import ctypes
import itertools

import pytest

DRAWS = [1, 63, 64, 65, 100, 2047, 2048, 4096, 5013, 9037, 10**4, 4 * 10**5]
SYNC_CHUNKS = [-1, 0, 1, 2, 3, 7, 8, 64]
SYNC_STAGGER = [0, 1, 10, 50, 100]
DOUBLES = [8, 20, 257, 761]           # of results per draw


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def planned(lib, n_draws, sync_chunks, sync_stagger, doubles, interp=False, cross=False,
            likelihood=False, n_lanes=4, float32=True, pipeline=1, chain=False):
    """(staggered, boundaries) of tc_debug_sync_chunks, or None: the serial path."""
    from tabcorr_amd import _lib
    options = (ctypes.c_int * 3)(sync_chunks, sync_stagger, pipeline)
    n_chunks, staggered = ctypes.c_int(-1), ctypes.c_int(-1)
    begins = (ctypes.c_int64 * 65)()
    call = chain | likelihood << 1 | float32 << 2 | interp << 3 | cross << 4
    _lib.check(lib.tc_debug_sync_chunks(n_draws, 8 * doubles, 1 if likelihood else doubles - 1,
                                        options, n_lanes, call, ctypes.byref(n_chunks), begins,
                                        ctypes.byref(staggered)))
    if n_chunks.value == 0:
        assert staggered.value == 0
        return None
    return bool(staggered.value), list(begins[:n_chunks.value + 1])


def parent_plan(n_draws, sync_chunks, sync_stagger, doubles, interp=False, cross=False,
                likelihood=False, n_lanes=4, float32=True, pipeline=1, chain=False):
    """The parent's arithmetic: (staggered, boundaries -- repeated ones included) or None."""
    out_bytes = n_draws * doubles * 8
    second_cols = 1 if likelihood else doubles - 1
    # table.cpp: sync_chunks(); interp.cpp: the rule of tc_interp_predict_zheng07_batch (which
    # does not know option "ordered")
    if sync_chunks < 0 or not pipeline or n_lanes < 2 or (chain and not interp):
        return None
    if sync_chunks >= 1:
        n_chunks = min(sync_chunks, (n_draws + 63) // 64)
    elif n_draws < 2048:
        return None
    elif interp and cross:
        n_chunks = 1
    else:
        n_chunks = min(min(8, n_draws // 1024), max(2, out_bytes >> 20))
    # predict_chunked / interp_chunked
    chunk = ((n_draws + n_chunks - 1) // n_chunks + 63) // 64 * 64
    n_chunks = (n_draws + chunk - 1) // chunk
    begins = [min(n_draws, k * chunk) for k in range(n_chunks + 1)]
    staggered = (not interp and sync_stagger != 0 and out_bytes >= 16 << 20 and
                 second_cols * 8 >= 2048 and n_chunks >= 4 and not likelihood and n_lanes >= 2 and
                 float32)
    if staggered:
        if sync_chunks == 0:
            n_chunks = min(n_chunks, 6)
        ratio = (0.01 * sync_stagger) ** (1.0 / (n_chunks - 1))
        share = [ratio ** k for k in range(n_chunks)]
        total = 0.0
        for value in share:
            total += value
        done = 0.0
        begins = [0]
        for k in range(n_chunks):
            done += share[k]
            end = n_draws if k + 1 == n_chunks else \
                min(n_draws, (int(n_draws * done / total) + 63) // 64 * 64)
            begins.append(max(end, begins[k]))
    return staggered, begins


def without_repeats(begins):
    return [b for k, b in enumerate(begins) if k == 0 or b > begins[k - 1]]


def check_properties(n_draws, begins, what):
    assert begins[0] == 0 and begins[-1] == n_draws, what
    assert all(b % 64 == 0 for b in begins[1:-1]), what
    assert all(a < b for a, b in zip(begins, begins[1:])), what
    assert 1 <= len(begins) - 1 <= 64, what


@pytest.mark.parametrize('interp', [False, True], ids=['table', 'interpolator'])
@pytest.mark.parametrize('cross', [False, True], ids=['auto', 'cross'])
def test_the_plan_is_the_parents_without_empty_chunks(lib, interp, cross):
    n_planned = n_staggered = n_dropped = 0
    for n_draws, sync_chunks, sync_stagger, doubles in itertools.product(
            DRAWS, SYNC_CHUNKS, SYNC_STAGGER, DOUBLES):
        for likelihood, n_lanes, float32 in itertools.product((False, True), (1, 4),
                                                              (False, True)):
            args = (n_draws, sync_chunks, sync_stagger, doubles, interp, cross, likelihood,
                    n_lanes, float32)
            got, expect = planned(lib, *args), parent_plan(*args)
            assert (got is None) == (expect is None), args
            if got is None:
                continue
            assert got == (expect[0], without_repeats(expect[1])), args
            check_properties(n_draws, got[1], args)
            n_planned += 1
            n_staggered += got[0]
            n_dropped += len(expect[1]) != len(got[1])
    # the sweep reaches what it is there for: plans, staggered ones (tables only), and the
    # parent's empty chunks
    assert n_planned > 2000
    assert (n_staggered > 0) == (not interp) and (n_dropped > 0) == (not interp)


def test_the_serial_path(lib):
    for kwargs in ({'pipeline': 0}, {'n_lanes': 1}, {'chain': True}):
        assert planned(lib, 10**4, 0, 10, 20, **kwargs) is None
        assert planned(lib, 10**4, 4, 10, 20, **kwargs) is None
    assert planned(lib, 10**4, -1, 10, 20) is None
    assert planned(lib, 2047, 0, 10, 20) is None
    assert planned(lib, 2047, 0, 10, 20, interp=True, cross=True) is None


def test_anchors(lib):
    """(draws, sync_chunks, sync_stagger, doubles per draw) of a float32 table -> boundaries."""
    equal = {
        (9037, 0, 10, 20): [0, 4544, 9037],
        (9037, 3, 10, 20): [0, 3072, 6144, 9037],
        (9037, 8, 10, 20): list(range(0, 8065, 1152)) + [9037],
        (100, 64, 10, 20): [0, 64, 100],
        (4096, 3, 10, 20): [0, 1408, 2816, 4096],
        (5013, 7, 10, 8): list(range(0, 4609, 768)) + [5013],
    }
    for args, begins in equal.items():
        assert planned(lib, *args) == (False, begins), args
    staggered = {
        (10000, 0, 10, 761): [0, 3968, 6464, 8000, 9024, 9664, 10000],
        (8192, 0, 10, 257): [0, 3264, 5312, 6592, 7360, 7872, 8192],
        (8192, 6, 1, 257): [0, 4992, 6976, 7744, 8064, 8192],      # (the parent: six, one empty)
    }
    for args, begins in staggered.items():
        assert planned(lib, *args) == (True, begins), args
    assert parent_plan(8192, 6, 1, 257)[1] == [0, 4992, 6976, 7744, 8064, 8192, 8192]
    # the same table in float64, or a likelihood: equal chunks
    assert planned(lib, 8192, 0, 10, 257, float32=False) == (False, list(range(0, 8193, 1024)))
    assert planned(lib, 8192, 0, 10, 257, likelihood=True)[0] is False


def test_the_interpolator(lib):
    # mode cross, the automatic choice: one chunk from 2048 draws on
    for n_draws in (2048, 4096, 10**4, 4 * 10**5):
        assert planned(lib, n_draws, 0, 10, 761, interp=True, cross=True) == (False, [0, n_draws])
    # mode auto: as many as a table's; explicit counts too; never staggered
    for n_draws, sync_chunks, doubles in itertools.product((4096, 8192, 10**4, 4 * 10**5),
                                                           (0, 3, 6, 8), DOUBLES):
        for cross in (False, True):
            if cross and sync_chunks == 0:
                continue
            table = planned(lib, n_draws, sync_chunks, 0, doubles, cross=cross)
            for sync_stagger in SYNC_STAGGER:
                assert planned(lib, n_draws, sync_chunks, sync_stagger, doubles, interp=True,
                               cross=cross) == table, (n_draws, sync_chunks, doubles, cross)


def test_refuses_what_is_no_call(lib):
    from tabcorr_amd import _lib
    options = (ctypes.c_int * 3)(0, 10, 1)
    n_chunks, staggered = ctypes.c_int(), ctypes.c_int()
    begins = (ctypes.c_int64 * 65)()
    tail = (ctypes.byref(n_chunks), begins, ctypes.byref(staggered))
    assert lib.tc_debug_sync_chunks(-1, 160, 19, options, 4, 0, *tail) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_sync_chunks(100, 8, 19, options, 4, 0, *tail) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_sync_chunks(100, 160, 19, options, 0, 0, *tail) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_sync_chunks(100, 160, 19, None, 4, 0, *tail) == _lib.TC_ERR_INVALID
    for bad in ((65, 10, 1), (-2, 10, 1), (0, 101, 1)):
        assert lib.tc_debug_sync_chunks(100, 160, 19, (ctypes.c_int * 3)(*bad), 4, 0,
                                        *tail) == _lib.TC_ERR_INVALID
