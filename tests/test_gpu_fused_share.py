"""predict_fused_kernel, eight waves x 64 draws, the skipping instances whose last r pass is a
single sub-tile (U = 3, 5; csrc/fused_skip.h): option "fused_share" 1 hands the last passes of a
workgroup's eight (tile, part) jobs to whichever wave comes for one, 2 hands them out a group of
16 draws at a time, 0 leaves every wave its own.  Which wave forms a sum, and when, must not show:
all three give the same words, for predict() and for the fused likelihood, run after run -- with
no mask differing, with M0 spread over the bins, with NaN M0, with the skipping guard failed (a
pair-weight sum beyond 1e280; an infinite matrix entry), where group selection must still hold.
On a table with U = 4 the option changes nothing, the launch's shape included.
81 draws: one full workgroup and one with 17 real draws.  Needs an MI355X."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_DRAWS = 81
TOP = 15.0                       # synthetic tables: bins from 10.5 to 15.0
# name -> (n_prim, r bins, U, an infinite entry)
TABLES = {
    '10 x 19': (10, 19, 5, False),
    '18 x 12': (18, 12, 3, False),
    '50 x 19': (50, 19, 5, False),
    '10 x 19, inf entry': (10, 19, 5, True),
    '10 x 16 (U = 4)': (10, 16, 4, False),
}


def thetas(n_prim):
    from tabcorr_amd import synthetic
    regular = synthetic.zheng07_draws(N_DRAWS, seed=N_DRAWS + n_prim)
    out = {}
    equal = regular.copy()
    equal[:, 2] = 12.3
    out['equal M0'] = equal
    spread = regular.copy()
    spread[:, 2] = np.linspace(10.4, TOP + 0.2, N_DRAWS)
    spread[::7, 2] = np.round(spread[::7, 2] * 10) / 10        # some exactly on bin edges
    out['spread'] = spread[np.random.default_rng(n_prim).permutation(N_DRAWS)]
    nan = out['spread'].copy()
    nan[[1, 20, 41, 70], 2] = np.nan
    out['nan M0'] = nan
    overflow = out['spread'].copy()
    overflow[6, 3] = -400.0      # M1 underflows, alpha > 0: an infinite pair-weight sum in
    overflow[6, 2] = 11.0        # workgroup 0, whose guard fails; workgroup 1 still skips
    out['guard failed'] = overflow
    return out


_tables = {}


def table_of(name):
    from tabcorr_amd import TabCorr, _lib, synthetic
    if name not in _tables:
        n_prim, n_r, _, infinite = TABLES[name]
        table = synthetic.synthetic_table(n_prim, 1, (n_r, ), 'auto', seed=n_prim + n_r)
        if infinite:
            table = dict(table)
            table['tpcf_matrix'] = table['tpcf_matrix'].copy()
            # (a pair of satellite bins in a row-major upper triangle; wherever it lies, the table
            # is no longer finite and nothing may be skipped)
            n = 2 * n_prim
            table['tpcf_matrix'][n_r // 2, n_prim * n - n_prim * (n_prim - 1) // 2 + 1] = np.inf
        halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                      table['tpcf_shape'], table['attrs'])
        handle = halotab.to_device().handle
        lib = _lib.load()
        for key, value in (('fused', 2), ('fused_min_draws', 1), ('single_draw', 0),
                           ('fused_draws', 64), ('fused_waves', 8)):
            _lib.check(lib.tc_table_set_option(handle, key.encode(), value))
        _tables[name] = halotab
    return _tables[name]


def likelihood_of(n_r):
    rng = np.random.default_rng(n_r)
    vector = np.geomspace(30.0, 0.05, n_r)
    a = rng.normal(size=(n_r, n_r))
    return vector, a @ a.T / np.mean(vector)**2


def run(halotab, theta, n_r, share, skip=1):
    """predict and the fused likelihood with option fused_share = share; the launch's shape."""
    from tabcorr_amd import _lib
    lib = _lib.load()
    handle = halotab.to_device().handle
    _lib.check(lib.tc_table_set_option(handle, b'fused_skip', skip))
    _lib.check(lib.tc_table_set_option(handle, b'fused_share', share))
    vector, precision = likelihood_of(n_r)
    with np.errstate(all='ignore'):
        ngal, xi = halotab.predict_batch(theta)
        launch = [ctypes.c_int() for _ in range(4)]
        _lib.check(lib.tc_table_last_launch(handle, *[ctypes.byref(v) for v in launch]))
        shape = tuple(v.value for v in launch)
        assert shape[:2] == ((len(theta) + 63) // 64, 8), 'not the form asked for'
        ngal_l, chi2 = halotab.chi2_batch(theta, vector, precision)
    out = {key: np.ascontiguousarray(value, dtype=np.float64)
           for key, value in (('ngal', ngal), ('xi', xi), ('ngal_l', ngal_l), ('chi2', chi2))}
    return out, shape


def assert_same_bits(a, b, what):
    for key in a:
        differing = int(np.sum(a[key].view(np.uint64) != b[key].view(np.uint64)))
        assert differing == 0, '%s, %s: %d of %d values differ' % (what, key, differing,
                                                                    a[key].size)


@pytest.mark.parametrize('name', list(TABLES))
def test_sharing_keeps_the_bits(name):
    n_prim, n_r, _, infinite = TABLES[name]
    halotab = table_of(name)
    for case, theta in thetas(n_prim).items():
        what = '%s, %s' % (name, case)
        results = {}
        for share in (0, 1, 2):
            first, shape = run(halotab, theta, n_r, share)
            again, shape_again = run(halotab, theta, n_r, share)
            assert_same_bits(again, first, what + ', fused_share %d twice' % share)
            assert shape_again == shape
            results[share] = (first, shape)
        for share in (1, 2):
            assert_same_bits(results[share][0], results[0][0],
                             what + ', fused_share %d against 0' % share)
            # (the launch is the same one: same workgroups, waves and LDS)
            assert results[share][1] == results[0][1], what
        # ... and the same as with every product issued by the wave that owns its part
        plain, _ = run(halotab, theta, n_r, 2, skip=0)
        assert_same_bits(results[2][0], plain, what + ', against fused_skip 0')
        if case == 'spread' and not infinite:
            assert np.all(np.isfinite(results[0][0]['xi'])), 'regular draws'


def test_option_is_checked():
    from tabcorr_amd import _lib
    lib = _lib.load()
    handle = table_of('10 x 19').to_device().handle
    for value in (-1, 3):
        assert lib.tc_table_set_option(handle, b'fused_share', value) != 0
    for value in (2, 1, 0):
        assert lib.tc_table_set_option(handle, b'fused_share', value) == 0
