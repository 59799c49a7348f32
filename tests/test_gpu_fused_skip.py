"""predict_fused_kernel, eight waves x 64 draws (csrc/fused_skip.h): option "fused_skip" 1 places a
workgroup's draws in the order of M0 and issues no matrix instruction for a block of densities
that is exactly zero for a group of 16 draws, with the parts (0, 1) and (2, 3) sharing a SIMD; 3
the same with the parts paired as ever; 2 leaves the draws where they are as well; 0 issues every
product.  All four must agree bit for bit -- for predict() and for the fused
likelihood, with every draw's satellites gone, with exactly one group's worth of such draws and
one less, with M0 stepping through the bins, with degenerate M0 and overflowing satellites beside
regular draws, on tables with infinite, NaN and negative entries -- and with the oracle.
Needs an MI355X."""

import ctypes

import numpy as np
import pytest

import exact_tables
from util import assert_rel

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SHAPES = [(4, 19), (5, 19), (10, 19), (18, 19), (50, 3)]      # (n_prim, r bins)
N_DRAWS = (64, 81, 129)          # whole workgroups; a partly filled tile; an empty tile
TOP = 15.0                       # synthetic tables: bins from 10.5 to 15.0


def thetas(n_draws, n_prim):
    """name -> (theta, rows to compare with the oracle)."""
    from tabcorr_amd import synthetic
    regular = synthetic.zheng07_draws(n_draws, seed=n_draws + n_prim)
    everyone = np.ones(n_draws, dtype=bool)
    out = {}
    above = regular.copy()
    above[:, 2] = TOP + 0.5 + 0.01 * np.arange(n_draws)
    out['above'] = (above, everyone)
    for count in (16, 15):
        some = regular.copy()
        rows = (np.arange(count) * 5 + 2) % 64          # spread over both tiles of workgroup 0
        assert len(set(rows)) == count
        some[rows, 2] = TOP + 1.0
        out['group%d' % count] = (some, everyone)
    stepping = regular.copy()
    stepping[:, 2] = np.linspace(10.4, TOP + 0.2, n_draws)
    stepping[::7, 2] = np.round(stepping[::7, 2] * 10) / 10     # some exactly on bin edges
    out['stepping'] = (stepping, everyone)
    special = stepping[::-1].copy()
    special[1, 2] = np.nan
    special[5, 2] = np.inf
    special[17, 2] = -np.inf
    special[33, 2] = -300.0
    special[min(70, n_draws - 1), 2] = np.nan
    out['special'] = (special, everyone)
    overflow = above.copy()
    overflow[::3] = regular[::3]
    overflow[6, 3] = -400.0          # M1 underflows, alpha > 0: infinite satellites (kInfSat)
    overflow[6, 2] = 11.0
    rows = everyone.copy()
    rows[6] = False                  # (test_gpu_fused.py holds degenerate draws to the other path)
    out['overflow'] = (overflow, rows)
    return out


_handles = {}


def handle_of(name, table):
    from tabcorr_amd import TabCorr, _lib
    if name not in _handles:
        halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                      table['tpcf_shape'], table['attrs'])
        handle = halotab.to_device().handle
        lib = _lib.load()
        for key, value in (('fused', 2), ('fused_min_draws', 1), ('single_draw', 0),
                           ('fused_draws', 64), ('fused_waves', 8)):
            _lib.check(lib.tc_table_set_option(handle, key.encode(), value))
        _handles[name] = halotab
    return _handles[name]


def likelihood_of(n_r):
    rng = np.random.default_rng(n_r)
    vector = np.geomspace(30.0, 0.05, n_r)
    a = rng.normal(size=(n_r, n_r))
    return vector, a @ a.T / np.mean(vector)**2


def run(halotab, theta, skip, n_r):
    """predict and the fused likelihood with option fused_skip = skip."""
    from tabcorr_amd import _lib
    lib = _lib.load()
    handle = halotab.to_device().handle
    _lib.check(lib.tc_table_set_option(handle, b'fused_skip', skip))
    vector, precision = likelihood_of(n_r)
    with np.errstate(all='ignore'):
        ngal, xi = halotab.predict_batch(theta)
        launch = [ctypes.c_int() for _ in range(4)]
        _lib.check(lib.tc_table_last_launch(handle, *[ctypes.byref(v) for v in launch]))
        assert (launch[0].value, launch[1].value) == ((len(theta) + 63) // 64, 8), \
            'not the form asked for'
        ngal_l, chi2 = halotab.chi2_batch(theta, vector, precision)
    return {key: np.ascontiguousarray(value, dtype=np.float64)
            for key, value in (('ngal', ngal), ('xi', xi), ('ngal_l', ngal_l), ('chi2', chi2))}


def assert_same_bits(a, b, what):
    for key in a:
        differing = int(np.sum(a[key].view(np.uint64) != b[key].view(np.uint64)))
        assert differing == 0, '%s, %s: %d of %d values differ' % (what, key, differing,
                                                                    a[key].size)


def check_against_oracle(got, table, theta, rows, n_r, what):
    from oracle import tabcorr_oracle as oracle
    with np.errstate(all='ignore'):
        expect_ngal, expect_xi = oracle.predict_zheng07_batch(table, theta)
    vector, precision = likelihood_of(n_r)
    for result in got:
        finite = np.isfinite(expect_xi)
        assert_rel(result['ngal'][rows], expect_ngal[rows], RTOL, what + ' ngal')
        assert_rel(result['ngal_l'][rows], expect_ngal[rows], RTOL, what + ' ngal (likelihood)')
        assert not np.any(np.isfinite(result['xi'][rows][~finite[rows]])), what
        assert_rel(np.where(finite, result['xi'], 0.0)[rows], np.where(finite, expect_xi, 0.0)[rows],
                   RTOL, what + ' xi')
        whole = rows & np.all(finite, axis=1)
        delta = expect_xi[whole] - vector
        # (the quadratic form cancels: relative to the sum of its terms' sizes)
        size = np.einsum('bi,ij,bj->b', np.abs(delta), np.abs(precision), np.abs(delta))
        expect_chi2 = np.einsum('bi,ij,bj->b', delta, precision, delta)
        assert np.all(np.abs(result['chi2'][whole] - expect_chi2) <= 1e-9 * size), what + ' chi2'


@pytest.mark.parametrize('n_draws', N_DRAWS)
@pytest.mark.parametrize('n_prim, n_r', SHAPES)
def test_skipping_keeps_the_bits(n_prim, n_r, n_draws):
    from tabcorr_amd import synthetic
    table = synthetic.synthetic_table(n_prim, 1, (n_r, ), 'auto', seed=n_prim + n_r)
    halotab = handle_of('synthetic %d %d' % (n_prim, n_r), table)
    for name, (theta, rows) in thetas(n_draws, n_prim).items():
        what = 'n_prim %d, %d draws, %s' % (n_prim, n_draws, name)
        plain = run(halotab, theta, 0, n_r)
        ordered = run(halotab, theta, 1, n_r)
        in_place = run(halotab, theta, 2, n_r)
        unpaired = run(halotab, theta, 3, n_r)
        assert_same_bits(ordered, plain, what + ', fused_skip 1 against 0')
        assert_same_bits(in_place, plain, what + ', fused_skip 2 against 0')
        assert_same_bits(unpaired, plain, what + ', fused_skip 3 against 0')
        check_against_oracle((plain, ordered), table, theta, rows, n_r, what)


def special_tables():
    """The benchmark's 100 bins with 3 r bins: an infinite entry, a NaN entry (the kernel's guard
    must switch skipping off: 0 x inf is not 0), and integer entries of either sign."""
    from tabcorr_amd import synthetic
    base = synthetic.synthetic_table(50, 1, (3, ), 'auto', seed=53)
    out = {}
    for name, value in (('inf entry', np.inf), ('nan entry', np.nan)):
        table = dict(base)
        table['tpcf_matrix'] = base['tpcf_matrix'].copy()
        # (one entry of the middle r bin: the pair of satellite bins 0 and 1 in a row-major upper
        # triangle; wherever it lies, the table is no longer finite)
        table['tpcf_matrix'][1, 50 * 100 - 50 * 49 // 2 + 1] = value
        out[name] = table
    out['negative entries'] = exact_tables.exact_table(50, 1, (3, ), 'auto', seed=5)
    return out


@pytest.mark.parametrize('name', ['inf entry', 'nan entry', 'negative entries'])
def test_skipping_keeps_the_bits_on_special_tables(name):
    table = special_tables()[name]
    halotab = handle_of(name, table)
    for n_draws in (81, 129):
        cases = thetas(n_draws, 50)
        for case in ('above', 'stepping', 'group16', 'overflow'):
            theta, rows = cases[case]
            what = '%s, %d draws, %s' % (name, n_draws, case)
            plain = run(halotab, theta, 0, 3)
            ordered = run(halotab, theta, 1, 3)
            in_place = run(halotab, theta, 2, 3)
            assert_same_bits(ordered, plain, what + ', fused_skip 1 against 0')
            assert_same_bits(in_place, plain, what + ', fused_skip 2 against 0')
            check_against_oracle((plain, ordered), table, theta, rows, 3, what)
