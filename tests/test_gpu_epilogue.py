"""The steps behind a batch kernel's sums that have one copy -- spline weights (csrc/spline.h:
the interpolator kernels, the mode-cross one-launch kernels, the host), the transposed write-out
of a results tile and the body of the two finalisation kernels (csrc/epilogue.h) -- and the ones
the one-launch kernels keep written out (the likelihood of a tile, the exchange of a tile's
shares between workgroups, the per-draw tail of the two mode-cross kernels).  Sharing changed no
bit, and the next change to any of these steps must not either unless it says so: every case
returns, bit for bit (NaN words included), what the commit before returned on an MI355X
(tests/golden/epilogue_parent.npz, recorded by tests/golden/make_epilogue_parent.py with that
commit's library), and those recorded values agree with the oracle at the tolerances of
test_gpu_cross_fused.py (float32 tables: the one test_gpu_full_size.py states for them).  Needs
an MI355X."""

import importlib.util
import os

import numpy as np
import pytest

from util import GOLDEN, assert_rel

pytestmark = pytest.mark.gpu

RTOL = 1e-10          # (test_gpu_cross_fused.py)
RTOL_CHI2 = 1e-9
RTOL_F32 = 1e-5       # (test_gpu_full_size.py: the float32 path's stated tolerance)


def load_recorder():
    spec = importlib.util.spec_from_file_location(
        'make_epilogue_parent', os.path.join(GOLDEN, 'make_epilogue_parent.py'))
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
    """The oracle's (ngal, xi) per table, draws, decoration and separation, computed once."""
    cache = {}

    def values(case, separate):
        from oracle import tabcorr_oracle as oracle
        key = (case['shape'], case['mode'], case['grid'], case['vary_n_h'], separate,
               case['degenerate'], case['assembias'], case['modulate'], case['form'] == 'small')
        if key not in cache:
            theta = recorder.theta_of(case)
            with np.errstate(all='ignore'):
                if case['grid'] is not None:
                    tables, _, points = recorder.interpolator_of(case)
                    cache[key] = oracle.interpolator_predict_zheng07_batch(
                        tables, oracle.interpolator_setup(tables, points), theta,
                        recorder.x_of(case, points), separate_gal_type=separate, extrapolate=True)
                else:
                    cache[key] = oracle.predict_zheng07_batch(
                        recorder.table_of(case), theta, separate_gal_type=separate,
                        modulate_with_cenocc=case['modulate'],
                        assembias=recorder.strengths_of(case) if case['assembias'] else None)
        return cache[key]
    return values


def check_against_oracle(case, want, oracle_values):
    """The recorded values `want` of a case against the oracle."""
    interp = case['grid'] is not None
    f32 = case['dtype'] == 'float32'
    rows = np.ones(len(recorder.theta_of(case)), dtype=bool)
    if case['degenerate']:      # (the regular draws beside the degenerate ones)
        rows[list(recorder.DEGENERATE_ROWS)] = False

    def check_xi(got, expect, what, floor):
        if f32:     # (test_gpu_full_size.py: relative, with the array's scale as the floor)
            np.testing.assert_allclose(got[rows], expect[rows], rtol=RTOL_F32,
                                       atol=RTOL_F32 * np.max(np.abs(expect[rows])), err_msg=what)
        else:
            assert_rel(got[rows], expect[rows], RTOL, what, floor=floor)

    def check(tag, separate):
        expect_ngal, expect_xi = oracle_values(case, separate)
        if separate:        # (test_gpu_cross_fused.py: compare)
            for key in expect_ngal:
                assert_rel(want['ngal_' + key + tag][rows], expect_ngal[key][rows], RTOL,
                           'ngal ' + key)
            for key in expect_xi:
                check_xi(want['xi_' + key + tag], expect_xi[key], 'xi ' + key,
                         1e-12 if interp else 1e-13)
        else:
            assert_rel(want['ngal' + tag][rows], expect_ngal[rows], RTOL, 'ngal')
            check_xi(want['xi' + tag], expect_xi, 'xi', 1e-12 if interp else 1e-14)
    if case['form'] == 'small':
        expect_ngal, expect_xi = oracle_values(case, False)
        for i in range(3):      # the un-batched calls
            assert_rel(want['ngal_one%d' % i], expect_ngal[i:i + 1], RTOL, 'ngal of call %d' % i)
            assert_rel(want['xi_one%d' % i], expect_xi[i], RTOL, 'xi of call %d' % i, floor=1e-12)
        check('', False)
        check('', True)
    elif case['chi2']:
        expect_ngal, expect_xi = oracle_values(case, False)
        vector, precision = recorder.likelihood_of(case)
        delta = expect_xi - vector
        assert_rel(want['ngal'], expect_ngal, RTOL, 'ngal')
        assert_rel(want['chi2'], np.einsum('bi,ij,bj->b', delta, precision, delta), RTOL_CHI2,
                   'chi2')
    else:
        check('', case['separate'])
    if case['degenerate']:
        # the degenerate draws themselves: NaN for NaN, infinite for infinite (the rule for
        # components whose norm is not finite), the finite values as everywhere
        expect_ngal, expect_xi = oracle_values(case, True)
        pairs = [(want['ngal_' + key], expect_ngal[key]) for key in expect_ngal]
        pairs += [(want['xi_' + key], expect_xi[key]) for key in expect_xi]
        for got, expect in pairs:
            assert np.array_equal(np.isnan(got), np.isnan(expect))
            assert np.array_equal(np.isinf(got), np.isinf(expect))
            assert np.array_equal(np.signbit(got[np.isinf(got)]),
                                  np.signbit(expect[np.isinf(expect)]))
            finite = np.isfinite(expect)
            assert_rel(got[finite], expect[finite], RTOL, 'degenerate draws', floor=1e-13)


@pytest.mark.parametrize('name, case', CASES, ids=[name for name, _ in CASES])
def test_same_bits_as_the_parent_commit(name, case, parent, oracle_values):
    want = parent[name]
    got = recorder.run_case(case)           # (asserts that the form asked for ran)
    assert sorted(got) == sorted(want)
    assert tuple(got['launch']) == tuple(want['launch'])
    for key in want:
        if key != 'launch':
            assert got[key].shape == want[key].shape
            assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), key
            differing = int(np.sum(got[key].view(np.uint64) != want[key].view(np.uint64)))
            assert differing == 0, '%s: %d of %d words differ from the parent\'s' % (
                key, differing, want[key].size)
    check_against_oracle(case, want, oracle_values)


def test_the_recorded_cases_are_the_ones_asked_for(parent):
    """81 draws (two tiles, the second partial), synthetic tables; per case the launch is the
    form asked for."""
    cases = dict(CASES)
    assert set(parent) == set(cases)
    assert recorder.N_DRAWS == 81
    shapes = {name: (case['shape'], case['grid'], case['mode'], case['dtype'])
              for name, case in CASES}

    def has(name, shape, grid=None, mode='cross', dtype='float64'):
        assert shapes[name] == (shape, grid, mode, dtype), name
    # register form: total and separated, several workgroups per tile and one; decorated;
    # likelihood; degenerate draws
    for tag in ('_tot', '_sep'):
        has('register' + tag, (20, 1, 13))
        has('register_one' + tag, (20, 1, 13))
        has('register_assembias' + tag, (20, 2, 13))
        has('register_modulate' + tag, (9, 3, 5))
        assert cases['register_assembias' + tag]['assembias']
        assert cases['register_modulate' + tag]['modulate']
        # chunk form per instance, deferred pairs asked for and not; one workgroup per tile
        for setting in ('_on', '_off'):
            has('chunk32' + setting + tag, (9, 3, 19))
            has('chunk64' + setting + tag, (30, 2, 40))
        has('chunk32_on_one' + tag, (9, 3, 19))
        has('wide' + tag, (40, 2, 13))
        has('interp4' + tag, (20, 2, 13), (4, ))
        has('interp4x4' + tag, (10, 2, 3), (4, 4))
        assert cases['interp4x4' + tag]['vary_n_h']
        has('three_table' + tag, (20, 2, 13))
        has('three_interp4' + tag, (20, 2, 13), (4, ))
        has('three_f32' + tag, (10, 2, 7), dtype='float32')
    has('register_chi2', (20, 1, 13))
    has('chunk128_tot', (10, 2, 100))
    has('chunk32_on_chi2', (9, 3, 19))
    has('chunk32_off_chi2', (9, 3, 19))
    has('interp4_chi2', (20, 2, 13), (4, ))
    has('register_degenerate_sep', (20, 1, 13))
    has('chunk32_degenerate_sep', (9, 3, 19))
    has('three_auto_chi2', (10, 1, 19), mode='auto')
    has('small_cross4x4', (10, 2, 3), (4, 4))
    has('small_auto4', (10, 1, 19), (4, ), mode='auto')
    for name in ('register_chi2', 'chunk32_on_chi2', 'chunk32_off_chi2', 'chunk32_deferred_chi2',
                 'interp4_chi2', 'three_auto_chi2'):
        assert cases[name]['chi2'] and 'chi2' in parent[name]
    for name in ('register_degenerate_sep', 'chunk32_degenerate_sep'):
        assert cases[name]['degenerate'] and cases[name]['separate']
        # (the degenerate draws left their mark: NaN results, and not only NaN)
        for key in ('xi_centrals', 'xi_satellites'):
            bad = np.isnan(parent[name][key]).any(axis=-1)
            assert bad.any() and not bad.all()
    # the launches
    lds = {name: int(result['launch'][3]) for name, result in parent.items()}
    for name, result in parent.items():
        assert recorder.launch_is_the_form(cases[name], result['launch']), name
    for name in ('register_tot', 'register_sep', 'chunk32_on_tot', 'chunk32_deferred_tot'):
        assert parent[name]['launch'][0] > 2            # several workgroups per tile
    for name in ('register_one_tot', 'register_one_sep', 'chunk32_on_one_tot',
                 'chunk32_on_one_sep', 'chunk32_off_one_tot', 'chunk32_deferred_one_tot'):
        assert parent[name]['launch'][0] == 2
    # (kernel_args.h: the register form's LDS depends on the components alone; the chunk form's
    # is larger, whatever the rows)
    for name, case in CASES:
        if case['form'] == 'register':
            assert lds[name] == lds['register_sep' if case['separate'] else 'register_tot'], name
    assert lds['wide_tot'] > lds['register_tot'] and lds['wide_sep'] > lds['register_sep']
    assert lds['chunk32_on_tot'] > lds['register_tot']
    assert lds['chunk32_on_tot'] < lds['chunk64_on_tot'] < lds['chunk128_tot']
    # (the deferred pairs' bitmap lies behind the buffers: kernel_args.h)
    for rows in (32, 64):
        assert (lds['chunk%d_deferred_tot' % rows] > lds['chunk%d_undeferred_tot' % rows])
    assert lds['chunk32_deferred_chi2'] == lds['chunk32_deferred_tot']
    assert lds['chunk32_deferred_one_tot'] == lds['chunk32_deferred_tot']
