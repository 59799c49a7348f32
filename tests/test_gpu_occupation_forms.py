"""The occupation arithmetic ON THE DEVICE, per bin and per branch, in every kernel form.

Every form of the Zheng07 kernels computes the mean occupations for itself; only
occ_zheng07_kernel's were ever read by a test, and the tight checks of the expansions ran on the
host.  Here each form predicts from tables whose correlation matrix is 0 / 1 (tests/
occupation_reference.py: selector_tables), which returns its in-kernel occupations to a few ulp,
for draws placed at the top of and just beyond every stratum (number of terms of a lane's
expansion, plateaus, bins below M0, alpha at and outside [0, 4], negative sigma), shuffled -- a
wave holds lanes of every kind -- and with whole 64-draw tiles of one kind (the wave-uniform
shortcuts fire).  Each (bin, draw) pair is compared with the extended reference within the
allowance of its stratum: 4 x the error of the same inline code on the host
(occupation_reference.HOST_MAX), centrals absolute, satellites relative (modulated: to the
unmodulated value).  The form that ran is asserted from tc_table_last_launch after every call.

Which expansions a form really takes (series = 3): occ_zheng07_kernel, the 8 x 64 and 16 x 64
forms and the mode-cross one-launch kernel of more than 16 rows: both; with modulate no
satellite expansion, decorated no central one; the deferring 8 x 64 instances and the latency
form (8 x 40): the satellites' shortest expansion per bin only (occ_sat_record), the other pairs
by the deferred node loop; the halves (8 x 32), predict_cross_small_kernel and the un-batched
kernel: node loops only.  The strata are those of the hooks at series = 3 whatever the form
takes: where a form runs the node loop for a pair of a term-count stratum, that is what is
checked there, against the same allowance.

Cells a form cannot reach: strata a table does not have (occupation_reference.expected_strata:
no satellite expansion on bins wider than ~0.2 dex -- 12x1, 9x2, 7x3 --, 12 and 16 satellite
terms only on the narrow tables, no central node loop, 20 or 24 terms and no plateau at 0 on the
narrow tables, whose limits lie below SIGMA_MIN resp. whose span is 0.3 dex); the un-batched
kernel's 32 draws cannot hold 64 pairs of a stratum that has a bin or two per draw: 8 there.

Out of scope: the resident kernels (they share single_draw_body; their bit equality is tested
in test_gpu_async.py), the Leauthaud11 forward kernels, the gradient kernels (their own kits),
float32 tables (their occupations are float64 anyway).  Needs an MI355X."""

import ctypes

import numpy as np
import pytest

import occupation_reference as ref

pytestmark = pytest.mark.gpu

MIN_PAIRS = 64
UNBATCHED_MIN_PAIRS = 8        # (see the module docstring)
UNBATCHED_CASES = [('50x1', False, False), ('narrow', False, False), ('9x2', True, True),
                   ('12x1', False, False)]
_HANDLES = {}


def make_tabcorr(table):
    from tabcorr_amd import TabCorr
    return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                               table['attrs'])


def set_option(halotab, name, value):
    from tabcorr_amd import _lib
    _lib.check(_lib.load().tc_table_set_option(halotab.to_device().handle, name.encode(), value))


def last_launch(halotab):
    from tabcorr_amd import _lib
    values = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.load().tc_table_last_launch(halotab.to_device().handle,
                                                *[ctypes.byref(v) for v in values]))
    return tuple(v.value for v in values)


def selectors(name, mode, n_r):
    """The selector tables of a table on the device, made once per process."""
    key = (name, mode, n_r)
    if key not in _HANDLES:
        table = ref.make_table(name, mode, n_r)
        _HANDLES[key] = (table, [make_tabcorr(s) for s in ref.selector_tables(table, n_r)])
    return _HANDLES[key]


def batch_of(p, rows, decorated):
    theta = p['theta'][rows]
    return np.hstack([theta, p['strengths'][rows]]) if decorated else theta


def report(form, name, cells):
    for cell in sorted(cells):
        count, worst, limit = cells[cell]
        print('%-28s %-8s %s %-4d pairs %7d  max %.2e  allowed %.2e' % (
            (form, name) + cell + (count, worst, limit)))


def check(form, name, values, rows, min_pairs=MIN_PAIRS, **variant):
    """Compare, print, and assert the cells' counts and allowances."""
    p = ref.prepared(name)
    cells, failed = ref.check_cells(name, values, rows, what=form, **variant)
    report(form, name, cells)
    expected = ref.expected_strata(p['table'], p['limits'])
    for kind in ('cen', 'sat'):
        for stratum in expected[kind]:
            assert cells.get((kind, stratum), (0, ))[0] >= min_pairs, (form, name, kind, stratum)
    assert not failed, failed
    return cells


# ---- occ_zheng07_kernel through mean_occupation_batch -------------------------------------------

OCC_CASES = [(name, grouped, series, n_gauss, modulate, decorated)
             for name in sorted(ref.TABLES)
             for grouped, series, n_gauss, modulate, decorated in (
                 [(1, series, 10, m, d) for series in (0, 1, 3)
                  for m, d in ((False, False), (True, False), (False, True), (True, True))] +
                 [(0, 3, 10, False, False), (0, 3, 10, True, True),
                  (1, 3, 4, False, False), (1, 3, 4, True, True), (0, 3, 4, False, True)])
             if grouped == 1 or ref.TABLES[name] in ((9, 2), (7, 3), 'narrow2')]


@pytest.mark.parametrize('name, grouped, series, n_gauss, modulate, decorated', OCC_CASES)
def test_occupation_kernel(name, grouped, series, n_gauss, modulate, decorated):
    p = ref.prepared(name)
    _, tables = selectors(name, 'auto', ref.N_R['auto'])
    halotab = tables[0]
    set_option(halotab, 'grouped', grouped)
    set_option(halotab, 'series', series)
    for order in ('shuffled', 'uniform'):
        rows = p['orders'][order]
        got = halotab.mean_occupation_batch(batch_of(p, rows, decorated), n_gauss_prim=n_gauss,
                                            modulate_with_cenocc=modulate, assembias=decorated)
        check('occ g%d s%d n%d %s' % (grouped, series, n_gauss, order), name, got, rows,
              n_gauss=n_gauss, modulate=modulate, decorated=decorated)
    set_option(halotab, 'grouped', 1)


# ---- predict_fused_kernel -----------------------------------------------------------------------

def fused_options(halotab, **options):
    base = {'fused': 2, 'fused_min_draws': 1, 'single_draw': 0, 'series': 3, 'fused_waves': 0,
            'fused_draws': 64, 'fused_defer': 0, 'sync_chunks': 0}
    base.update(options)
    for key, value in base.items():
        set_option(halotab, key, value)


def predict_occupations(name, mode, n_r, rows, decorated, modulate, options, ran):
    """The in-kernel occupations of the draws `rows` from every selector table; `ran(halotab,
    n_draws)` confirms the form after each call."""
    p = ref.prepared(name)
    table, tables = selectors(name, mode, n_r)
    batch = batch_of(p, rows, decorated)
    results = []
    for halotab in tables:
        options(halotab)
        ngal, xi = halotab.predict_batch(batch, modulate_with_cenocc=modulate,
                                         assembias=decorated)
        assert ran(halotab, len(batch)), last_launch(halotab)
        results.append((ngal, xi))
    return ref.readout(table, results, n_r)


FUSED_FORMS = {
    # name: (options, (workgroup draws, waves))
    '8x64 defer 0': ({'fused_waves': 8, 'fused_defer': 0}, (64, 8)),
    '8x64 defer 1': ({'fused_waves': 8, 'fused_defer': 1}, (64, 8)),
    '8x64 defer 2': ({'fused_waves': 8, 'fused_defer': 2}, (64, 8)),
    '16x64': ({'fused_waves': 16}, (64, 16)),
    '8x32 halves': ({'fused_draws': 32}, (32, 8)),
    '8x40 latency': ({'fused_draws': 40, 'sync_chunks': 1, 'fused_defer': 2}, (40, 8)),
}
FUSED_CASES = (
    [('8x64 defer 0', name, False, False) for name in ('12x1', '50x1', '9x2', '7x3', 'narrow')] +
    [('8x64 defer 0', '9x2', True, False), ('8x64 defer 0', '7x3', False, True),
     ('8x64 defer 0', 'narrow2', True, True)] +
    [(form, name, False, False) for form in ('8x64 defer 1', '8x64 defer 2', '8x40 latency')
     for name in ('50x1', 'narrow')] +
    [('16x64', '50x1', False, False), ('16x64', '9x2', False, True)] +
    [('8x32 halves', name, False, False) for name in ('12x1', '50x1', '7x3')] +
    [('8x32 halves', '9x2', False, True), ('8x32 halves', 'narrow2', True, True)])


@pytest.mark.parametrize('form, name, modulate, decorated', FUSED_CASES)
def test_fused_forms(form, name, modulate, decorated):
    options, (draws, waves) = FUSED_FORMS[form]

    def ran(halotab, n):
        # (test_gpu_fused.py: fused_ran / latency_form_ran, and the 32-draw form's workgroups)
        workgroups, got_waves, slabs, _ = last_launch(halotab)
        return workgroups == (n + draws - 1) // draws and got_waves == waves and slabs == 0
    p = ref.prepared(name)
    for order in ('shuffled', 'uniform'):
        rows = p['orders'][order]
        got = predict_occupations(name, 'auto', ref.N_R['auto'], rows, decorated, modulate,
                                  lambda halotab: fused_options(halotab, **options), ran)
        check('fused %s %s' % (form, order), name, got, rows, modulate=modulate,
              decorated=decorated)


# ---- mode cross ---------------------------------------------------------------------------------

CROSS_CASES = (
    # more than 16 rows: predict_cross_fused_kernel, deferred pairs on and off
    [('fused', 16, name, defer, False, False) for name in ('50x1', '9x2', '7x3', 'narrow2')
     for defer in (1, 0)] +
    [('fused', 16, '9x2', 1, True, False), ('fused', 16, '7x3', 1, False, True)] +
    # up to 16 rows: predict_cross_small_kernel, and the 32-row chunk form from
    # cross_wide_min_draws draws on (groups of at most two bins)
    [('small', 15, name, 1, False, False) for name in ('12x1', '9x2', 'narrow2', '7x3')] +
    [('small', 15, '9x2', 1, True, True)] +
    [('wide', 15, name, 1, False, False) for name in ('9x2', 'narrow2', '50x1')])


@pytest.mark.parametrize('form, n_r, name, defer, modulate, decorated', CROSS_CASES)
def test_cross_forms(form, n_r, name, defer, modulate, decorated):
    p = ref.prepared(name)
    seen = {}

    def options(halotab):
        for key, value in (('fused', 2), ('fused_min_draws', 1), ('single_draw', 0),
                           ('series', 3), ('cross_defer', defer),
                           ('cross_wide_min_draws', 1 if form == 'wide' else 0)):
            set_option(halotab, key, value)

    def ran(halotab, n):
        # (test_gpu_cross_fused.py: cross_ran; the chunk form differs from the register form in
        # its LDS)
        workgroups, waves, slabs, lds = last_launch(halotab)
        tiles = (n + 63) // 64
        seen[id(halotab)] = lds
        return (waves == 8 and slabs == 0 and workgroups % tiles == 0 and
                1 <= workgroups // tiles <= 8)
    for order in ('shuffled', 'uniform'):
        rows = p['orders'][order]
        got = predict_occupations(name, 'cross', n_r, rows, decorated, modulate, options, ran)
        check('cross %s defer %d %s' % (form, defer, order), name, got, rows, modulate=modulate,
              decorated=decorated)
    if form == 'wide':
        # the register form's launch on the same handles: another LDS size
        _, tables = selectors(name, 'cross', n_r)
        for halotab in tables:
            set_option(halotab, 'cross_wide_min_draws', 0)
            halotab.predict_batch(p['theta'][:64])
            assert last_launch(halotab)[3] != seen[id(halotab)], 'the chunk form did not run'


# ---- the un-batched kernel ------------------------------------------------------------------------

@pytest.mark.parametrize('name, modulate, decorated', UNBATCHED_CASES)
def test_unbatched_kernel(name, modulate, decorated):
    """32 draws, one call each, through single_draw_kernel (option "resident" 0: one launch per
    call): no batched kernel ran on the handle -- tc_table_last_launch stays at zero -- and no
    resident one."""
    from tabcorr_amd import _lib
    p = ref.prepared(name)
    rows = ref.pick_draws(name, 32, UNBATCHED_MIN_PAIRS)
    table = ref.make_table(name)
    tables = [make_tabcorr(s) for s in ref.selector_tables(table)]      # (fresh handles)
    results = []
    for halotab in tables:
        for key, value in (('single_draw', 1), ('resident', 0), ('series', 3)):
            set_option(halotab, key, value)
        ngal, xi = [], []
        for row in rows:
            n, x = halotab.predict_batch(batch_of(p, [row], decorated),
                                         modulate_with_cenocc=modulate, assembias=decorated)
            ngal.append(n[0])
            xi.append(x[0])
        assert last_launch(halotab) == (0, 0, 0, 0)
        launches, running = ctypes.c_int64(-1), ctypes.c_int(-1)
        _lib.check(_lib.load().tc_table_resident_stats(
            halotab.to_device().handle, ctypes.byref(launches), None, None,
            ctypes.byref(running)))
        assert launches.value == 0 and running.value == 0
        results.append((np.array(ngal), np.array(xi)))
    got = ref.readout(table, results)
    check('un-batched', name, got, rows, min_pairs=UNBATCHED_MIN_PAIRS, modulate=modulate, decorated=decorated)
