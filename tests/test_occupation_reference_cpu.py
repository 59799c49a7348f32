"""tests/occupation_reference.py on the CPU: the extended reference against the oracle and
against mpmath, the per-bin readout through oracle.predict, the draws that fill every stratum of
every table of tests/test_gpu_occupation_forms.py, and the host hooks (the kernels' inline code)
against the reference per stratum -- the measurements the device allowances come from."""

import numpy as np
import pytest

import occupation_reference as ref
from oracle import tabcorr_oracle as oracle

VARIANTS = [(False, False), (True, False), (False, True), (True, True)]   # (modulate, decorated)
MIN_PAIRS = 64
MIN_TOP = 8


@pytest.mark.parametrize('name', sorted(ref.TABLES))
def test_reference_agrees_with_the_oracle(name):
    """The float64 oracle to 1e-13 (centrals absolute, satellites relative to the unmodulated
    value -- the oracle's own erf and pow are libm-grade, its M0 the correctly rounded 10**x;
    the ill-conditioned pairs, where the rounding of M0 alone exceeds that, aside)."""
    p = ref.prepared(name)
    table, theta, strengths = p['table'], p['theta'], p['strengths']
    sample = np.arange(0, len(theta), 16)
    for modulate, decorated in VARIANTS:
        occupation, scale, labels = ref.prepared_reference(name, 10, modulate, decorated)
        with np.errstate(all='ignore'):
            expect = np.array([oracle.mean_occupation(
                table, oracle.Zheng07(theta[i], modulate, strengths[i] if decorated else None))
                for i in sample])
        errors = ref.pair_errors(expect, occupation[sample], p['central'], scale[sample])
        ill = labels['stratum'][sample] == ref.SAT_ILL
        assert np.max(errors[~ill]) < 1e-13, (name, modulate, decorated, np.max(errors[~ill]))


def test_reference_agrees_with_mpmath():
    """40 digits on a few hundred (bin, draw) pairs of every kind: the reference's own error is
    below 1e-17 absolute (centrals: erf from float64 with its first-order correction) and 1e-17
    relative (satellites; the ill-conditioned pairs aside, where the longdouble M0's own
    rounding is multiplied by KAPPA), far below anything asserted against it."""
    mpmath = pytest.importorskip('mpmath')
    mpmath.mp.dps = 40
    rng = np.random.default_rng(2)
    checked = 0
    for name in ('50x1', '7x3', 'narrow2'):
        p = ref.prepared(name)
        n_bins = len(p['table']['gal_type'])
        for modulate, decorated in VARIANTS:
            occupation, scale, labels = ref.prepared_reference(name, 10, modulate, decorated)
            for _ in range(20):
                i, b = int(rng.integers(len(p['theta']))), int(rng.integers(n_bins))
                exact = ref.mpmath_occupation(
                    p['table'], p['theta'][i], b, 10, modulate,
                    p['strengths'][i] if decorated else None)
                difference = abs(ref_mpf(occupation[i, b]) - exact)
                if p['central'][b]:
                    assert float(difference) < 2e-16, (name, i, b)       # (scipy's erf: 1.2e-16)
                    checked += 1
                    continue
                # (relative to the unmodulated value, as everywhere)
                error = 0.0 if difference == 0 else float(difference / ref_mpf(scale[i, b]))
                if labels['stratum'][i, b] == ref.SAT_ILL:
                    # (KAPPA times the 1.1e-19 of the longdouble M0)
                    assert error < 1e-15, (name, i, b, error, modulate, decorated)
                else:
                    assert error < (2e-16 if modulate else 1e-17), (name, i, b, error, modulate,
                                                                    decorated)
                checked += 1
    assert checked == 240


def ref_mpf(value):
    """A longdouble as an exact mpmath number."""
    import mpmath
    high = float(value)
    return mpmath.mpf(high) + mpmath.mpf(float(value - np.longdouble(high)))


@pytest.mark.parametrize('mode', ['auto', 'cross'])
@pytest.mark.parametrize('name', ['12x1', '7x3'])
def test_readout_recovers_the_occupations(name, mode):
    """oracle.predict with the selector tables returns the occupations it was given: the zeros
    of the 0 / 1 matrices are exact, what is left is the rounding of ngal, the row and the
    square root."""
    table = ref.make_table(name, mode)
    p = ref.prepared(name)
    theta = p['theta'][::16]
    occupation = np.array([oracle.mean_occupation(table, oracle.Zheng07(t)) for t in theta])
    selectors = ref.selector_tables(table)
    assert len(selectors) == -(-len(table['gal_type']) // ref.N_R[mode])
    for selector in selectors:
        assert set(np.unique(selector['tpcf_matrix'])) <= {0.0, 1.0}
        assert np.all(np.sum(selector['tpcf_matrix'], axis=1) <= 1)
    results = []
    for selector in selectors:
        predictions = [oracle.predict(selector, n) for n in occupation]
        results.append((np.array([r[0] for r in predictions]),
                        np.array([r[1] for r in predictions])))
    got = ref.readout(table, results).astype(np.float64)
    np.testing.assert_allclose(got, occupation, rtol=4 * ref.EPS, atol=0)


@pytest.mark.parametrize('name', sorted(ref.TABLES))
def test_draws_fill_every_stratum(name):
    """Finite draws; every stratum the table has holds at least 64 (bin, draw) pairs, every
    term count pairs at the top of its stratum (the count changes within 2 per cent of 1 / sigma
    resp. M0) and just beyond it; the uniform order has whole 64-draw tiles on the wave-uniform
    shortcuts; both orders hold every draw once."""
    p = ref.prepared(name)
    theta, labels = p['theta'], ref.prepared_reference(name)[2]
    assert theta.shape == (1536, 5) and np.all(np.isfinite(theta))
    assert np.all(np.abs(theta[:, 1]) >= ref.SIGMA_MIN)
    for order in p['orders'].values():
        assert np.array_equal(np.sort(order), np.arange(len(theta)))
    expected = ref.expected_strata(p['table'], p['limits'])
    counts = ref.stratum_maxima(np.zeros(labels['stratum'].shape), labels['stratum'],
                                p['central'])
    for kind in ('cen', 'sat'):
        for stratum in expected[kind]:
            assert counts.get((kind, stratum), (0, ))[0] >= MIN_PAIRS, (name, kind, stratum)
        columns = p['central'] if kind == 'cen' else ~p['central']
        for terms in (ref.CEN_TERMS if kind == 'cen' else ref.SAT_TERMS):
            if terms not in expected[kind]:
                continue
            at_top = labels['top'][:, columns] & (labels['stratum'][:, columns] == terms)
            assert np.sum(at_top) >= MIN_TOP, (name, kind, terms)
    # what the tables are there for
    if name == '50x1':
        assert expected['sat'] >= {20, 24, 28, 32} and expected['cen'] >= {8, 12, 16, 20, 24}
        assert np.all(labels['shortest'][~p['central']] > 0)     # (the defer and latency forms)
    if name.startswith('narrow'):
        assert expected['sat'] >= set(ref.SAT_TERMS) and expected['cen'] >= {8, 12}
        assert np.all(labels['shortest'][~p['central']] > 0)
    # whole tiles of one kind in the uniform order: plateaus at 1 and below M0 for every lane
    stratum = labels['stratum'][p['orders']['uniform']]
    tiles = stratum.reshape(len(theta) // 64, 64, -1)
    uniform = np.all(tiles == tiles[:, :1], axis=1)              # (tile, bin)
    for kind, value in (('cen', ref.CEN_PLATEAU_1), ('sat', ref.SAT_BELOW)):
        columns = p['central'] if kind == 'cen' else ~p['central']
        assert np.sum(uniform[:, columns] & (tiles[:, 0][:, columns] == value)) >= 4, (name, kind)
    if ref.CEN_PLATEAU_0 in expected['cen']:
        assert np.sum(uniform[:, p['central']] &
                      (tiles[:, 0][:, p['central']] == ref.CEN_PLATEAU_0)) >= 4, name
    # ... and none in the shuffled one, bar the bins that are uniform for the whole batch
    shuffled = labels['stratum'][p['orders']['shuffled']].reshape(len(theta) // 64, 64, -1)
    mixed = ~np.all(shuffled == shuffled[:, :1], axis=1)
    assert np.mean(mixed) > 0.9, name


@pytest.mark.parametrize('name', ['50x1', 'narrow', '9x2', '12x1'])
def test_thirty_two_draws_for_the_unbatched_kernel(name):
    """The 32 draws the un-batched kernel gets, one call each, hold 8 pairs of every stratum
    the table has (64 do not fit: the longest satellite expansions serve a bin per draw)."""
    p = ref.prepared(name)
    rows = ref.pick_draws(name, 32, 8)
    assert len(set(rows.tolist())) == 32
    stratum = ref.prepared_reference(name)[2]['stratum'][rows]
    expected = ref.expected_strata(p['table'], p['limits'])
    for kind in ('cen', 'sat'):
        columns = p['central'] if kind == 'cen' else ~p['central']
        for value in expected[kind]:
            assert np.sum(stratum[:, columns] == value) >= 8, (name, kind, value)


def test_host_hooks_against_the_reference_per_stratum(capsys):
    """The kernels' inline code on the host (tc_debug_central_series, tc_debug_satellite_series:
    the expansion and the node loop of every pair) against the reference: the maxima recorded in
    occupation_reference.HOST_MAX hold, and no allowance made of them exceeds 1e-13."""
    measured = {}
    for name in sorted(ref.TABLES):
        p = ref.prepared(name)
        for n_gauss in (10, 4):
            occupation, _, labels = ref.prepared_reference(name, n_gauss)
            for kind in ('series', 'nodes'):
                errors = ref.pair_errors(labels[kind], occupation, p['central'])
                for cell, (count, worst) in ref.stratum_maxima(errors, labels['stratum'],
                                                               p['central']).items():
                    before = measured.get(cell, (0, 0.0))
                    measured[cell] = (before[0] + count, max(before[1], worst))
    with capsys.disabled():
        print()
        for cell in sorted(measured):
            print('host hooks %s %-4d pairs %8d  max %.3e  recorded %s' % (
                cell + measured[cell] + (ref.HOST_MAX.get(cell), )))
    assert set(measured) - {('sat', ref.SAT_ILL)} == set(ref.HOST_MAX)
    for cell, recorded in ref.HOST_MAX.items():
        assert measured[cell][1] <= recorded, (cell, measured[cell], recorded)
        for modulate in (False, True):
            for decorated in (False, True):
                assert ref.allowance(cell[0], cell[1], modulate, decorated) <= ref.LIMIT
    # the ill-conditioned pairs are what they are said to be: a minority, and beyond the others
    ill = measured[('sat', ref.SAT_ILL)]
    assert ill[0] < 0.1 * sum(count for count, _ in measured.values())
