"""Per-bin mean occupations in extended precision, a readout that makes any prediction kernel
return its own in-kernel occupations, and draws placed by the per-lane branch they take.

TEST INFRASTRUCTURE (tests/test_occupation_reference_cpu.py, tests/test_gpu_occupation_forms.py).

Reference
---------
`reference_occupation` does what ``oracle.mean_occupation`` does (tabcorr/tabcorr.py:537-578) for
plain Zheng07, ``modulate_with_cenocc`` and Zheng07 decorated at the median split, with every
operation in ``np.longdouble`` (64-bit mantissa): log10 of the node masses, 10**x, the powers,
the weights and the sums.  Its inputs are what the reference hands to the model callbacks: the
node masses as float64 numbers (tabcorr.py:548 forms ``10**(...)`` in float64), so that it shares
its nodes with the kernels; erf comes from scipy in float64 (absolute error <= 1.2e-16) with the
first-order correction for the rounding of its argument.

Conditioning (why the draws are what they are)
----------------------------------------------
The kernels hold log10 M_k of a node as a float64: a rounding of <= 8.9e-16 at log10 M ~ 12,
which the central occupation sees through d<N_cen>/dlog M <= 0.564 / sigma.  With
|sigma| >= SIGMA_MIN = 0.03 that is <= 1.7e-14, inside the allowances; below, the node loop is
right to ~1e-15 / sigma whatever it does, so such draws measure the conditioning, not the
kernel.  Likewise (M_k - M0)^alpha with M0 = exp10(logM0) (relative error <= 6e-16): a node a
relative distance g above M0 carries an error 6e-16 alpha / g.  `snap_m0` therefore moves every
M0 that falls between two nodes of a satellite bin to their midpoint, at most five nodes deep
into a bin (at least five nodes then lie above it and the nearest one's share of the sum is a few
per cent), and draws with alpha < 0 -- where the nearest node dominates -- keep M0 below the
table.  What is left is measured, not guessed: `reference_occupation` returns the condition
number KAPPA of every satellite pair with respect to M0, and the pairs beyond KAPPA_MAX are
counted under SAT_ILL and not asserted on (2 per cent of all pairs; the hooks' error there
reaches 6e-12, all of it the rounding of M0).

Allowances (issue section 5; measured by test_occupation_reference_cpu.py)
-------------------------------------------------------------------------
HOST_MAX holds, per galaxy type, stratum and kind ('series': the expansion the kernels take,
'nodes': the node loop), the largest error of the host hooks (tc_debug_central_series /
tc_debug_satellite_series: the kernels' inline code run on the host) against the reference over
the pairs of all tables of `TABLES`, both batches.  Centrals: absolute; satellites: relative.
The device allowance is 4 x that maximum, never below FLOOR = 8 ulp: the device adds only
changes of rounding order -- 5 + 5 nodes in the halves, FMA contraction, the Newton reciprocal,
the product with n_h, the sum with exact zeros, the division by ngal, the square root --, each
about an ulp, which the host measurement cannot see where it is exact (plateaus, alpha = 0).
"""

import ctypes

import numpy as np

EPS = 2.0**-52
FLOOR = 8 * EPS
SIGMA_MIN = 0.03
LIMIT = 1e-13           # no allowance may exceed it (issue section 5)

# strata: the number of terms of the expansion the draw's lane takes for the bin, 0 = the node
# loop, and the branches next to them
CEN_NODES, CEN_PLATEAU_1, CEN_PLATEAU_0, CEN_NEGATIVE = 0, 100, 101, 102
CEN_TERMS = (8, 12, 16, 20, 24)
SAT_NODES, SAT_BELOW, SAT_INSIDE, SAT_ALPHA_OUT, SAT_ALPHA_0, SAT_ALPHA_4 = 0, 200, 201, 202, 203, 204
SAT_TERMS = (12, 16, 20, 24, 28, 32)
# KAPPA = |d ln <N_sat> / d ln M0| = alpha M0 sum_k W_k (M_k - M0)^(alpha - 1) / sum_k W_k (M_k - M0)^alpha,
# the condition number of a satellite bin with respect to M0 (`reference_occupation` returns it):
# the rounding of M0 = exp10(logM0) itself, <= 6e-16 in the kernels, reaches the bin multiplied
# by it, whatever the kernel does afterwards.  Pairs beyond KAPPA_MAX measure the conditioning of
# the formula, not the kernel: they are counted (stratum SAT_ILL) and not asserted on.
SAT_ILL = 299
KAPPA_MAX = 24.0
NAMES = {('cen', 0): 'node loop', ('cen', 100): 'plateau at 1', ('cen', 101): 'plateau at 0',
         ('cen', 102): 'negative sigma', ('sat', 0): 'node loop',
         ('sat', 200): 'every node at or below M0', ('sat', 201): 'M0 inside the bin',
         ('sat', 202): 'alpha outside [0, 4]', ('sat', 203): 'alpha = 0', ('sat', 204): 'alpha = 4'}

# Measured host maxima (tests/test_occupation_reference_cpu.py::
# test_host_hooks_against_the_reference_per_stratum measures them again and prints them;
# 2026-10-19, on top of commit 1362556): per (type, stratum) the largest error of the hooks'
# expansion and node loop over the tables of TABLES, n_gauss_prim 10 and 4.
HOST_MAX = {
    ('cen', 0): 2.9e-16,
    ('cen', 8): 2.2e-16,
    ('cen', 12): 4.3e-16,
    ('cen', 16): 6.9e-16,
    ('cen', 20): 2.5e-16,
    ('cen', 24): 8.3e-16,
    ('cen', 100): 1.2e-16,
    ('cen', 101): 1.2e-16,
    ('cen', 102): 2.4e-16,
    ('sat', 0): 5.8e-15,
    ('sat', 12): 5.1e-15,
    ('sat', 16): 5.8e-15,
    ('sat', 20): 6.4e-15,
    ('sat', 24): 5.7e-15,
    ('sat', 28): 7.3e-15,
    ('sat', 32): 5.1e-15,
    ('sat', 200): 0.0e+00,
    ('sat', 201): 5.8e-15,
    ('sat', 202): 6.7e-15,
    ('sat', 203): 5.8e-16,
    ('sat', 204): 8.0e-15,
}
# (the modulation multiplies a satellite node by <N_cen> from the node loop's erf: its absolute
# error, the largest over the centrals' strata, enters relative to the unmodulated value)
CEN_NODE_MAX = max(value for (kind, _), value in HOST_MAX.items() if kind == 'cen')


def allowance(kind, stratum, modulate=False, decorated=False):
    """The device allowance of a ('cen' | 'sat', stratum) cell: 4 x the host maximum, at least
    FLOOR.  Centrals absolute, satellites relative (modulated: to the unmodulated value, and
    with the centrals' node-loop error on top).  Decorated centrals: n + s min(n, 1 - n) has
    slope <= 2 in n; decorated satellites are n (1 +- s): the relative error stays."""
    base = HOST_MAX[kind, stratum]
    if kind == 'sat' and modulate:
        base = base + CEN_NODE_MAX
    value = max(4.0 * base, FLOOR)
    if kind == 'cen' and decorated:
        value *= 2.0
    return value


# ---- tables -----------------------------------------------------------------------------------

def narrow_table(n_sec=1, mode='auto', n_r=19, n_prim=24, seed=3):
    """Bins of 0.0125 dex (the reference's AbacusSummit tables have 0.0121): the 8- and 12-term
    central strata at ordinary sigma, the 12- and 16-term satellite strata at all."""
    from tabcorr_amd import synthetic
    table = synthetic.synthetic_table(n_prim, n_sec, (n_r, ), mode, seed=seed)
    table['gal_type'] = synthetic.synthetic_gal_type(n_prim, n_sec, seed=seed, log_m_min=12.0,
                                                     log_m_max=12.0 + 0.0125 * n_prim)
    return table


# name -> (n_prim, n_sec) of synthetic_table, or 'narrow'
TABLES = {'12x1': (12, 1), '50x1': (50, 1), '9x2': (9, 2), '7x3': (7, 3), 'narrow': 'narrow',
          'narrow2': 'narrow2'}
N_R = {'auto': 19, 'cross': 16}


def make_table(name, mode='auto', n_r=None):
    from tabcorr_amd import synthetic
    n_r = N_R[mode] if n_r is None else n_r
    if name == 'narrow':
        return narrow_table(1, mode, n_r)
    if name == 'narrow2':
        return narrow_table(2, mode, n_r, n_prim=16)
    n_prim, n_sec = TABLES[name]
    return synthetic.synthetic_table(n_prim, n_sec, (n_r, ), mode, seed=n_prim)


def is_centrals(gal_type):
    column = gal_type['gal_type']
    return (column == b'centrals') | (column == 'centrals')


def node_masses(gal_type, n_gauss=10):
    """(n_bins, n_gauss) float64 node masses and the Gauss-Legendre weights, as
    tabcorr/tabcorr.py:544-549 forms them."""
    x, w = np.polynomial.legendre.leggauss(n_gauss)
    x = (x + 1) / 2
    log_min = gal_type['log_prim_haloprop_min']
    d_log = gal_type['log_prim_haloprop_max'] - log_min
    return 10**(log_min[:, np.newaxis] + d_log[:, np.newaxis] * x), w


# ---- the reference ----------------------------------------------------------------------------

def _erf(z):
    """erf of a longdouble array: scipy's float64 erf plus the first-order term of the
    argument's rounding."""
    from scipy.special import erf
    z64 = z.astype(np.float64)
    dz = z - z64.astype(np.longdouble)
    gauss = 2 / np.sqrt(np.pi * np.longdouble(1)) * np.exp(-z64.astype(np.longdouble)**2)
    return erf(z64).astype(np.longdouble) + dz * gauss


def _decorate(n, strength, above, upper):
    """Heaviside assembly bias at the median split (oracle.heaviside_assembias, f1 = f2 = 1/2)
    of the node values n (draws, bins, nodes); strength (draws, ); above (bins, )."""
    one = np.longdouble(1)
    strength = np.clip(strength, -1.0, 1.0).astype(np.longdouble)[:, np.newaxis, np.newaxis]
    if upper is None:
        limit = n
    else:
        limit = np.minimum(upper * one - n, n)
    shift = strength * limit
    return np.where(above[np.newaxis, :, np.newaxis], n + shift, n - shift)


def reference_occupation(table, theta, n_gauss=10, modulate=False, strengths=None, chunk=256):
    """Mean occupations (n_draws, n_bins) in np.longdouble, and the UNMODULATED, undecorated
    satellite value per bin (zero in the centrals' columns): what the modulated tolerance is
    relative to; and KAPPA (see above) of the satellite pairs."""
    gal_type = table['gal_type']
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    ld = np.longdouble
    mass64, w = node_masses(gal_type, n_gauss)
    mass = mass64.astype(ld)
    log_mass = np.log10(mass)
    central = is_centrals(gal_type)
    if 'prim_haloprop_dist_index' in gal_type.dtype.names:
        power = gal_type['prim_haloprop_dist_index'].astype(ld)[:, np.newaxis] + 1
    else:
        power = np.zeros((len(gal_type), 1), dtype=ld)
    weight = w.astype(ld) * (mass / mass[:, :1])**power
    weight = weight / np.sum(weight, axis=-1, keepdims=True)
    above = gal_type['sec_haloprop_percentile'] > 0.5
    out = np.zeros((len(theta), len(gal_type)), dtype=ld)
    plain = np.zeros((len(theta), len(gal_type)), dtype=ld)
    kappa = np.zeros((len(theta), len(gal_type)))
    for begin in range(0, len(theta), chunk):
        t = theta[begin:begin + chunk].astype(ld)
        sel = slice(begin, begin + chunk)
        z = (log_mass[np.newaxis] - t[:, 0, np.newaxis, np.newaxis]) / t[:, 1, np.newaxis,
                                                                         np.newaxis]
        n_cen = (1 + _erf(z)) / 2
        m0 = np.power(ld(10), t[:, 2])[:, np.newaxis, np.newaxis]
        m1 = np.power(ld(10), t[:, 3])[:, np.newaxis, np.newaxis]
        x = mass[np.newaxis] - m0
        positive = x > 0
        with np.errstate(all='ignore'):
            n_sat = np.where(positive, np.power(np.where(positive, x, 1) / m1,
                                                t[:, 4, np.newaxis, np.newaxis]), 0)
        plain[sel] = np.where(central, 0, np.sum(weight * n_sat, axis=-1))
        with np.errstate(all='ignore'):
            slope = np.sum(weight * np.where(positive, n_sat / np.where(positive, x, 1), 0),
                           axis=-1)
            kappa[sel] = np.where(central | (plain[sel] == 0), 0,
                                  np.abs(t[:, 4, np.newaxis]) * m0[:, :, 0] * slope / plain[sel])
        if modulate:
            n_sat = n_sat * n_cen
        if strengths is not None:
            s = np.asarray(strengths, dtype=np.float64)[begin:begin + chunk]
            n_cen = _decorate(n_cen, s[:, 0], above, 1)
            n_sat = _decorate(n_sat, s[:, 1], above, None)
        node = np.where(central[np.newaxis, :, np.newaxis], n_cen, n_sat)
        out[sel] = np.sum(weight * node, axis=-1)
    return out, plain, kappa


def mpmath_occupation(table, theta, bin_index, n_gauss=10, modulate=False, strengths=None,
                      digits=40):
    """One (bin, draw) pair with mpmath at `digits` digits (same inputs as the reference)."""
    import mpmath
    gal_type = table['gal_type']
    with mpmath.workdps(digits):
        mp = mpmath.mpf
        mass64, w = node_masses(gal_type, n_gauss)
        row = gal_type[bin_index]
        central = bool(is_centrals(gal_type)[bin_index])
        power = mp(float(row['prim_haloprop_dist_index'])) + 1
        above = float(row['sec_haloprop_percentile']) > 0.5
        t = [mp(float(v)) for v in theta]
        total, norm = mp(0), mp(0)
        for k in range(n_gauss):
            m = mp(float(mass64[bin_index, k]))
            n_cen = (1 + mpmath.erf((mpmath.log10(m) - t[0]) / t[1])) / 2
            x = m - mp(10)**t[2]
            n_sat = (x / mp(10)**t[3])**t[4] if x > 0 else mp(0)
            if modulate:
                n_sat = n_sat * n_cen
            if strengths is not None:
                s_cen, s_sat = [mp(float(np.clip(v, -1, 1))) for v in strengths]
                shift = s_cen * min(1 - n_cen, n_cen)
                n_cen = n_cen + shift if above else n_cen - shift
                n_sat = n_sat * (1 + s_sat) if above else n_sat * (1 - s_sat)
            wk = mp(float(w[k])) * (m / mp(float(mass64[bin_index, 0])))**power
            total += wk * (n_cen if central else n_sat)
            norm += wk
        return total / norm


# ---- per-bin readout --------------------------------------------------------------------------

def selector_tables(table, n_r=None):
    """ceil(n_bins / n_r) tables with the same gal_type and a 0 / 1 tpcf_matrix: row r of table
    k selects bin k n_r + r -- mode cross T[r, b] = 1, so xi_r ngal = N_b n_h_b; mode auto
    T[r, p(b, b)] = 1, so sqrt(xi_r) ngal = N_b n_h_b.  The zeros are exact: whatever kernel
    predicts from such a table returns its own in-kernel occupations to a few ulp."""
    mode = table['attrs']['mode']
    n_r = N_R[mode] if n_r is None else n_r
    n_bins = len(table['gal_type'])
    n_columns = n_bins * (n_bins + 1) // 2 if mode == 'auto' else n_bins
    out = []
    for first in range(0, n_bins, n_r):
        matrix = np.zeros((n_r, n_columns))
        for r, b in enumerate(range(first, min(first + n_r, n_bins))):
            matrix[r, b * (b + 1) // 2 + b if mode == 'auto' else b] = 1.0
        out.append({'gal_type': table['gal_type'], 'tpcf_matrix': matrix, 'tpcf_shape': (n_r, ),
                    'attrs': dict(table['attrs'])})
    return out


def readout(table, results, n_r=None):
    """Occupations (n_draws, n_bins) in longdouble from the (ngal, xi) of `selector_tables`'
    tables, in their order."""
    mode = table['attrs']['mode']
    n_r = N_R[mode] if n_r is None else n_r
    n_h = table['gal_type']['n_h'].astype(np.longdouble)
    n_bins = len(n_h)
    columns = []
    for ngal, xi in results:
        ngal = np.asarray(ngal, dtype=np.float64).astype(np.longdouble)[:, np.newaxis]
        xi = np.asarray(xi, dtype=np.float64).reshape(len(ngal), n_r).astype(np.longdouble)
        columns.append((np.sqrt(xi) if mode == 'auto' else xi) * ngal)
    return np.concatenate(columns, axis=1)[:, :n_bins] / n_h


# ---- the host hooks ---------------------------------------------------------------------------

def _hook(name, n_gauss, row, *columns):
    from tabcorr_amd import _lib
    lib = _lib.load()
    columns = [np.ascontiguousarray(c, dtype=np.float64) for c in columns]
    n = len(columns[0])
    series, nodes = np.empty(n), np.empty(n)
    terms = np.zeros(n, dtype=np.int32)
    _lib.check(getattr(lib, name)(
        n_gauss, float(row['log_prim_haloprop_min']), float(row['log_prim_haloprop_max']),
        float(row['prim_haloprop_dist_index']), n, *[_lib.as_double_p(c) for c in columns],
        _lib.as_double_p(series), _lib.as_double_p(nodes),
        terms.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return series, nodes, terms


def central_hook(row, theta, n_gauss=10):
    """(N_cen by the expansion -- the node loop where none applies --, by the node loop, terms)
    of one central bin for the draws theta."""
    series, nodes, terms = _hook('tc_debug_central_series', n_gauss, row, theta[:, 0], theta[:, 1])
    return 0.5 + 0.5 * series, 0.5 + 0.5 * nodes, terms


def satellite_hook(row, theta, n_gauss=10):
    return _hook('tc_debug_satellite_series', n_gauss, row, theta[:, 2], theta[:, 3], theta[:, 4])


def label_pairs(table, theta, n_gauss=10, kappa=None):
    """Stratum of every (draw, bin) pair, from the host hooks and the branches the kernels
    take next to the expansions (kernels.hip.h: occ_bin_zheng07).

    Returns a dict: 'stratum' (n_draws, n_bins) int; 'terms' the hooks' term counts; 'series' and
    'nodes' the hooks' values (centrals N_cen, satellites the unmodulated N_sat); 'top' pairs
    whose term count changes when 1 / sigma resp. M0 grows by 2 per cent (the top of the
    stratum, where a missing pass costs most); 'shortest' per bin the term count of the bin's
    shortest satellite expansion (0: none; centrals 0).  kappa (n_draws, n_bins): the condition
    numbers `reference_occupation` returns -- satellite pairs beyond KAPPA_MAX become SAT_ILL."""
    gal_type = table['gal_type']
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    central = is_centrals(gal_type)
    n, n_bins = len(theta), len(gal_type)
    out = {key: np.zeros((n, n_bins), dtype=dtype) for key, dtype in (
        ('stratum', np.int32), ('terms', np.int32), ('series', np.float64),
        ('nodes', np.float64), ('top', bool))}
    out['shortest'] = np.zeros(n_bins, dtype=np.int32)
    mass, _ = node_masses(gal_type, n_gauss)
    log_mass = np.log10(mass)
    grown = theta.copy()
    grown[:, 1] /= 1.02
    grown[:, 2] += np.log10(1.02)
    far = theta[:1].copy()
    far[0, 2], far[0, 4] = 3.0, 1.0
    with np.errstate(all='ignore'):
        for b in range(n_bins):
            row = gal_type[b]
            if central[b]:
                series, nodes, terms = central_hook(row, theta, n_gauss)
                terms_grown = central_hook(row, grown, n_gauss)[2]
                inv_sigma = 1.0 / theta[:, 1]
                z_a = (log_mass[b, 0] - theta[:, 0]) * inv_sigma
                z_b = (log_mass[b, -1] - theta[:, 0]) * inv_sigma
                stratum = terms.copy()
                stratum[theta[:, 1] < 0] = CEN_NEGATIVE
                stratum[np.minimum(z_a, z_b) >= 6.0] = CEN_PLATEAU_1
                stratum[np.maximum(z_a, z_b) <= -6.0] = CEN_PLATEAU_0
            else:
                series, nodes, terms = satellite_hook(row, theta, n_gauss)
                terms_grown = satellite_hook(row, grown, n_gauss)[2]
                out['shortest'][b] = satellite_hook(row, far, n_gauss)[2][0]
                m0 = 10.0**theta[:, 2]
                stratum = terms.copy()
                stratum[np.any(mass[b] <= m0[:, np.newaxis], axis=-1)] = SAT_INSIDE
                stratum[theta[:, 4] == 0.0] = SAT_ALPHA_0
                stratum[theta[:, 4] == 4.0] = SAT_ALPHA_4
                stratum[(theta[:, 4] < 0.0) | (theta[:, 4] > 4.0)] = SAT_ALPHA_OUT
                stratum[np.all(mass[b] <= m0[:, np.newaxis], axis=-1)] = SAT_BELOW
                if kappa is not None:
                    stratum[(kappa[:, b] > KAPPA_MAX) & (stratum != SAT_BELOW)] = SAT_ILL
            out['stratum'][:, b] = stratum
            out['terms'][:, b] = terms
            out['series'][:, b] = series
            out['nodes'][:, b] = nodes
            out['top'][:, b] = (terms > 0) & (terms_grown != terms)
    return out


# ---- limits of the strata, by bisection on the hooks ------------------------------------------

def central_limits(row, n_gauss=10):
    """{terms: the smallest sigma at which the bin's expansion of that many terms serves a
    draw} (the stratum's upper limit in 1 / sigma)."""
    limits = {}
    theta = np.zeros((1, 5))
    theta[0, 0] = 12.0

    def terms(sigma):
        theta[0, 1] = sigma
        return central_hook(row, theta, n_gauss)[2][0]
    for count in CEN_TERMS:
        lo, hi = 1e-5, 1e4            # terms(lo) > count or 0; terms(hi) <= count
        if not 0 < terms(hi) <= count:
            continue
        for _ in range(70):
            mid = np.sqrt(lo * hi)
            if 0 < terms(mid) <= count:
                hi = mid
            else:
                lo = mid
        limits[count] = hi
    return limits


def satellite_limits(row, n_gauss=10):
    """{terms: (log10 of the largest M0 that many terms serve, log10 of the next double's side)}
    for the term counts the bin has."""
    theta = np.zeros((1, 5))
    theta[0, 3], theta[0, 4] = 13.0, 1.0

    def terms(log_m0):
        theta[0, 2] = log_m0
        return satellite_hook(row, theta, n_gauss)[2][0]
    limits = {}
    low = 3.0
    if terms(low) == 0:
        return limits
    for count in SAT_TERMS:
        if count < terms(low):
            continue
        lo, hi = low, float(row['log_prim_haloprop_max'])      # served at lo, not at hi
        if not 0 < terms(lo) <= count:
            continue
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if 0 < terms(mid) <= count:
                lo = mid
            else:
                hi = mid
        limits[count] = (lo, hi)
    # (counts that share their limit with a shorter one do not exist for this bin)
    seen, out = set(), {}
    for count in sorted(limits):
        key = round(limits[count][0], 9)
        if key not in seen:
            out[count] = limits[count]
            seen.add(key)
    return out


# ---- the draws --------------------------------------------------------------------------------

def snap_m0(gal_type, log_m0, deepest=4):
    """Move every M0 that lies between two nodes (of the ten-node rule) of the satellite bins to
    the midpoint of its neighbours; inside a bin at most `deepest` nodes deep (see the module
    docstring: conditioning)."""
    central = is_centrals(gal_type)
    mass, _ = node_masses(gal_type[~central], 10)
    mass = np.unique(mass, axis=0)               # (bins that share their nodes)
    mass = mass[np.argsort(mass[:, 0])]
    flat = mass.ravel()
    assert np.all(np.diff(flat) > 0)
    m0 = 10.0**np.asarray(log_m0, dtype=np.float64)
    out = np.array(log_m0, dtype=np.float64)
    index = np.searchsorted(flat, m0)            # flat[index - 1] < m0 <= flat[index]
    inside = (index > 0) & (index < len(flat))
    k = index[inside] - 1                        # the node below
    local = k % 10
    k = np.where(local > deepest, k - (local - deepest), k)
    out[inside] = np.log10(0.5 * (flat[k] + flat[k + 1]))
    return out


def stratified_draws(table, n_draws=1536, seed=0, limits=None):
    """(theta (n, 5), strengths (n, 2), order_uniform, order_shuffled): finite draws that fill
    every stratum a table has, `order_uniform` with whole 64-draw tiles of one kind (the
    wave-uniform shortcuts fire: plateaus, bins below every M0), `order_shuffled` with every
    kind in every wave."""
    from tabcorr_amd import synthetic
    gal_type = table['gal_type']
    central = is_centrals(gal_type)
    rng = np.random.default_rng(seed)
    lo_edge = float(np.min(gal_type['log_prim_haloprop_min']))
    hi_edge = float(np.max(gal_type['log_prim_haloprop_max']))
    span = hi_edge - lo_edge

    def random_draws(n):
        theta = synthetic.zheng07_draws(n, seed=int(rng.integers(1 << 30)))
        # (logMmin and logM0 follow the table's range: the narrow table sits inside the prior box)
        theta[:, 0] = rng.uniform(lo_edge + 0.1 * span, hi_edge - 0.3 * span, n)
        theta[:, 2] = rng.uniform(lo_edge - 0.3 * span, lo_edge + 0.6 * span, n)
        return theta
    blocks, kinds = [], []

    def add(theta, kind):
        blocks.append(theta)
        kinds.extend([kind] * len(theta))

    # whole tiles on the plateaus and below M0: an ensemble clustered around one point, narrow
    # enough that the same bins are on a plateau / below M0 for every draw
    theta = random_draws(192)
    theta[:, 0] = lo_edge + 0.5 * span + rng.uniform(-0.01, 0.01, 192) * min(span, 1.0)
    theta[:, 1] = rng.uniform(SIGMA_MIN, min(0.05, span / 40 + SIGMA_MIN), 192)
    theta[:, 2] = lo_edge + 0.45 * span + rng.uniform(-0.01, 0.01, 192) * min(span, 1.0)
    add(theta, 'cluster')
    theta = random_draws(64)
    theta[:, 0] = rng.uniform(4.0, 5.0, 64)                       # every bin at 1 ...
    theta[:, 1] = rng.uniform(0.1, 0.7, 64)
    theta[:, 2] = rng.uniform(hi_edge + 0.5, hi_edge + 1.5, 64)   # ... and below M0
    add(theta, 'ones')
    # the limits of the centrals' strata
    cen_limits = central_limits(gal_type[central][0]) if limits is None else limits[0]
    for count, sigma in sorted(cen_limits.items()):
        if not SIGMA_MIN / 0.98 <= sigma <= 50.0:
            continue
        for side, (a, b) in (('top', (1.0, 1.02)), ('next', (0.98, 1.0 - 1e-9))):
            theta = random_draws(16)
            theta[:, 1] = sigma * rng.uniform(a, b, 16)
            theta[0, 1] = sigma * (a if side == 'top' else b)
            add(theta, 'cen %d %s' % (count, side))
    theta = random_draws(64)
    theta[:, 1] = -theta[:, 1]
    add(theta, 'negative sigma')
    if cen_limits.get(24, 0.0) > SIGMA_MIN * 1.1:
        theta = random_draws(48)
        theta[:, 1] = rng.uniform(SIGMA_MIN, cen_limits[24] * 0.97, 48)
        add(theta, 'cen nodes')
    # alpha
    for kind, values in (('alpha 0', np.zeros(48)), ('alpha 4', np.full(48, 4.0)),
                         ('alpha above 4', rng.uniform(4.1, 5.5, 48))):
        theta = random_draws(48)
        theta[:, 4] = values
        add(theta, kind)
    theta = random_draws(48)
    theta[:, 4] = rng.uniform(-1.0, -0.05, 48)
    theta[:, 2] = rng.uniform(lo_edge - 1.5, lo_edge - 0.5, 48)   # (conditioning: see above)
    add(theta, 'alpha below 0')
    # the limits of the satellites' strata, bin by bin
    sat_rows = gal_type[~central]
    _, first = np.unique(sat_rows['log_prim_haloprop_min'], return_index=True)
    sat_limits = ({int(b): satellite_limits(sat_rows[b]) for b in first} if limits is None
                  else limits[1])
    placed = [(count, b) for b in sorted(sat_limits) for count in sat_limits[b]]
    budget = max(0, n_draws - sum(len(b) for b in blocks) - 160)
    per = 2
    if placed:
        keep = placed if 2 * per * len(placed) <= budget else [
            placed[i] for i in np.linspace(0, len(placed) - 1, budget // (2 * per)).astype(int)]
        for count, b in keep:
            lo, hi = sat_limits[b][count]
            theta = random_draws(2 * per)
            theta[:per, 2] = lo + np.log10(1.0 - 0.02 * rng.uniform(0, 1, per))
            theta[0, 2] = lo
            theta[per:, 2] = hi + np.log10(1.0 + 0.02 * rng.uniform(0, 1, per))
            theta[per, 2] = hi
            # (alpha as large as the conditioning allows: KAPPA ~ alpha M0 / (Mc - M0))
            centre = 0.5 * (sat_rows[b]['log_prim_haloprop_min'] +
                            sat_rows[b]['log_prim_haloprop_max'])
            unit = 1.0 / (10.0**(centre - hi) - 1.0)
            theta[:, 4] = rng.uniform(0.3, min(3.9, 0.8 * KAPPA_MAX / unit), 2 * per)
            add(theta[:per], 'sat %d top' % count)
            add(theta[per:], 'sat %d next' % count)
    add(random_draws(n_draws - sum(len(b) for b in blocks)), 'random')
    theta = np.concatenate(blocks)
    assert len(theta) == n_draws, len(theta)
    # the placed M0 keep their place (they lie below their bin); the others leave the nodes alone
    placed_m0 = np.array([kind.startswith('sat ') for kind in kinds])
    snapped = snap_m0(gal_type, theta[:, 2])
    theta[:, 2] = np.where(placed_m0, theta[:, 2], snapped)
    strengths = rng.uniform(-0.95, 0.95, (n_draws, 2))
    assert np.all(np.isfinite(theta)) and np.all(np.abs(theta[:, 1]) >= SIGMA_MIN)
    # (the clustered ensemble and the draws at 1 first, each a whole number of 64-draw tiles;
    # then kind by kind)
    rank = np.array([0 if k == 'cluster' else 1 if k == 'ones' else 2 for k in kinds])
    order_uniform = np.lexsort((np.arange(n_draws), np.array(kinds), rank))
    order_shuffled = rng.permutation(n_draws)
    return theta, strengths, order_uniform, order_shuffled, (cen_limits, sat_limits), kinds


# ---- errors per stratum -----------------------------------------------------------------------

def pair_errors(values, reference, central, scale=None):
    """|value - reference| for the centrals' columns (absolute: the occupation lies in [0, 1]),
    |value - reference| / scale for the satellites' (scale: the reference itself, or the
    unmodulated value where the satellites are modulated); 0 where both are exactly 0, inf where
    only one is."""
    values = np.asarray(values).astype(np.longdouble)
    scale = reference if scale is None else scale
    difference = np.abs(values - reference)
    with np.errstate(all='ignore'):
        relative = np.where(difference == 0, 0, difference / np.abs(scale))
    return np.where(central[np.newaxis], difference, relative).astype(np.float64)


def stratum_maxima(errors, stratum, central, select=None):
    """{('cen' | 'sat', stratum): (count, largest error)} over the pairs of `select`."""
    out = {}
    for name, columns in (('cen', central), ('sat', ~central)):
        e, s = errors[:, columns], stratum[:, columns]
        keep = np.ones(e.shape, dtype=bool) if select is None else select[:, columns]
        for value in np.unique(s[keep]):
            chosen = keep & (s == value)
            out[name, int(value)] = (int(np.sum(chosen)), float(np.max(e[chosen])))
    return out


def expected_strata(table, limits):
    """The strata `stratified_draws` fills for this table: {'cen': set, 'sat': set}."""
    gal_type = table['gal_type']
    span = float(np.max(gal_type['log_prim_haloprop_max']) -
                 np.min(gal_type['log_prim_haloprop_min']))
    cen_limits, sat_limits = limits
    cen = {count for count, sigma in cen_limits.items() if SIGMA_MIN / 0.98 <= sigma <= 50.0}
    cen |= {CEN_PLATEAU_1, CEN_NEGATIVE}
    if cen_limits.get(24, 0.0) > SIGMA_MIN * 1.1:
        cen.add(CEN_NODES)
    sat = {count for counts in sat_limits.values() for count in counts}
    sat |= {SAT_BELOW, SAT_ALPHA_OUT, SAT_ALPHA_0, SAT_ALPHA_4}
    if span >= 1.0:
        # (a table wider than the clustered ensemble's 6 sigma and the bins' own width)
        cen.add(CEN_PLATEAU_0)
        sat |= {SAT_NODES, SAT_INSIDE}
    return {'cen': cen, 'sat': sat}


# ---- one table's draws, labels and references, made once --------------------------------------

_PREPARED = {}


def prepared(name):
    """Draws, labels and limits of table `name` (mode auto; the gal_type and hence the
    occupations are the same in mode cross), cached for the process."""
    if name not in _PREPARED:
        table = make_table(name)
        theta, strengths, uniform, shuffled, limits, kinds = stratified_draws(table)
        _PREPARED[name] = {'table': table, 'theta': theta, 'strengths': strengths,
                           'orders': {'uniform': uniform, 'shuffled': shuffled},
                           'limits': limits, 'kinds': kinds, 'reference': {}, 'labels': {},
                           'central': is_centrals(table['gal_type'])}
    return _PREPARED[name]


def prepared_reference(name, n_gauss=10, modulate=False, decorated=False):
    """(occupations, scale of the satellites' relative error, labels) of `prepared(name)`."""
    p = prepared(name)
    key = (n_gauss, modulate, decorated)
    if key not in p['reference']:
        occupation, plain, kappa = reference_occupation(
            p['table'], p['theta'], n_gauss, modulate, p['strengths'] if decorated else None)
        scale = occupation
        if modulate:
            scale = plain
            if decorated:
                above = p['table']['gal_type']['sec_haloprop_percentile'] > 0.5
                s_sat = p['strengths'][:, 1:2].astype(np.longdouble)
                scale = plain * np.where(above[np.newaxis], 1 + s_sat, 1 - s_sat)
        if n_gauss not in p['labels']:
            p['labels'][n_gauss] = label_pairs(p['table'], p['theta'], n_gauss, kappa)
        p['reference'][key] = (occupation, scale)
    return p['reference'][key] + (p['labels'][n_gauss], )


def check_cells(name, values, rows, n_gauss=10, modulate=False, decorated=False, what=''):
    """Per (type, stratum) cell the count and largest error of the occupations `values` of the
    draws `rows` (indices into the prepared draws) against the reference, and the cells beyond
    their allowance: ({cell: (count, error, allowance)}, [failing cells])."""
    p = prepared(name)
    occupation, scale, labels = prepared_reference(name, n_gauss, modulate, decorated)
    errors = pair_errors(values, occupation[rows], p['central'], scale[rows])
    cells, failed = {}, []
    for cell, (count, worst) in stratum_maxima(errors, labels['stratum'][rows],
                                                p['central']).items():
        if cell == ('sat', SAT_ILL):
            continue
        limit = allowance(cell[0], cell[1], modulate, decorated)
        cells[cell] = (count, worst, limit)
        if not worst <= limit:
            failed.append((what, name) + cell + (count, worst, limit))
    return cells, failed


def pick_draws(name, n=32, enough=8):
    """`n` of the prepared draws that together hold at least `enough` pairs of every stratum of
    the table (the un-batched kernel takes one draw per call): each time the draw with the most
    pairs of the stratum that is furthest from `enough`."""
    p = prepared(name)
    stratum = prepared_reference(name)[2]['stratum']
    expected = expected_strata(p['table'], p['limits'])
    cells = [(p['central'], s) for s in sorted(expected['cen'])]
    cells += [(~p['central'], s) for s in sorted(expected['sat'])]
    per_draw = np.array([np.sum(stratum[:, columns] == value, axis=1) for columns, value in cells])
    chosen, have = [], np.zeros(len(cells), dtype=np.int64)
    for _ in range(n):
        counts = per_draw[int(np.argmin(np.minimum(have, 10 * enough)))].copy()
        counts[chosen] = -1
        chosen.append(int(np.argmax(counts)))
        have = have + per_draw[:, chosen[-1]]
    return np.array(chosen)
