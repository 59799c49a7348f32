"""The occupation VJP on the device (TabCorr.predict_vjp / chi2_grad_occupation, the
tc_predict_occupation_vjp_* and tc_chi2_occupation_grad_* entry points) against the NumPy
reference of vjp_reference.py and the oracle's values.  Needs an MI355X.

Allowance of a gradient element: |got - ref| <= 1e-10 (|ref| + scale) -- the project's parity bar
applied to the value and to the terms that cancel in it (vjp_reference: scale); ngal and xi to
1e-10 relative.  Every case prints its largest error in units of that allowance.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference  # noqa: E402
import vjp_reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    D, LDS_LIMIT, RTOL, check_refused, check_still_serves, chi2_data, device_call, largest,
    same_bits)
from util import assert_rel, load_golden, table_from_golden  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DRAW_COUNTS = [1, D + 1, 2 * D + 3]
N_MAX = max(DRAW_COUNTS)
KINDS = ['zheng07', 'decorated', 'random']

_tables = {}
_occupations = {}
_references = {}


def make_table(n_prim, n_sec, tpcf_shape, mode, **kwargs):
    from tabcorr_amd import TabCorr
    table = synthetic.synthetic_table(n_prim, n_sec, tpcf_shape, mode, seed=3)
    return table, TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                      table['tpcf_shape'], table['attrs'], **kwargs)


def get_table(case):
    """(table dict, TabCorr) of a case (n_prim, n_sec, tpcf_shape, mode), made once."""
    if case not in _tables:
        _tables[case] = make_table(*case)
    return _tables[case]


def decorated_draws(n_draws, seed):
    """(n_draws, 7): Zheng07 draws with assembly-bias strengths 0.1 <= |A| <= 0.9."""
    rng = np.random.default_rng(seed + 100)
    strength = rng.uniform(0.1, 0.9, size=(n_draws, 2)) * rng.choice([-1.0, 1.0], (n_draws, 2))
    return np.hstack([synthetic.zheng07_draws(n_draws, seed=seed), strength])


def occupations_of(table, kind, n_draws=N_MAX):
    """(n_draws, n_bins) occupations, every draw with galaxies: from the oracle for plain or
    decorated Zheng07 draws (the first seed from 5 on that leaves no draw empty), or random
    positive numbers of which about a quarter, never all, are exactly zero."""
    n_bins = len(table['gal_type'])
    if kind == 'random':
        rng = np.random.default_rng(n_bins)
        occupation = rng.uniform(0.1, 2.0, size=(n_draws, n_bins))
        zero = rng.uniform(size=occupation.shape) < 0.25
        zero[np.arange(n_draws), rng.integers(n_bins, size=n_draws)] = False
        occupation[zero] = 0.0
        return occupation
    for seed in range(5, 25):
        theta = decorated_draws(n_draws, seed)
        occupation = np.array([oracle.mean_occupation(table, oracle.Zheng07(
            t[:5], assembias=t[5:] if kind == 'decorated' else None)) for t in theta])
        if np.all(occupation @ table['gal_type']['n_h'] > 0.0):
            return occupation
    raise AssertionError('no seed gives draws with galaxies')


def get_occupations(case, kind):
    key = (case, kind)
    if key not in _occupations:
        _occupations[key] = occupations_of(get_table(case)[0], kind)
        _occupations[key].setflags(write=False)
    return _occupations[key]


def cotangents(case, which, n_draws=N_MAX):
    """g_xi (n_draws, ) + tpcf_shape and g_ngal (n_draws, ) or None.  'random'; 'no_ngal'; 'unit_R':
    the unit vector of r bin R alone; 'ngal': g_xi = 0 and g_ngal = 1."""
    tpcf_shape = case[2]
    n_r = int(np.prod(tpcf_shape))
    rng = np.random.default_rng(17)
    g_xi = rng.normal(size=(n_draws, n_r))
    g_ngal = rng.normal(size=n_draws)
    if which == 'no_ngal':
        g_ngal = None
    elif which == 'ngal':
        g_xi, g_ngal = np.zeros((n_draws, n_r)), np.ones(n_draws)
    elif which.startswith('unit_'):
        g_xi, g_ngal = np.zeros((n_draws, n_r)), None
        g_xi[:, int(which[5:])] = 1.0
    return g_xi.reshape((n_draws, ) + tpcf_shape), g_ngal


def get_reference(case, kind, which):
    """Occupations, cotangents and the reference (ngal, xi, g_occupation, scale) of N_MAX draws,
    computed once per combination and never modified: a batch of n draws is the first n."""
    key = (case, kind, which)
    if key not in _references:
        table, _ = get_table(case)
        occupation = get_occupations(case, kind)
        g_xi, g_ngal = cotangents(case, which)
        reference = vjp_reference.vjp_batch(table, occupation, g_xi, g_ngal)
        assert np.all(reference[0] > 0.0) and all(np.all(np.isfinite(a)) for a in reference)
        for array in (g_xi, g_ngal) + reference:
            if array is not None:
                array.setflags(write=False)
        _references[key] = (occupation, g_xi, g_ngal, reference)
    return _references[key]


def check_gradient(got, ref, scale, what):
    allowance = RTOL * (np.abs(ref) + scale)
    error = np.abs(got - ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(error == 0.0, 0.0, error / allowance)
    print('%s: max |g - reference| / allowance = %.3g' % (what, np.max(ratio)))
    assert got.shape == ref.shape
    assert np.all(error <= allowance), (what, np.max(ratio))


def check_call(halotab, occupation, g_xi, g_ngal, reference, n, what):
    ngal, xi, g_occupation = halotab.predict_vjp(
        occupation[:n], g_xi[:n], None if g_ngal is None else g_ngal[:n])
    assert ngal.shape == (n, ) and xi.shape == g_xi[:n].shape
    assert_rel(ngal, reference[0][:n], RTOL, what + ' ngal')
    assert_rel(xi, reference[1][:n], RTOL, what + ' xi')
    check_gradient(g_occupation, reference[2][:n], reference[3][:n], what)
    return g_occupation


# Mode auto: 2, 4, 14, 16, 18, 36, 66 and 100 bins -- one step of four matrix columns, whole tiles
# of 16 rows, one bin past a tile, groups of percentile bins (whose library order differs from the
# rows of gal_type), more tiles than waves.  Mode cross: 36 and 66 bins (one slab of 64, one slab
# and two bins) and 132 (more than two slabs).  Every tpcf_shape appears in both modes.
AUTO_CASES = [(1, 1, (1, ), 'auto'), (2, 1, (5, ), 'auto'), (7, 1, (3, 4), 'auto'),
              (8, 1, (19, ), 'auto'), (9, 1, (1, ), 'auto'), (9, 2, (5, ), 'auto'),
              (33, 1, (3, 4), 'auto'), (50, 1, (19, ), 'auto')]
CROSS_CASES = [(9, 2, (1, ), 'cross'), (18, 1, (5, ), 'cross'), (33, 1, (3, 4), 'cross'),
               (33, 2, (19, ), 'cross')]
CASES = AUTO_CASES + CROSS_CASES


def case_id(case):
    return '%s-%dx%d-%s' % (case[3], case[0], case[1], 'x'.join(map(str, case[2])))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_vjp_matches_reference(case, kind):
    """Random cotangents with and without g_ngal at 1, 17 and 35 draws; at 17 draws the unit
    vectors of the first and the last r bin (single rows of the Jacobian) and g_ngal = 1 alone
    (the bare n_h)."""
    table, halotab = get_table(case)
    n_r = int(np.prod(case[2]))
    for which in ('random', 'no_ngal'):
        occupation, g_xi, g_ngal, reference = get_reference(case, kind, which)
        for n in DRAW_COUNTS:
            what = '%s %s %s n=%d' % (case_id(case), kind, which, n)
            check_call(halotab, occupation, g_xi, g_ngal, reference, n, what)
    for which in sorted({'unit_0', 'unit_%d' % (n_r - 1), 'ngal'}):
        occupation, g_xi, g_ngal, reference = get_reference(case, kind, which)
        what = '%s %s %s n=%d' % (case_id(case), kind, which, D + 1)
        got = check_call(halotab, occupation, g_xi, g_ngal, reference, D + 1, what)
        if which == 'ngal':
            assert_rel(got, np.broadcast_to(table['gal_type']['n_h'], got.shape), RTOL)
    # un-batched
    occupation, g_xi, g_ngal, reference = get_reference(case, kind, 'random')
    one = halotab.predict_vjp(occupation[2], g_xi[2], g_ngal[2])
    full = halotab.predict_vjp(occupation, g_xi, g_ngal)
    assert np.ndim(one[0]) == 0 and one[1].shape == case[2] and one[2].shape == occupation[2].shape
    assert one[0] == full[0][2] and np.array_equal(one[1], full[1][2])
    assert np.array_equal(one[2], full[2][2])
    # ngal and xi are the forward seam's, to parity
    forward = halotab.predict(np.array(occupation))
    assert_rel(full[0], forward[0], RTOL)
    assert_rel(full[1], forward[1], RTOL)


# ---- the likelihood form --------------------------------------------------------------------

def chi2_inputs(case, kind, symmetric):
    """Occupations, a data vector near draw 3's xi and a precision matrix."""
    table, _ = get_table(case)
    occupation = get_occupations(case, kind)
    data, precision = chi2_data(oracle.predict(table, occupation[3])[1], symmetric)
    return occupation, data, precision


def check_chi2(got, reference, data, precision, what):
    """chi2 to rtol + 1e-10 sum_r |v_r| |xi_r| with v = 2 P_sym e (the allowance of xi carried
    through chi2 = e^T P e, as tests/test_gpu_grad.py does); dchi2 / dn to the allowance of the
    module with the likelihood's scale."""
    ngal, chi2, dchi2 = got
    ngal_ref, chi2_ref, dchi2_ref, scale, xi = reference
    n = len(ngal)
    flat = xi.reshape(len(xi), -1)[:n]
    v = 2.0 * (flat - np.ravel(data)) @ (0.5 * (precision + precision.T))
    chi2_allow = RTOL * np.abs(chi2_ref[:n]) + RTOL * np.sum(np.abs(v) * np.abs(flat), axis=1)
    assert_rel(ngal, ngal_ref[:n], RTOL, what + ' ngal')
    print('%s: max |chi2 - reference| / allowance = %.3g' % (
        what, np.max(np.abs(chi2 - chi2_ref[:n]) / chi2_allow)))
    assert np.all(np.abs(chi2 - chi2_ref[:n]) <= chi2_allow)
    check_gradient(dchi2, dchi2_ref[:n], scale[:n], what + ' dchi2')


CHI2_CASES = [(2, 1, (5, ), 'auto'), (9, 2, (5, ), 'auto'), (33, 1, (3, 4), 'auto'),
              (50, 1, (19, ), 'auto'), (9, 2, (1, ), 'cross'), (33, 2, (19, ), 'cross')]


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('case', CHI2_CASES, ids=case_id)
def test_chi2_gradient_matches_reference(case, symmetric):
    """chi2 and dchi2 / dn at 1, 17 and 35 draws, for the three kinds of occupations; the
    non-symmetric precision pins the P_sym convention.  The value agrees with the forward
    likelihood of the same occupations."""
    table, halotab = get_table(case)
    for kind in KINDS:
        occupation, data, precision = chi2_inputs(case, kind, symmetric)
        reference = vjp_reference.chi2_grad_batch(table, occupation, data, precision)
        for n in DRAW_COUNTS:
            got = halotab.chi2_grad_occupation(occupation[:n], data, precision)
            assert got[0].shape == got[1].shape == (n, ) and got[2].shape == (n, occupation.shape[1])
            check_chi2(got, reference, data, precision,
                       'chi2 %s %s n=%d %s' % (case_id(case), kind, n, symmetric))
    one = halotab.chi2_grad_occupation(occupation[2], data, precision)
    assert np.ndim(one[0]) == 0 and np.ndim(one[1]) == 0
    assert one[0] == got[0][2] and one[1] == got[1][2] and np.array_equal(one[2], got[2][2])


# ---- batch invariance, host and device entry points -------------------------------------------

def device_vjp(halotab, occupation, g_xi=None, g_ngal=None, data=None, precision=None, flags=0):
    """tc_predict_occupation_vjp_batch_device (with g_xi) or tc_chi2_occupation_grad_batch_device
    (with data and precision)."""
    from tabcorr_amd import _lib
    device = halotab.to_device()
    n, n_r = len(occupation), device.n_r
    if g_xi is None:
        data, precision = _lib.contiguous(np.ravel(data)), _lib.contiguous(precision)
        return device_call(device, 'tc_chi2_occupation_grad_batch_device',
                           [occupation, n, flags, _lib.as_double_p(data),
                            _lib.as_double_p(precision)], [n, n, occupation.shape])
    return device_call(device, 'tc_predict_occupation_vjp_batch_device',
                       [occupation, n, flags, g_ngal, g_xi], [n, (n, n_r), occupation.shape])


@pytest.mark.parametrize('case', [(50, 1, (19, ), 'auto'), (9, 2, (5, ), 'auto'),
                                  (33, 2, (19, ), 'cross')], ids=case_id)
def test_batch_invariance(case):
    """A draw's (ngal, xi, g_occupation) -- and (ngal, chi2, dchi2 / dn) -- are the same bits
    alone, in 17 draws (at two different columns of a workgroup) and in 35 draws, through the
    host and the device entry points.  Draw 5 has an all-zero occupation: its own results are NaN
    and none of its neighbours' are."""
    _, halotab = get_table(case)
    occupation = np.array(get_occupations(case, 'random'))
    occupation[5] = 0.0
    g_xi, g_ngal = cotangents(case, 'random')
    _, data, precision = chi2_inputs(case, 'random', False)
    others = np.arange(N_MAX) != 5

    def predict(rows, device=False):
        if device:
            return device_vjp(halotab, occupation[rows], g_xi.reshape(N_MAX, -1)[rows],
                               g_ngal[rows])
        return halotab.predict_vjp(occupation[rows], g_xi[rows], g_ngal[rows])

    def likelihood(rows, device=False):
        if device:
            return device_vjp(halotab, occupation[rows], data=data, precision=precision)
        return halotab.chi2_grad_occupation(occupation[rows], data, precision)

    for call in (predict, likelihood):
        full = call(slice(0, N_MAX))
        assert full[0][5] == 0.0 and np.all(np.isnan(full[1][5])) and np.all(np.isnan(full[2][5]))
        assert all(np.all(np.isfinite(a[others])) for a in full)
        for rows in (slice(0, 1), slice(0, D + 1), slice(3, D + 4), slice(D, D + 1),
                     slice(N_MAX - 1, N_MAX), slice(4, 5), slice(5, 6), slice(6, 7)):
            assert same_bits(call(rows), [a[rows] for a in full]), (call.__name__, rows)
        for n in DRAW_COUNTS:
            assert same_bits(call(slice(0, n), device=True), [a[:n] for a in full], reshape=True)
    # g_ngal = NULL through the device entry point
    assert same_bits(device_vjp(halotab, occupation, g_xi.reshape(N_MAX, -1)),
                     halotab.predict_vjp(occupation, g_xi), reshape=True)


# ---- the chain rule, end to end ---------------------------------------------------------------

@pytest.mark.parametrize('mode', ['auto', 'cross'])
def test_chain_rule_against_central_differences_of_the_oracle(mode):
    """What the feature is for: d chi2 / d theta_k of the seven-parameter decorated Zheng07 model
    as dchi2_docc @ dn/dtheta_k, against central differences of the oracle's chi2 with the bound
    of test_reference_vjp_matches_central_differences: |J - FD(h/2)| <= |FD(h) - FD(h/2)| +
    8 eps |chi2| / (h/2).  dn/dtheta_k is differenced in NumPy from the oracle's occupations with
    the five-point stencil of step h/2, whose own error (fourth order) is far below the bound's.
    logMmin and logM0 sit midway between their neighbouring nodes, more than 4 h from both (the
    decoration has a kink where <N_cen> crosses 1/2 at a node, <N_sat> where M0 crosses one)."""
    case = (9, 2, (5, ), mode)
    table, halotab = get_table(case)
    nodes = grad_reference.nodes_of(table)
    h = 1e-3
    rng = np.random.default_rng(11)
    precision = np.eye(5) * 5 + 0.3 * rng.normal(size=(5, 5))
    thetas = decorated_draws(6, seed=5)
    for column in (0, 2):
        for t in thetas:
            j = np.searchsorted(nodes, t[column])
            t[column] = 0.5 * (nodes[j - 1] + nodes[j])
            assert np.min(np.abs(nodes - t[column])) > 4 * h

    def occupation_of(theta):
        return oracle.mean_occupation(table, oracle.Zheng07(theta[:5], assembias=theta[5:]))

    data = oracle.predict(table, occupation_of(thetas[0]))[1].ravel() * (
        1.0 + 0.05 * rng.normal(size=5))

    def chi2_of(theta):
        e = oracle.predict(table, occupation_of(theta))[1].ravel() - data
        return e @ precision @ e

    def difference(theta, k, step):
        e = np.zeros(7)
        e[k] = step
        return (chi2_of(theta + e) - chi2_of(theta - e)) / (2 * step)

    ngal, chi2, dchi2_docc = halotab.chi2_grad_occupation(
        np.array([occupation_of(t) for t in thetas]), data, precision)
    worst = 0.0
    for d, theta in enumerate(thetas):
        assert_rel(chi2[d], chi2_of(theta), 1e-8)
        for k in range(7):
            e = np.zeros(7)
            e[k] = h / 2
            dn = (-occupation_of(theta + 2 * e) + 8 * occupation_of(theta + e) -
                  8 * occupation_of(theta - e) + occupation_of(theta - 2 * e)) / (12 * (h / 2))
            analytic = dchi2_docc[d] @ dn
            coarse, fine = difference(theta, k, h), difference(theta, k, h / 2)
            bound = abs(coarse - fine) + 8 * EPS * abs(chi2_of(theta)) / (h / 2)
            worst = max(worst, abs(analytic - fine) / bound)
            assert abs(analytic - fine) <= bound, (d, k, analytic, fine, coarse)
    print('chain rule %s: worst |J - FD(h/2)| / bound = %.3g' % (mode, worst))


# ---- what is refused --------------------------------------------------------------------------
# The documented budget of vjp_auto_kernel (csrc/vjp.h), in rows of D doubles: w of every bin and
# one row of zeros, sum_r g_r U_ri of every bin, per r bin four partial q_r, the cotangent and xi,
# and two rows for ngal and sum_r g_r xi_r.


def vjp_auto_lds_bytes(n_bins, n_r):
    return (2 * n_bins + 1 + 6 * n_r + 2) * D * 8


def check_served_case(case, what):
    occupation, g_xi, g_ngal, reference = get_reference(case, 'random', 'random')
    check_call(get_table(case)[1], occupation, g_xi, g_ngal, reference, D + 1, what)


@pytest.mark.parametrize('n_r', [1, 2])
def test_lds_limit_auto(n_r):
    """n_sec = 1: the table with the most bins that predict_vjp serves runs with (nearly) the
    whole LDS of a CU and matches the reference, in both forms; one more primary bin is refused
    by both, naming LDS, and the handle goes on serving predict_batch."""
    n_prim = largest(lambda n: vjp_auto_lds_bytes(2 * n, n_r) <= LDS_LIMIT)
    table, halotab = make_table(n_prim, 1, (n_r, ), 'auto')
    occupation = occupations_of(table, 'random', D + 1)
    g_xi, g_ngal = cotangents((n_prim, 1, (n_r, ), 'auto'), 'random', D + 1)
    reference = vjp_reference.vjp_batch(table, occupation, g_xi, g_ngal)
    what = 'LDS limit auto %d bins, %d r bins' % (2 * n_prim, n_r)
    check_call(halotab, occupation, g_xi, g_ngal, reference, D + 1, what)
    data, precision = 1.05 * reference[1][3], np.eye(n_r) + 0.1
    check_chi2(halotab.chi2_grad_occupation(occupation, data, precision),
               vjp_reference.chi2_grad_batch(table, occupation, data, precision), data, precision,
               what + ' chi2')
    table, halotab = make_table(n_prim + 1, 1, (n_r, ), 'auto')
    occupation = np.ones((3, 2 * n_prim + 2))
    check_refused(halotab, table, lambda _: halotab.predict_vjp(occupation, np.ones((3, n_r))))
    check_refused(halotab, table,
                  lambda _: halotab.chi2_grad_occupation(occupation, np.ones(n_r), np.eye(n_r)))
    check_served_case((9, 2, (5, ), 'auto'), 'after the LDS refusal')


def test_unsupported_requests_leave_the_handle_usable():
    from tabcorr_amd import _lib
    case = (9, 2, (5, ), 'auto')
    table, halotab = get_table(case)
    _, single = make_table(*case, compute_dtype='float32')
    occupation = np.array(get_occupations(case, 'random')[:5])
    # (1e-5: the float32 path's stated tolerance)
    check_refused(single, table, lambda _: single.predict_vjp(occupation, np.ones((5, 5))),
                  'float64', 1e-5)
    check_refused(single, table,
                  lambda _: single.chi2_grad_occupation(occupation, np.ones(5), np.eye(5)),
                  'float64', 1e-5)
    check_served_case(case, 'after the float32 refusal')

    device = halotab.to_device()
    outputs = [np.empty(5 * 2), np.empty(5 * 3 * 5), np.empty_like(occupation)]
    g_xi = np.ones((5, 5))
    for flags in (_lib.FLAG_SEPARATE_GAL_TYPE, _lib.FLAG_ASSEMBIAS):
        with device.lock:
            statuses = [device.lib.tc_predict_occupation_vjp_batch(
                device.handle, _lib.as_double_p(occupation), 5, flags, None,
                _lib.as_double_p(g_xi), *[_lib.as_double_p(a) for a in outputs]),
                device.lib.tc_chi2_occupation_grad_batch(
                    device.handle, _lib.as_double_p(occupation), 5, flags,
                    _lib.as_double_p(np.ones(5)), _lib.as_double_p(np.eye(5)),
                    *[_lib.as_double_p(a) for a in outputs])]
        for status in statuses:
            assert status == _lib.TC_ERR_UNSUPPORTED
            with pytest.raises(NotImplementedError):
                _lib.check(status)
        check_still_serves(halotab, table)
        check_served_case(case, 'after refused flags 0x%x' % flags)


# ---- real tables ------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['bolplanck_wp', 'bolplanck_ds'])
def test_real_table(name):
    from tabcorr_amd import TabCorr
    golden = load_golden(name)
    table = table_from_golden(golden)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                  table['tpcf_shape'], table['attrs'])
    n = D + 1
    theta = np.resize(np.array(golden['theta'], dtype=np.float64), (n, 5)).copy()
    theta[len(golden['theta']):] += 0.01 * np.arange(1, n - len(golden['theta']) + 1)[:, None]
    occupation = np.array([oracle.mean_occupation(table, oracle.Zheng07(t)) for t in theta])
    case = (0, 0, tuple(table['tpcf_shape']), table['attrs']['mode'])
    g_xi, g_ngal = cotangents(case, 'random', n)
    reference = vjp_reference.vjp_batch(table, occupation, g_xi, g_ngal)
    assert np.all(reference[0] > 0.0)
    check_call(halotab, occupation, g_xi, g_ngal, reference, n, name)
    n_r = int(np.prod(case[2]))
    rng = np.random.default_rng(11)
    data = reference[1][3] * (1.0 + 0.05 * rng.normal(size=reference[1][3].shape))
    scale = np.abs(np.ravel(data))
    precision = (np.diag(rng.uniform(1.0, 2.0, size=n_r)) +
                 0.01 * rng.normal(size=(n_r, n_r))) / np.outer(scale, scale)
    check_chi2(halotab.chi2_grad_occupation(occupation, data, precision),
               vjp_reference.chi2_grad_batch(table, occupation, data, precision), data, precision,
               name + ' chi2')
