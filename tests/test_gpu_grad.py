"""Analytic gradients on the device (TabCorr.predict_batch_grad / chi2_grad_batch /
predict_grad, the tc_*_grad_* entry points) against the reference Jacobian of grad_reference.py
and the oracle's values.  Needs an MI355X.

Tolerance of a derivative: rtol = 1e-10 (the project's parity bar) plus, per (draw, k), 1e-10 x
the size of the terms that cancel in it (grad_reference.jacobian: scale) -- the same bar applied
to those terms.  Every case prints its largest error in units of that allowance.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import (  # noqa: E402
    D, LDS_LIMIT, RTOL, check_refused, check_still_serves, chi2_data, device_call, largest,
    same_bits)
from util import assert_rel, load_golden, table_from_golden  # noqa: E402

pytestmark = pytest.mark.gpu

DRAW_COUNTS = [1, D - 1, D, D + 1, 2 * D + 3]
N_MAX = max(DRAW_COUNTS)

_tables = {}
_references = {}


def make_table(shape, mode, tpcf_shape=None):
    """(table dict, TabCorr) of a synthetic (n_prim, n_sec, n_r) table; `tpcf_shape`: the axes
    its n_r correlation function bins are reported in, (n_r, ) by default."""
    from tabcorr_amd import TabCorr
    tpcf_shape = (shape[2], ) if tpcf_shape is None else tuple(tpcf_shape)
    assert int(np.prod(tpcf_shape)) == shape[2]
    table = synthetic.synthetic_table(shape[0], shape[1], tpcf_shape, mode, seed=3)
    return table, TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                      table['tpcf_shape'], table['attrs'])


def get_table(shape, mode, tpcf_shape=None):
    """`make_table`, made once."""
    key = (shape, mode, tpcf_shape)
    if key not in _tables:
        _tables[key] = make_table(shape, mode, tpcf_shape)
    return _tables[key]


def get_reference(shape, mode, modulate, n_gauss, tpcf_shape=None, usable=False):
    """Draws and their reference (ngal, xi, dngal, dxi, scale), computed once per combination and
    never modified: a batch of n draws is the first n of them.  `usable`: the seed of the draws
    is the first one from 5 on with which every draw has galaxies and only finite reference
    results (a tiny table can leave a draw without any) -- chosen from the reference alone."""
    key = (shape, mode, modulate, n_gauss, tpcf_shape, usable)
    if key not in _references:
        table, _ = get_table(shape, mode, tpcf_shape)
        for seed in range(5, 25):
            theta = grad_reference.stress_draws(table, N_MAX, seed=seed, n_gauss_prim=n_gauss)
            with np.errstate(all='ignore'):
                reference = grad_reference.jacobian_batch(table, theta, n_gauss, modulate)
            if not usable or grad_reference.usable(reference):
                break
        else:
            raise AssertionError('no seed gives usable draws for %s' % (key, ))
        values = oracle.predict_zheng07_batch(table, theta, n_gauss_prim=n_gauss,
                                              modulate_with_cenocc=modulate)
        for array in (theta, ) + reference + values:
            array.setflags(write=False)
        _references[key] = (theta, reference, values)
    return _references[key]


def check_derivatives(got_dngal, got_dxi, reference, what):
    _, _, dngal, dxi, scale = reference
    assert_rel(got_dngal, dngal, RTOL, what + ' dngal')
    extra = (1, ) * (dxi.ndim - 2)
    allowance = RTOL * np.abs(dxi) + RTOL * scale.reshape(scale.shape + extra)
    error = np.abs(got_dxi - dxi)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(error == 0.0, 0.0, error / allowance)
    print('%s: max |dxi - reference| / allowance = %.3g' % (what, np.max(ratio)))
    assert np.all(error <= allowance), (what, np.max(ratio))


AUTO_SHAPES = [(7, 1, 5), (9, 2, 5), (50, 1, 19), (52, 2, 21)]
CROSS_SHAPES = [(9, 2, 5), (276, 2, 13)]
CASES = ([(shape, 'auto') for shape in AUTO_SHAPES] +
         [(shape, 'cross') for shape in CROSS_SHAPES])


@pytest.mark.parametrize('n_gauss', [10, 3])
@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', DRAW_COUNTS)
@pytest.mark.parametrize('shape,mode', CASES,
                         ids=['%s-%dx%dx%d' % ((m, ) + s) for s, m in CASES])
def test_gradient_matches_reference_jacobian(shape, mode, n_draws, modulate, n_gauss):
    _, halotab = get_table(shape, mode)
    theta, reference, values = get_reference(shape, mode, modulate, n_gauss)
    ngal, xi, dngal, dxi = halotab.predict_batch_grad(
        theta[:n_draws], n_gauss_prim=n_gauss, modulate_with_cenocc=modulate)
    assert dngal.shape == (n_draws, 5) and dxi.shape == (n_draws, 5, shape[2])
    what = '%s %s n=%d modulate=%s ng=%d' % (mode, shape, n_draws, modulate, n_gauss)
    assert_rel(ngal, values[0][:n_draws], RTOL, what + ' ngal')
    assert_rel(xi, values[1][:n_draws], RTOL, what + ' xi')
    assert_rel(ngal, reference[0][:n_draws], RTOL, what + ' ngal')
    check_derivatives(dngal, dxi, tuple(a[:n_draws] for a in reference), what)
    # logM0 above the top bin edge: no satellites, exactly zero derivatives
    empty = np.nonzero(theta[:n_draws, 2] >
                       get_table(shape, mode)[0]['gal_type']['log_prim_haloprop_max'].max())[0]
    for i in empty:
        assert np.all(reference[2][i, 2:] == 0.0)
        assert np.all(dngal[i, 2:] == 0.0) and np.all(dxi[i, 2:] == 0.0)


# Edges of the kernels' loops, at draw counts 1, D + 1 and 2 D + 3.  Mode auto: 2, 4, 16, 32 and
# 64 bins are 1, 1, 4, 8 and 16 steps of four matrix columns (fewer than one round of four, one
# round, two rounds whose look-ahead repeats the last step throughout) in 1, 1, 1, 2 and 4 row
# tiles, the last three without a padding row; 1, 3 and 4 r bins leave waves of the workgroup
# without an r bin or give every wave exactly one.  Mode cross: 64 and 66 bins are one slab and
# one slab plus two bins.  12 r bins reported as (3, 4) and 37 r bins (two r tiles of the
# handle's own table, which the gradient table is read back from) are further layouts; one node
# per bin is the shortest node loop.  Entries: shape, mode, tpcf_shape, n_gauss.
EDGE_CASES = (
    [(shape, 'auto', None, 10)
     for shape in [(1, 1, 1), (2, 1, 3), (8, 1, 4), (16, 1, 17), (32, 1, 2), (5, 1, 37)]] +
    [((9, 2, 12), 'auto', (3, 4), 10), ((9, 2, 12), 'cross', (3, 4), 10),
     ((32, 1, 3), 'cross', None, 10), ((33, 1, 3), 'cross', None, 10),
     ((9, 2, 5), 'auto', None, 1), ((9, 2, 5), 'cross', None, 1)])


def case_id(case):
    shape, mode, tpcf_shape, n_gauss = case
    return '%s-%dx%dx%d%s-ng%d' % ((mode, ) + shape + (
        '' if tpcf_shape is None else '-as-' + 'x'.join(map(str, tpcf_shape)), n_gauss))


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', [1, D + 1, 2 * D + 3])
@pytest.mark.parametrize('case', EDGE_CASES, ids=case_id)
def test_gradient_at_the_edges_of_the_loops(case, n_draws, modulate):
    shape, mode, tpcf_shape, n_gauss = case
    _, halotab = get_table(shape, mode, tpcf_shape)
    theta, reference, values = get_reference(shape, mode, modulate, n_gauss, tpcf_shape,
                                             usable=True)
    # no draw is dropped: every one of them has galaxies and a finite reference
    assert len(theta) == N_MAX and grad_reference.usable(reference)
    assert np.all(values[0] > 0.0) and np.all(np.isfinite(values[1]))
    ngal, xi, dngal, dxi = halotab.predict_batch_grad(
        theta[:n_draws], n_gauss_prim=n_gauss, modulate_with_cenocc=modulate)
    reported = (shape[2], ) if tpcf_shape is None else tpcf_shape
    assert ngal.shape == (n_draws, ) and xi.shape == (n_draws, ) + reported
    assert dngal.shape == (n_draws, 5) and dxi.shape == (n_draws, 5) + reported
    what = '%s n=%d modulate=%s' % (case_id(case), n_draws, modulate)
    assert_rel(ngal, values[0][:n_draws], RTOL, what + ' ngal')
    assert_rel(xi, values[1][:n_draws], RTOL, what + ' xi')
    assert_rel(ngal, reference[0][:n_draws], RTOL, what + ' ngal')
    check_derivatives(dngal, dxi, tuple(a[:n_draws] for a in reference), what)


def chi2_inputs(shape, mode, modulate, symmetric, usable=False):
    """theta, the reference, a data vector near draw 3's xi and a precision matrix."""
    theta, reference, _ = get_reference(shape, mode, modulate, 10, usable=usable)
    data, precision = chi2_data(reference[1][3], symmetric)
    return theta, reference, data, precision


def check_chi2_values(chi2, dchi2, reference, data, precision, what):
    """chi2 and dchi2 against the reference (xi and dxi with one r axis) and the allowances that
    test_chi2_gradient derives."""
    _, xi, _, dxi, scale = reference
    p_sym = 0.5 * (precision + precision.T)
    e = xi - data
    v = 2.0 * e @ p_sym
    chi2_ref = np.einsum('nr,rs,ns->n', e, precision, e)
    dchi2_ref = np.einsum('nr,nkr->nk', v, dxi)
    chi2_allow = RTOL * np.abs(chi2_ref) + RTOL * np.sum(np.abs(v) * np.abs(xi), axis=1)
    a_rk = RTOL * (np.abs(dxi) + scale[:, :, None])
    dchi2_allow = (RTOL * np.abs(dchi2_ref) + np.einsum('nr,nkr->nk', np.abs(v), a_rk) +
                   2.0 * RTOL * np.einsum('nr,nkr->nk', np.abs(xi) @ np.abs(p_sym), np.abs(dxi)))
    print('%s: max error / allowance = %.3g (chi2), %.3g (dchi2)' % (
        what, np.max(np.abs(chi2 - chi2_ref) / chi2_allow),
        np.max(np.abs(dchi2 - dchi2_ref) / np.maximum(dchi2_allow, 1e-300))))
    assert np.all(np.abs(chi2 - chi2_ref) <= chi2_allow)
    assert np.all(np.abs(dchi2 - dchi2_ref) <= dchi2_allow)


def check_chi2_gradient(shape, mode, symmetric, modulate=False, n_draws=N_MAX, usable=False):
    _, halotab = get_table(shape, mode)
    theta, reference, data, precision = chi2_inputs(shape, mode, modulate, symmetric, usable)
    theta = theta[:n_draws]
    ngal_ref, xi, dngal_ref, dxi, scale = (a[:n_draws] for a in reference)
    ngal, chi2, dngal, dchi2 = halotab.chi2_grad_batch(theta, data, precision,
                                                       modulate_with_cenocc=modulate)
    assert ngal.shape == chi2.shape == (n_draws, ) and dngal.shape == dchi2.shape == (n_draws, 5)
    check_chi2_values(chi2, dchi2, (ngal_ref, xi, dngal_ref, dxi, scale), data, precision,
                      'chi2 %s %s n=%d modulate=%s' % (mode, shape, n_draws, modulate))
    assert_rel(ngal, ngal_ref, RTOL)
    assert_rel(dngal, dngal_ref, RTOL)
    # the value agrees with the forward entry point to parity
    assert_rel(chi2, halotab.chi2_batch(theta, data, precision,
                                        modulate_with_cenocc=modulate)[1], RTOL)


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('shape,mode', [((9, 2, 5), 'auto'), ((50, 1, 19), 'auto'),
                                        ((52, 2, 21), 'auto'), ((9, 2, 5), 'cross')])
def test_chi2_gradient(shape, mode, symmetric):
    """chi2 = e^T P e and dchi2_k = 2 e^T P_sym dxi_k; the non-symmetric precision pins the
    P_sym convention.  Allowance, from the allowances of xi (1e-10 |xi|) and dxi (a_rk = 1e-10
    (|dxi_rk| + scale_k)) carried through the two formulas with v = 2 P_sym e:
    chi2: rtol + 1e-10 sum_r |v_r| |xi_r|; dchi2_k: rtol + sum_r |v_r| a_rk +
    2e-10 sum_r (|P_sym| |xi|)_r |dxi_rk|."""
    check_chi2_gradient(shape, mode, symmetric)


# The likelihood route (no xi array: residuals and derivatives stay in LDS and finish_chi2
# completes them) beyond its mildest configuration: 1, 3 and 17 r bins in mode auto (waves
# without an r bin meet the others at the barrier ahead of finish_chi2); several slabs in mode
# cross (276 x 2 x 2 bins: the products accumulate in the rows the residuals end up in) and one
# slab plus two bins; batches that end in a partial workgroup; modulate_with_cenocc.
CHI2_EDGE_CASES = [((2, 1, 3), 'auto'), ((16, 1, 17), 'auto'),
                   ((276, 2, 13), 'cross'), ((33, 1, 3), 'cross')]


@pytest.mark.parametrize('modulate', [False, True], ids=['plain', 'modulate'])
@pytest.mark.parametrize('n_draws', [1, D + 1, N_MAX])
@pytest.mark.parametrize('shape,mode', CHI2_EDGE_CASES,
                         ids=['%s-%dx%dx%d' % ((m, ) + s) for s, m in CHI2_EDGE_CASES])
def test_chi2_gradient_edges(shape, mode, n_draws, modulate):
    """As test_chi2_gradient (same reference and allowances), with the non-symmetric
    precision."""
    check_chi2_gradient(shape, mode, False, modulate, n_draws, usable=True)


def device_grad(halotab, theta, n_gauss=10, flags=0):
    """tc_predict_grad_zheng07_batch_device: ngal, xi, dngal, dxi."""
    device = halotab.to_device()
    n, n_r = len(theta), device.n_r
    return device_call(device, 'tc_predict_grad_zheng07_batch_device',
                       [theta, 5, n, n_gauss, flags], [n, (n, n_r), (n, 5), (n, 5, n_r)])


def device_chi2_grad(halotab, theta, data, precision, n_gauss=10, flags=0):
    """tc_chi2_grad_zheng07_batch_device (the data vector and the precision matrix are host
    arrays there too): ngal, chi2, dngal, dchi2."""
    from tabcorr_amd import _lib
    device = halotab.to_device()
    n = len(theta)
    data = _lib.contiguous(np.ravel(data))
    precision = _lib.contiguous(precision)
    assert data.shape == (device.n_r, ) and precision.shape == (device.n_r, device.n_r)
    return device_call(device, 'tc_chi2_grad_zheng07_batch_device',
                       [theta, 5, n, n_gauss, flags, _lib.as_double_p(data),
                        _lib.as_double_p(precision)], [n, n, (n, 5), (n, 5)])


@pytest.mark.parametrize('shape,mode', [((50, 1, 19), 'auto'), ((7, 1, 5), 'auto'),
                                        ((276, 2, 13), 'cross')])
def test_batch_invariance(shape, mode):
    """A draw's 6 (1 + R) outputs are bit-equal in batches of 1, D + 1 and 2 D + 3 draws and
    between the host-array and the device-pointer entry points."""
    _, halotab = get_table(shape, mode)
    theta, _, _ = get_reference(shape, mode, False, 10)
    full = halotab.predict_batch_grad(theta)
    for n in (1, D + 1):
        assert same_bits(halotab.predict_batch_grad(theta[:n]), [b[:n] for b in full])
    # the last draw alone, and in the middle of another batch
    assert same_bits(halotab.predict_batch_grad(theta[-1:]), [b[-1:] for b in full])
    for n in (1, D + 1, N_MAX):
        assert same_bits(device_grad(halotab, theta[:n]), [b[:n] for b in full], reshape=True)


@pytest.mark.parametrize('shape,mode', [((16, 1, 17), 'auto'), ((50, 1, 19), 'auto'),
                                        ((276, 2, 13), 'cross'), ((33, 1, 3), 'cross')])
def test_chi2_batch_invariance_and_device_entry(shape, mode):
    """The kernels have one form, so the four results of the likelihood route are bit-equal
    between the host-array and the device-pointer entry points and a draw's results bit-equal in
    batches of 1, D + 1 and 2 D + 3 draws: conditions that follow from the design, no measured
    tolerance."""
    _, halotab = get_table(shape, mode)
    theta, _, data, precision = chi2_inputs(shape, mode, False, False, usable=True)
    full = halotab.chi2_grad_batch(theta, data, precision)
    assert all(np.all(np.isfinite(a)) for a in full)
    for n in (1, D + 1, N_MAX):
        host = halotab.chi2_grad_batch(theta[:n], data, precision)
        device = device_chi2_grad(halotab, theta[:n], data, precision)
        assert same_bits(host, [c[:n] for c in full]) and same_bits(device, host)
    # the last draw alone (column 0 of its workgroup instead of column 2)
    assert same_bits(halotab.chi2_grad_batch(theta[-1:], data, precision),
                     [c[-1:] for c in full])
    # modulate_with_cenocc through the flags of the device entry
    from tabcorr_amd import _lib
    host = halotab.chi2_grad_batch(theta[:D + 1], data, precision, modulate_with_cenocc=True)
    device = device_chi2_grad(halotab, theta[:D + 1], data, precision,
                              flags=_lib.FLAG_MODULATE_WITH_CENOCC)
    assert same_bits(device, host)
    assert not np.array_equal(host[1], full[1][:D + 1])


# ---- the LDS limit --------------------------------------------------------------------------
# The documented budget of the two kernels (csrc/grad.h), in rows of D doubles.  Mode auto: three
# rows per central bin, six per satellite bin, one row of zeros, six rows of totals and, for the
# likelihood, six rows per r bin.  Mode cross: six slabs of 64 bins, six rows per r bin, six rows
# of totals, the same for the likelihood.
CROSS_SLAB = 64


def auto_lds_bytes(n_bins, n_central, n_r, chi2):
    rows = 3 * n_central + 6 * (n_bins - n_central) + 1 + 6 + (6 * n_r if chi2 else 0)
    return rows * D * 8


def cross_lds_bytes(n_r):
    return (6 * CROSS_SLAB + 6 * n_r + 6) * D * 8


def lds_limit_case(shape, mode, tpcf_shape=None):
    """Table, draws (D + 1, all with galaxies) and reference of a table at the LDS limit."""
    table, halotab = make_table(shape, mode, tpcf_shape)
    for seed in range(5, 25):
        theta = grad_reference.stress_draws(table, D + 1, seed=seed)
        reference = grad_reference.jacobian_batch(table, theta)
        if grad_reference.usable(reference):
            return table, halotab, theta, reference
    raise AssertionError('no seed gives usable draws')


def check_against_reference(halotab, theta, reference, what):
    ngal, xi, dngal, dxi = halotab.predict_batch_grad(theta)
    assert dxi.shape == reference[3].shape
    assert_rel(ngal, reference[0], RTOL, what + ' ngal')
    assert_rel(xi, reference[1], RTOL, what + ' xi')
    check_derivatives(dngal, dxi, reference, what)


def test_lds_limit_auto():
    """n_sec = 1, three r bins: the table with the most bins that predict_batch_grad serves runs
    with (nearly) the whole LDS of a CU and matches the reference; one more primary bin is
    refused."""
    n_r = 3
    n_prim = largest(lambda n: auto_lds_bytes(2 * n, n, n_r, False) <= LDS_LIMIT)
    table, halotab, theta, reference = lds_limit_case((n_prim, 1, n_r), 'auto')
    check_against_reference(halotab, theta, reference, 'LDS limit auto %d bins' % (2 * n_prim))
    table, halotab = make_table((n_prim + 1, 1, n_r), 'auto')
    check_refused(halotab, table, halotab.predict_batch_grad)


def test_lds_limit_auto_between_the_two_budgets():
    """19 r bins: the likelihood keeps 6 n_r more rows, so the largest table that
    predict_batch_grad serves is refused by chi2_grad_batch -- and served again afterwards."""
    n_r = 19
    n_prim = largest(lambda n: auto_lds_bytes(2 * n, n, n_r, False) <= LDS_LIMIT)
    assert auto_lds_bytes(2 * n_prim, n_prim, n_r, True) > LDS_LIMIT
    table, halotab, theta, reference = lds_limit_case((n_prim, 1, n_r), 'auto')
    what = 'LDS limit auto %d bins, 19 r bins' % (2 * n_prim)
    check_against_reference(halotab, theta, reference, what)
    check_refused(halotab, table,
                  lambda draws: halotab.chi2_grad_batch(draws, np.zeros(n_r), np.eye(n_r)))
    check_against_reference(halotab, theta, reference, what + ' after the refusal')


def test_lds_limit_cross():
    """Mode cross, where the budget grows with n_r alone and is the same for both calls: the most
    r bins that are served (reported on two axes when their number divides by four) against the
    reference, for the gradient and for the likelihood; one more r bin is refused by both."""
    n_r = largest(lambda n: cross_lds_bytes(n) <= LDS_LIMIT)
    tpcf_shape = (4, n_r // 4) if n_r % 4 == 0 else (n_r, )
    table, halotab, theta, reference = lds_limit_case((9, 2, n_r), 'cross', tpcf_shape)
    assert reference[3].shape == (D + 1, 5) + tpcf_shape
    check_against_reference(halotab, theta, reference, 'LDS limit cross %d r bins' % n_r)
    flat = tuple(a.reshape(a.shape[:a.ndim - len(tpcf_shape)] + (n_r, )) if i in (1, 3) else a
                 for i, a in enumerate(reference))
    rng = np.random.default_rng(11)
    data = flat[1][3] * (1.0 + 0.05 * rng.normal(size=n_r))
    precision = np.diag(rng.uniform(1.0, 2.0, size=n_r)) + 0.01 * rng.normal(size=(n_r, n_r))
    ngal, chi2, dngal, dchi2 = halotab.chi2_grad_batch(theta, data.reshape(tpcf_shape), precision)
    check_chi2_values(chi2, dchi2, flat, data, precision, 'LDS limit cross chi2')
    assert_rel(ngal, reference[0], RTOL)
    assert_rel(dngal, reference[2], RTOL)
    table, halotab = make_table((9, 2, n_r + 1), 'cross')
    check_refused(halotab, table, halotab.predict_batch_grad)
    check_refused(halotab, table, lambda draws: halotab.chi2_grad_batch(
        draws, np.zeros(n_r + 1), np.eye(n_r + 1)))


@pytest.mark.parametrize('name', ['bolplanck_wp', 'bolplanck_ds'])
def test_real_table(name):
    from tabcorr_amd import TabCorr, Zheng07Model
    from tabcorr_amd.models import ZHENG07_KEYS
    data = load_golden(name)
    table = table_from_golden(data)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                  table['tpcf_shape'], table['attrs'])
    nodes = grad_reference.nodes_of(table)
    theta = np.resize(np.array(data['theta'], dtype=np.float64), (N_MAX, 5)).copy()
    theta[len(data['theta']):] += 0.01
    theta = grad_reference.centre_log_m0(theta, nodes)
    reference = grad_reference.jacobian_batch(table, theta)
    ngal, xi, dngal, dxi = halotab.predict_batch_grad(theta)
    values = oracle.predict_zheng07_batch(table, theta)
    assert_rel(ngal, values[0], RTOL)
    assert_rel(xi, values[1], RTOL)
    check_derivatives(dngal, dxi, reference, name)
    if name == 'bolplanck_wp':
        model = Zheng07Model(redshift=0.0)
        for key, value in zip(ZHENG07_KEYS, theta[0]):
            model.param_dict[key] = value
        one = halotab.predict_grad(model)
        assert isinstance(one[0], float) and one[1].shape == tuple(table['tpcf_shape'])
        assert list(one[2]) == list(ZHENG07_KEYS) and list(one[3]) == list(ZHENG07_KEYS)
        assert one[0] == ngal[0] and np.array_equal(one[1], xi[0])
        for k, key in enumerate(ZHENG07_KEYS):
            assert one[2][key] == dngal[0, k]
            assert np.array_equal(one[3][key], dxi[0, k])


def test_unsupported_requests_leave_the_handle_usable():
    from tabcorr_amd import TabCorr, _lib
    table = synthetic.synthetic_table(9, 2, (5, ), 'auto', seed=3)
    theta = synthetic.zheng07_draws(5, seed=2)
    single = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                 table['attrs'], compute_dtype='float32')
    # (1e-5: the float32 path's stated tolerance)
    check_refused(single, table, single.predict_batch_grad, 'float64', 1e-5)

    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                  table['attrs'])
    device = halotab.to_device()
    n, n_r = len(theta), device.n_r
    outputs = [np.empty(n * 2), np.empty(n * 3 * n_r), np.empty(n * 10), np.empty(n * 15 * n_r)]
    for flags, columns in ((_lib.FLAG_SEPARATE_GAL_TYPE, 5), (_lib.FLAG_ASSEMBIAS, 7)):
        wide = np.ascontiguousarray(np.hstack([theta, np.zeros((n, 2))])[:, :columns])
        with device.lock:
            status = device.lib.tc_predict_grad_zheng07_batch(
                device.handle, _lib.as_double_p(wide), columns, n, 10, flags,
                *[_lib.as_double_p(a) for a in outputs])
        assert status == _lib.TC_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            _lib.check(status)
        check_still_serves(halotab, table)
    # and the gradient call itself still serves the handle
    reference = grad_reference.jacobian_batch(
        table, grad_reference.centre_log_m0(theta.copy(), grad_reference.nodes_of(table)))
    got = halotab.predict_batch_grad(
        grad_reference.centre_log_m0(theta.copy(), grad_reference.nodes_of(table)))
    check_derivatives(got[2], got[3], reference, 'after the refused calls')
