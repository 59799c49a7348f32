"""The host path between a derivative entry point and its launch -- the argument checks, the upload
of the likelihood's operands, the staging of host arrays, the slabs of a large batch -- is plumbing:
whoever rewrites it must change no bit.  Every derivative entry point of the three handle kinds
(table, interpolator, joint), through the host-array and the _device symbol, for every family and
form, and the occupation VJP, returns bit for bit (NaN words included) what the parent commit
returned on an MI355X (tests/golden/grad_paths_parent.npz, recorded by
tests/golden/make_grad_paths_parent.py with that commit's library) and launches the same
(workgroups, waves, slabs, LDS bytes); the recorded values pass the reference checks of the
derivative suites, with the tolerances those suites state; and a handle that has served one kind of
derivative call after another returns what a fresh handle returns, so neither the operand cache nor
anything else a call leaves behind reaches the next one.  Needs an MI355X."""

import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assembias_grad_reference  # noqa: E402
import fisher_reference  # noqa: E402
import grad_reference  # noqa: E402
import interp_grad_reference  # noqa: E402
import joint_reference  # noqa: E402
import leauthaud11_grad_reference  # noqa: E402
import vjp_reference  # noqa: E402
from derivative_kit import RTOL  # noqa: E402
from util import GOLDEN, assert_rel  # noqa: E402

pytestmark = pytest.mark.gpu


def load_recorder():
    spec = importlib.util.spec_from_file_location(
        'make_grad_paths_parent', os.path.join(GOLDEN, 'make_grad_paths_parent.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


recorder = load_recorder()
CASES = recorder.cases()
N_GAUSS = recorder.N_GAUSS


@pytest.fixture(scope='module')
def parent():
    return recorder.unpack(np.load(recorder.FILE))


# ---- the references of the derivative suites, once per (target, family, modulate) ----------------

_references = {}


def base_reference(target, family, modulate):
    """The reference of a target's N_DRAWS base draws, never modified: the 5-tuple (ngal, xi,
    dngal, dxi, scale) of grad_reference / assembias_grad_reference / leauthaud11_grad_reference
    for a table and of joint_reference for a joint, the dict of interp_grad_reference for an
    interpolator."""
    key = (target, family, modulate)
    if key not in _references:
        from oracle import tabcorr_oracle as oracle
        tables, _, points = recorder.tables_for(target)
        theta = recorder.base_draws(target, family)
        kind = recorder.kind_of(target)
        with np.errstate(all='ignore'):
            if kind == 'table':
                module = {'zheng07': grad_reference, 'assembias': assembias_grad_reference,
                          'leauthaud11': leauthaud11_grad_reference}[family]
                reference = module.jacobian_batch(tables[0], theta, N_GAUSS, modulate)
            elif kind == 'joint':
                reference = joint_reference.jacobian_batch(tables, theta, N_GAUSS, modulate,
                                                           family == 'assembias')
            else:
                setup = oracle.interpolator_setup(tables, points)
                batch = (assembias_grad_reference.interp_jacobian_batch if family == 'assembias'
                         else interp_grad_reference.jacobian_batch)
                reference = batch(tables, setup, points, theta, recorder.base_x(target), N_GAUSS,
                                  modulate)
        for array in (reference.values() if isinstance(reference, dict) else reference):
            array.setflags(write=False)
        _references[key] = reference
    return _references[key]


def rows(reference, index):
    if isinstance(reference, dict):
        return {key: value[index] for key, value in reference.items()}
    return tuple(value[index] for value in reference)


def check_table_derivatives(dngal, dxi, reference, what):
    """test_gpu_grad.py: check_derivatives -- rtol = 1e-10 plus, per (draw, k), 1e-10 x the size
    of the terms that cancel."""
    _, _, dngal_ref, dxi_ref, scale = reference
    assert_rel(dngal, dngal_ref, RTOL, what + ' dngal')
    dxi_ref = fisher_reference.flatten(dxi_ref)
    allowance = RTOL * np.abs(dxi_ref) + RTOL * scale[:, :, None]
    error = np.abs(dxi - dxi_ref)
    assert np.all(error <= allowance), (what, float(np.max(error / allowance)))


def check_table_chi2(chi2, dchi2, reference, data, precision, what):
    """test_gpu_grad.py: check_chi2_values, which joint_reference.chi2_reference restates with
    the scale per row."""
    ngal, xi, dngal, dxi, scale = reference
    n = len(ngal)
    dxi = fisher_reference.flatten(dxi)
    flat = (ngal, xi.reshape(n, -1), dngal, dxi, np.repeat(scale[:, :, None], dxi.shape[2], 2))
    joint_reference.check_chi2(chi2, dchi2, flat, data, precision, what)


def check_against_reference(case, want):
    """The recorded arrays `want` of a case (the kept draws of a large one) against the reference
    of its suite, with that suite's tolerances."""
    target, family, form = case['target'], case['family'], case['form']
    kind = recorder.kind_of(target)
    index = recorder.rows_of(case)
    if recorder.is_digest(case):
        index = np.concatenate([index[:recorder.N_EDGE], index[-recorder.N_EDGE:]])
        want = {key: np.concatenate([want[key], want[key + '$']])
                for key in want if key != 'launch' and key[-1] not in '#$'}
    n = len(index)
    n_r = recorder.n_r_of(target)
    data, precision = recorder.operands_of(n_r, case['symmetric'])
    what = '%s %s %s' % (target, family, form)
    if case['vjp']:
        table = recorder.tables_for(target)[0][0]
        occupation = recorder.base_occupations(target)[index]
        if form == 'chi2':
            ngal, chi2, dchi2, scale, xi = vjp_reference.chi2_grad_batch(table, occupation, data,
                                                                         precision)
            # (test_gpu_vjp.py: check_chi2)
            flat = xi.reshape(n, -1)
            v = 2.0 * (flat - data) @ (0.5 * (precision + precision.T))
            allow = RTOL * np.abs(chi2) + RTOL * np.sum(np.abs(v) * np.abs(flat), axis=1)
            assert_rel(want['ngal'].ravel(), ngal, RTOL, what + ' ngal')
            assert np.all(np.abs(want['chi2'].ravel() - chi2) <= allow), what
            assert np.all(np.abs(want['dchi2_docc'] - dchi2) <= RTOL * (np.abs(dchi2) + scale))
        else:
            g_xi, g_ngal = (a[index] for a in recorder.base_cotangents(target))
            ngal, xi, g, scale = vjp_reference.vjp_batch(table, occupation, g_xi, g_ngal)
            assert_rel(want['ngal'].ravel(), ngal, RTOL, what + ' ngal')
            assert_rel(want['xi'], xi.reshape(n, -1), RTOL, what + ' xi')
            # (test_gpu_vjp.py: check_gradient)
            assert np.all(np.abs(want['g_occupation'] - g) <= RTOL * (np.abs(g) + scale)), what
        return
    reference = rows(base_reference(target, family, case['modulate']), index)
    if kind == 'interp':
        assert interp_grad_reference.usable(reference), what
        q = reference['dngal'].shape[1]
        if form == 'predict':
            got = (want['ngal'].ravel(), want['xi'].reshape(reference['xi'].shape), want['dngal'],
                   want['dxi'].reshape(reference['dxi'].shape))
            interp_grad_reference.check(got, reference, what)
            return
        import test_gpu_interp_grad as interp_suite
        interp_suite.check_chi2_values((want['ngal'].ravel(), want['chi2'].ravel(), want['dngal'],
                                        want['dchi2']), reference, data, precision, what)
        dxi, a = fisher_reference.interp_jacobian(reference)
    else:
        assert grad_reference.usable(reference), what
        ngal, xi, dngal, dxi_ref, scale = reference
        q = dngal.shape[1]
        assert_rel(want['ngal'].ravel(), ngal, RTOL, what + ' ngal')
        if form == 'predict':
            got_dxi = want['dxi'].reshape(n, q, n_r)
            if kind == 'joint':
                at = 0
                for table in recorder.tables_for(target)[0]:
                    # (per table: the floor of assert_rel is that of the table's own scale)
                    part = slice(at, at + len(table['tpcf_matrix']))
                    assert_rel(want['xi'][:, part], xi[:, part], RTOL, what + ' xi')
                    at = part.stop
                joint_reference.check_derivatives(want['dngal'], got_dxi, reference, what)
            else:
                assert_rel(want['xi'], xi.reshape(n, -1), RTOL, what + ' xi')
                check_table_derivatives(want['dngal'], got_dxi, reference, what)
            return
        if kind == 'joint':
            np.testing.assert_allclose(want['dngal'], dngal, rtol=RTOL,
                                       atol=1e-14 * np.max(np.abs(dngal)))
            joint_reference.check_chi2(want['chi2'].ravel(), want['dchi2'], reference, data,
                                       precision, what)
            dxi, a = joint_reference.fisher_jacobian(reference)
        else:
            assert_rel(want['dngal'], dngal, RTOL, what + ' dngal')
            check_table_chi2(want['chi2'].ravel(), want['dchi2'], reference, data, precision, what)
            dxi, a = fisher_reference.table_jacobian(reference)
    if form == 'fisher':
        fisher_reference.check(want['fisher'].reshape(n, q, q), dxi, a, precision, what)


# ---- the bits ------------------------------------------------------------------------------------

def assert_same_bits(case, got, want, what):
    """A run's result against a recorded one."""
    got = recorder.stored_form(case, got)
    assert sorted(got) == sorted(want), what
    assert tuple(got['launch']) == tuple(want['launch']), (what, got['launch'], want['launch'])
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


@pytest.mark.parametrize('name, case', CASES, ids=[name for name, _ in CASES])
def test_same_bits_as_the_parent_commit(name, case, parent):
    recorded, unrepeatable = parent
    want = recorded[name]
    got = recorder.run_case(case)
    if name in unrepeatable:    # (the parent's own two runs differed: the reference alone judges)
        check_against_reference(case, recorder.stored_form(case, got))
    else:
        assert_same_bits(case, got, want, name)
    check_against_reference(case, want)


def test_the_recorded_cases_are_the_ones_asked_for(parent):
    recorded, unrepeatable = parent
    cases = dict(CASES)
    assert set(recorded) == set(cases)
    assert unrepeatable <= set(cases)
    assert recorder.N_DRAWS == 35 and recorder.N_SLABS == (1 << 18) + 17
    assert recorder.TABLES['auto19'][0] == recorder.TABLES['cross19'][0] == (9, 2, 19)
    assert recorder.n_r_of('joint') == 38
    assert all(shape == (3, 2, 2) for shape, _ in recorder.NARROW.values())
    # every family and form of every handle kind, through both symbols
    seen = {(recorder.kind_of(c['target']), c['family'], c['form'], c['entry'])
            for c in cases.values() if not c['vjp'] and not recorder.is_digest(c)}
    for kind, families in recorder.FAMILIES.items():
        assert {(kind, family, form, entry) for family in families for form in recorder.FORMS
                for entry in ('host', 'device')} <= seen
    assert {(c['target'], c['form'], c['entry']) for c in cases.values()
            if c['vjp'] and not recorder.is_digest(c)} == {
        (target, form, entry) for target in ('auto19', 'cross19')
        for form in ('predict', 'chi2') for entry in ('host', 'device')}
    for kind in recorder.FAMILIES:
        of_kind = [c for c in cases.values() if recorder.kind_of(c['target']) == kind]
        assert any(c['modulate'] for c in of_kind) and any(not c['symmetric'] for c in of_kind)
    # more than one slab: two launches' worth of draws, reported by the handle
    slabs = {name: c for name, c in cases.items() if recorder.is_digest(c)}
    assert {(c['target'], c['form'], c['entry']) for c in slabs.values()
            if c['family'] == 'zheng07' and not c['vjp'] and c['target'] in recorder.NARROW} == {
        (target, form, entry) for target in recorder.NARROW for form in ('predict', 'chi2')
        for entry in ('host', 'device')}
    assert {recorder.kind_of(c['target']) for c in slabs.values()} == {'table', 'interp', 'joint'}
    assert any(c['vjp'] for c in slabs.values())
    assert any(c['family'] == 'leauthaud11' and c['form'] == 'fisher' for c in slabs.values())
    for name, case in slabs.items():
        assert case['n_draws'] == recorder.N_SLABS and case['entry'] in ('host', 'device')
        # (the last launch is the second slab's: 17 draws, two workgroups of 16)
        assert recorded[name]['launch'][0] == 2, name


SEQUENCES = {'table': 'auto19', 'interp': 'interp_auto', 'joint': 'joint'}


@pytest.mark.parametrize('kind', list(SEQUENCES))
def test_nothing_a_derivative_call_set_outlives_it(kind, parent):
    """One handle: prediction gradient, likelihood with (data A, P A), Fisher matrix with (data B,
    P B), the likelihood with (data A, P A) again, predict_batch -- each returns what a fresh
    handle returns."""
    recorded, unrepeatable = parent
    cases = dict(CASES)
    target = SEQUENCES[kind]
    handles = recorder.Target(target)
    for suffix in ('_zheng07_predict_host', '_zheng07_chi2_host',
                   '_zheng07_fisher_host_nonsymmetric', '_zheng07_chi2_host'):
        name = target + suffix
        got = recorder.run_case(cases[name], handles)
        if name not in unrepeatable:
            assert_same_bits(cases[name], got, recorded[name], name)
    theta = np.ascontiguousarray(recorder.base_draws(target, 'zheng07'))
    args = [theta] + ([recorder.base_x(target)] if kind == 'interp' else [])
    kwargs = {'extrapolate': True} if kind == 'interp' else {}
    fresh = recorder.Target(target)
    used, new = ((h.halotabs[0] if kind == 'joint' else h.owner) for h in (handles, fresh))
    for got, expect in zip(used.predict_batch(*args, **kwargs), new.predict_batch(*args, **kwargs)):
        assert np.array_equal(got.view(np.uint64), expect.view(np.uint64))
