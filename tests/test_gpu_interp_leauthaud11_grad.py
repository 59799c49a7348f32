"""The interpolator's gradients of the Leauthaud11 family on the device (`family='leauthaud11'` of
Interpolator.predict_batch_grad / chi2_grad_batch / chi2_fisher_batch / fisher_batch, predict_grad
and fisher of a Leauthaud11Model, the tc_interp_*_grad_leauthaud11_* entry points) against the
reference Jacobian over (11, D) of interp_leauthaud11_grad_reference.py, the forward interpolator
and the table gradients.  Needs an MI355X.

Allowance everywhere: 1e-10 relative plus 1e-10 of the absolute scale of the terms that cancel
(interp_grad_reference.check); chi2 and dchi2 carry it as test_gpu_interp_grad.check_chi2_values
does, the Fisher matrix as fisher_reference does.  Every case prints its largest error in units
of its allowance.  The draws are leauthaud11_grad_reference.stress_draws(n, seed=5), the first n
of them for a batch of n; every test asserts that ALL of them have galaxies in every table and a
finite reference, and none is left out of a comparison.  The occupation is smooth: no draw has to
keep clear of a node.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference  # noqa: E402
import interp_leauthaud11_grad_reference as reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import D, LDS_LIMIT, RTOL, chi2_data, device_call, same_bits  # noqa: E402
from test_gpu_interp_grad import check_chi2_values, make_interpolator, make_x  # noqa: E402
from util import assert_rel  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILY = 'leauthaud11'
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARAMS = 11
N_MAX = 2 * D + 3

_cases = {}


def make_tables(grid, n_prim, n_sec, tpcf_shape, mode, classes):
    """Tables and points of a synthetic grid.  classes: 'one' (a shared gal_type), 'two' (every
    other table's n_h times 1.2: two classes interleaved in list order), 'own' (every table its
    own n_h: K classes)."""
    tables, keys, points = synthetic.synthetic_interpolator(grid, n_prim, n_sec, tpcf_shape, mode,
                                                            seed=40)
    for k, table in enumerate(tables):
        factor = {'one': 1.0, 'two': 1.2 if k % 2 else 1.0, 'own': 1.0 + 0.03 * k}[classes]
        if factor != 1.0:
            table['gal_type'] = table['gal_type'].copy()
            table['gal_type']['n_h'] *= factor
    return tables, keys, points


def finish_case(key, interp, tables, points, theta, x, modulate, n_gauss, extrapolate):
    """The reference of the draws, once: every draw has galaxies in every table."""
    setup = oracle.interpolator_setup(tables, points)
    expect = reference.jacobian_batch(tables, setup, points, theta, x, n_gauss, modulate)
    assert reference.has_galaxies(expect), key
    for array in [theta, x] + list(expect.values()):
        array.setflags(write=False)
    return {'interp': interp, 'tables': tables, 'points': points, 'setup': setup, 'theta': theta,
            'x': x, 'reference': expect, 'modulate': modulate, 'n_gauss': n_gauss,
            'extrapolate': extrapolate}


def get_case(grid, n_prim, n_sec, tpcf_shape, mode, n_draws, classes='two', modulate=False,
             n_gauss=10, x_kind='inside'):
    """Interpolator, its tables, draws (theta, x) and their reference, made once per combination
    and never modified: a batch of n draws is the first n of them."""
    key = (grid, n_prim, n_sec, tpcf_shape, mode, n_draws, classes, modulate, n_gauss, x_kind)
    if key not in _cases:
        tables, keys, points = make_tables(grid, n_prim, n_sec, tpcf_shape, mode, classes)
        setup = oracle.interpolator_setup(tables, points)
        theta = reference.draws(n_draws)
        x = make_x(points, setup, n_draws, x_kind, 5)
        _cases[key] = finish_case(key, make_interpolator(tables, keys, points), tables, points,
                                  theta, x, modulate, n_gauss, x_kind == 'outside')
    return _cases[key]


def keywords(case):
    return {'n_gauss_prim': case['n_gauss'], 'extrapolate': case['extrapolate'],
            'modulate_with_cenocc': case['modulate'], 'family': FAMILY}


def check_case(case, n, what):
    """Shapes, the reference Jacobian, and ngal / xi against the forward interpolator."""
    interp = case['interp']
    theta, x = case['theta'][:n], case['x'][:n]
    got = interp.predict_batch_grad(theta, x, **keywords(case))
    shape = tuple(interp.tabcorr_list[0].tpcf_shape)
    n_cols = N_PARAMS + len(interp.keys)
    assert got[0].shape == (n, ) and got[1].shape == (n, ) + shape
    assert got[2].shape == (n, n_cols) and got[3].shape == (n, n_cols) + shape
    reference.check(got, reference.first(case['reference'], n), what)
    ngal, xi = interp.predict_batch(theta, x, **keywords(case))
    assert_rel(got[0], ngal, RTOL, what + ' ngal against predict_batch')
    assert_rel(got[1], xi, RTOL, what + ' xi against predict_batch')
    return got


# ---- the Jacobian -------------------------------------------------------------------------------
# Mode auto: 14 and 28 bins (n_sec 1 and 2: one row tile and a second one), 18 bins (a second row
# tile with two rows); five r bins and twelve reported as (3, 4); ten nodes and one; grids of one,
# two and three dimensions (the 64 tables of the last make its reference the slow part: 3 draws).
# Mode cross: 36 bins (two slabs of 32: the second holds four bins), 66 bins (the last slab holds
# two), and the reference's database shape -- three axes, 14 r bins -- on 80 tables.
# Entries: grid, n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss, draw counts.
ONE = [1, D + 1, N_MAX]
MAIN_CASES = [
    ((4, ), 7, 1, (5, ), 'auto', False, 10, ONE),
    ((4, ), 7, 1, (5, ), 'auto', True, 10, ONE),
    ((4, ), 7, 1, (5, ), 'auto', False, 1, ONE),
    ((4, ), 7, 1, (5, ), 'auto', True, 1, ONE),
    ((4, 5), 7, 2, (5, ), 'auto', False, 10, [D + 1]),
    ((4, 5), 7, 2, (5, ), 'auto', True, 1, [D + 1]),
    ((4, 5), 9, 1, (3, 4), 'auto', True, 10, [D + 1]),
    ((4, 5), 9, 1, (3, 4), 'auto', False, 1, [D + 1]),
    ((4, 4, 4), 7, 1, (5, ), 'auto', False, 10, [3]),
    ((4, 4, 4), 7, 1, (5, ), 'auto', True, 1, [3]),
    ((4, 5), 18, 1, (5, ), 'cross', False, 10, [D + 1]),
    ((4, 5), 18, 1, (5, ), 'cross', True, 1, [D + 1]),
    ((4, ), 33, 1, (3, 4), 'cross', True, 10, ONE),
    ((4, ), 33, 1, (3, 4), 'cross', False, 1, [D + 1]),
    ((4, 5, 4), 18, 1, (14, ), 'cross', False, 10, [3]),
    ((4, 5, 4), 18, 1, (14, ), 'cross', True, 10, [3]),
]


def main_id(entry):
    grid, n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss = entry[:7]
    return '%s-%s-%dx%d-r%s-%s-ng%d' % (
        mode, 'x'.join(map(str, grid)), n_prim, n_sec, 'x'.join(map(str, tpcf_shape)),
        'modulate' if modulate else 'plain', n_gauss)


@pytest.mark.parametrize('entry', MAIN_CASES, ids=main_id)
def test_gradient_matches_reference_jacobian(entry):
    grid, n_prim, n_sec, tpcf_shape, mode, modulate, n_gauss, counts = entry
    case = get_case(grid, n_prim, n_sec, tpcf_shape, mode, max(counts), modulate=modulate,
                    n_gauss=n_gauss)
    for n in counts:
        check_case(case, n, '%s n=%d' % (main_id(entry), n))


@pytest.mark.parametrize('classes', ['one', 'two', 'own'])
@pytest.mark.parametrize('mode,n_prim', [('auto', 7), ('cross', 18)])
def test_classes_of_halo_tables(mode, n_prim, classes):
    """One class, two classes interleaved in list order, every table its own: the node loops run
    once per class, the results are those of the list."""
    # (twenty classes make the reference the slow part: the six stress draws)
    n = 6 if classes == 'own' else D + 1
    case = get_case((4, 5), n_prim, 1, (5, ), mode, n, classes=classes, modulate=True)
    n_classes = len(np.unique(case['setup']['unique_inverse']))
    assert n_classes == {'one': 1, 'two': 2, 'own': 20}[classes]
    check_case(case, n, '%s classes=%s' % (mode, classes))


@pytest.mark.parametrize('x_kind', ['node', 'outside'])
@pytest.mark.parametrize('mode,n_prim', [('auto', 7), ('cross', 18)])
def test_positions_of_x(mode, n_prim, x_kind):
    """On a grid node, and beyond the grid on both sides with extrapolate=True ('inside' is every
    other case of this file)."""
    case = get_case((4, 5), n_prim, 1, (5, ), mode, D + 1, x_kind=x_kind)
    n = D + 1
    got = check_case(case, n, '%s x=%s' % (mode, x_kind))
    if x_kind == 'outside':
        xp = case['setup']['xp']
        assert all(np.all((case['x'][:, d] < xp[d][0]) | (case['x'][:, d] > xp[d][-1]))
                   for d in range(2))
        with pytest.raises(ValueError, match='extrapolation'):
            case['interp'].predict_batch_grad(case['theta'], case['x'], family=FAMILY)
    if x_kind == 'node':
        # the value and the theta derivatives are those of the node's table
        expect = case['reference']
        for k in range(0, n, 5):
            table = case['interp'].tabcorr_list[k % 20]
            one = table.predict_batch_grad(case['theta'][k:k + 1], family=FAMILY)
            mine = (got[0][k:k + 1], got[1][k:k + 1], got[2][k:k + 1, :N_PARAMS],
                    got[3][k:k + 1, :N_PARAMS])
            for name, a, b in zip(('ngal', 'xi', 'dngal', 'dxi'), mine, one):
                scale = expect[name + '_scale'][k:k + 1]
                scale = scale[:, :N_PARAMS] if name in ('dngal', 'dxi') else scale
                assert np.all(np.abs(a - b) <= RTOL * np.abs(b) + RTOL * scale), (name, k)


@pytest.mark.parametrize('mode,n_prim', [('auto', 7), ('cross', 18)])
def test_grid_of_identical_tables(mode, n_prim):
    """d/dx is zero within the allowance and d/dtheta that of the single table."""
    key = ('identical', mode)
    if key not in _cases:
        tables, keys, points = synthetic.synthetic_interpolator((4, 5), n_prim, 1, (5, ), mode,
                                                                seed=40)
        tables = [tables[0]] * len(tables)
        setup = oracle.interpolator_setup(tables, points)
        n = D + 1
        _cases[key] = finish_case(key, make_interpolator(tables, keys, points), tables, points,
                                  reference.draws(n), make_x(points, setup, n, 'inside', 5),
                                  True, 10, False)
    case = _cases[key]
    expect, theta = case['reference'], case['theta']
    got = check_case(case, len(theta), 'identical tables %s' % mode)
    assert np.all(np.abs(got[2][:, N_PARAMS:]) <= RTOL * expect['dngal_scale'][:, N_PARAMS:])
    assert np.all(np.abs(got[3][:, N_PARAMS:]) <= RTOL * expect['dxi_scale'][:, N_PARAMS:])
    one = case['interp'].tabcorr_list[0].predict_batch_grad(theta, modulate_with_cenocc=True,
                                                            family=FAMILY)
    for name, a, b in (('ngal', got[0], one[0]), ('xi', got[1], one[1]),
                       ('dngal', got[2][:, :N_PARAMS], one[2]),
                       ('dxi', got[3][:, :N_PARAMS], one[3])):
        scale = expect[name + '_scale']
        scale = scale[:, :N_PARAMS] if name in ('dngal', 'dxi') else scale
        assert np.all(np.abs(a - b) <= RTOL * np.abs(b) + RTOL * scale), name


# ---- the likelihood and the Fisher matrix --------------------------------------------------------

def fixture_case():
    """The reference's own interpolator tests/golden/ds_efficient.hdf5: four mode-cross tables of
    1104 bins (35 slabs of 32, the last holds 16 bins), 13 r bins, one axis; 3 draws."""
    key = 'ds_efficient'
    if key not in _cases:
        from tabcorr_amd import Interpolator
        interp = Interpolator.read(os.path.join(REPO, 'tests', 'golden', 'ds_efficient.hdf5'))
        tables = [{'gal_type': h.gal_type.as_array(),
                   'tpcf_matrix': np.asarray(h.tpcf_matrix, dtype=np.float64),
                   'tpcf_shape': tuple(h.tpcf_shape), 'attrs': dict(h.attrs)}
                  for h in interp.tabcorr_list]
        assert len(tables) == 4 and len(tables[0]['gal_type']) == 1104
        assert tables[0]['attrs']['mode'] == 'cross' and len(tables[0]['tpcf_matrix']) == 13
        points = np.asarray(interp.points, dtype=np.float64)
        setup = oracle.interpolator_setup(tables, points)
        _cases[key] = finish_case(key, interp, tables, points, reference.draws(3),
                                  make_x(points, setup, 3, 'inside', 5), True, 10, False)
    return _cases[key]


def likelihood_inputs(case, symmetric):
    """A data vector near the last draw's xi and a precision matrix in units of |xi| (a lensing
    signal spans decades over its r bins), symmetric positive definite or not."""
    xi = case['reference']['xi'][-1].ravel()
    data, precision = chi2_data(xi, symmetric)
    size = np.abs(data)
    return data, precision / np.outer(size, size)


LIKELIHOOD_CASES = {
    'auto-4x5-28': lambda: get_case((4, 5), 7, 2, (5, ), 'auto', D + 1, modulate=True),
    'cross-4-66': lambda: get_case((4, ), 33, 1, (3, 4), 'cross', N_MAX, modulate=True),
    'cross-4x5x4-36-r14': lambda: get_case((4, 5, 4), 18, 1, (14, ), 'cross', 3),
    'ds_efficient': fixture_case,
}


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('name', list(LIKELIHOOD_CASES))
def test_likelihood_and_fisher(name, symmetric):
    """chi2, dchi2 and fisher (11 + D, 11 + D) against the reference Jacobian; the non-symmetric
    precision pins the P_sym convention.  `chi2_fisher_batch`'s first four results are the bits of
    `chi2_grad_batch`, `fisher_batch` is its Fisher matrix bit for bit, which is symmetric to the
    bit and does not depend on the data."""
    case = LIKELIHOOD_CASES[name]()
    interp, theta, x, expect = case['interp'], case['theta'], case['x'], case['reference']
    n = len(theta)
    n_cols = N_PARAMS + len(interp.keys)
    shape = tuple(interp.tabcorr_list[0].tpcf_shape)
    data, precision = likelihood_inputs(case, symmetric)
    what = 'likelihood %s %s' % (name, 'spd' if symmetric else 'nonsymmetric')
    got = interp.chi2_fisher_batch(theta, x, data.reshape(shape), precision, **keywords(case))
    assert [g.shape for g in got] == [(n, ), (n, ), (n, n_cols), (n, n_cols), (n, n_cols, n_cols)]
    check_chi2_values(got[:4], expect, data, precision, what)
    dxi, a = fisher_reference.interp_jacobian(expect)
    _, allow = fisher_reference.check(got[4], dxi, a, precision, what)
    assert np.array_equal(got[4], got[4].transpose(0, 2, 1))
    if symmetric:
        for matrix, bound in zip(got[4], allow):
            assert np.linalg.eigvalsh(matrix)[0] >= -np.max(bound)
    assert same_bits(got[:4], interp.chi2_grad_batch(theta, x, data, precision,
                                                     **keywords(case)))
    forecast = interp.fisher_batch(theta, x, precision, **keywords(case))
    assert same_bits(forecast, (got[0], got[2], got[4]))
    # the value agrees with the forward entry point to parity
    assert_rel(got[1], interp.chi2_batch(theta, x, data, precision, n_gauss_prim=case['n_gauss'],
                                         modulate_with_cenocc=case['modulate'], family=FAMILY)[1],
               RTOL, what + ' chi2 against chi2_batch')


# ---- batch invariance and the device entries -----------------------------------------------------

def device_entry(interp, theta, x, flags, data=None, precision=None, fisher=False):
    """tc_interp_predict_grad_leauthaud11_batch_device or, with data, the likelihood entry, with
    its Fisher matrix or with NULL in its place."""
    from tabcorr_amd import _lib
    device = interp.to_device()
    n, n_r, n_cols = len(theta), device.tables[0].n_r, N_PARAMS + x.shape[1]
    arguments = [theta, 14, x, n, 10, flags]
    if data is None:
        return device_call(device, 'tc_interp_predict_grad_leauthaud11_batch_device', arguments,
                           [n, (n, n_r), (n, n_cols), (n, n_cols, n_r)], 'tc_interp_synchronize')
    data, precision = _lib.contiguous(np.ravel(data)), _lib.contiguous(precision)
    arguments += [_lib.as_double_p(data), _lib.as_double_p(precision)]
    shapes = [n, n, (n, n_cols), (n, n_cols)]
    if fisher:
        return device_call(device, 'tc_interp_chi2_grad_leauthaud11_batch_device', arguments,
                           shapes + [(n, n_cols, n_cols)], 'tc_interp_synchronize')

    class WithoutFisher:
        """device_call's view of the handle whose entry gets NULL behind the four outputs."""
        lock, handle, lib = device.lock, device.handle, None

        def __getattr__(self, name):
            entry = getattr(device.lib, name)
            if name.endswith('_batch_device'):
                return lambda handle, *passed: entry(handle, *passed, None)
            return entry

    view = WithoutFisher()
    view.lib = view
    return device_call(view, 'tc_interp_chi2_grad_leauthaud11_batch_device', arguments, shapes,
                       'tc_interp_synchronize')


@pytest.mark.parametrize('entry', [((4, ), 7, 1, (5, ), 'auto'), ((4, ), 33, 1, (3, 4), 'cross')],
                         ids=['auto-4-14', 'cross-4-66'])
def test_batch_invariance_and_device_entries(entry):
    """The kernels have one form and every sum an order fixed by the interpolator: a draw alone and
    at positions 0, 15, 16 and last of a batch of 35 gives the same bits, and so do the
    device-pointer entries -- conditions that follow from the design, no tolerance."""
    from tabcorr_amd import _lib
    grid, n_prim, n_sec, tpcf_shape, mode = entry
    case = get_case(grid, n_prim, n_sec, tpcf_shape, mode, N_MAX, modulate=True)
    interp, theta, x = case['interp'], case['theta'], case['x']
    assert len(theta) == 35
    data, precision = likelihood_inputs(case, False)
    words = keywords(case)
    full = interp.predict_batch_grad(theta, x, **words)
    full_fisher = interp.chi2_fisher_batch(theta, x, data, precision, **words)
    assert all(np.all(np.isfinite(a)) for a in full + full_fisher)
    for k in (0, D - 1, D, len(theta) - 1):
        alone = interp.predict_batch_grad(theta[k:k + 1], x[k:k + 1], **words)
        assert same_bits(alone, [c[k:k + 1] for c in full]), k
        alone = interp.chi2_fisher_batch(theta[k:k + 1], x[k:k + 1], data, precision, **words)
        assert same_bits(alone, [c[k:k + 1] for c in full_fisher]), k
    for n in (1, D + 1):
        part = interp.chi2_fisher_batch(theta[:n], x[:n], data, precision, **words)
        assert same_bits(part, [c[:n] for c in full_fisher]), n
    # another data vector: the same Fisher matrix
    other = interp.chi2_fisher_batch(theta, x, 2.0 * data, precision, **words)
    assert np.array_equal(other[4], full_fisher[4])
    flags = _lib.FLAG_MODULATE_WITH_CENOCC
    for n in (1, D + 1, len(theta)):
        assert same_bits(device_entry(interp, theta[:n], x[:n], flags), [c[:n] for c in full],
                         reshape=True)
        assert same_bits(device_entry(interp, theta[:n], x[:n], flags, data, precision, True),
                         [c[:n] for c in full_fisher])
        assert same_bits(device_entry(interp, theta[:n], x[:n], flags, data, precision, False),
                         [c[:n] for c in full_fisher[:4]])


# ---- model objects -------------------------------------------------------------------------------

def test_predict_grad_and_fisher_of_a_model():
    """`predict_grad` and `fisher` of a Leauthaud11Model at z = 0.3: the smhm_*_0 and the six own
    entries are the bits of the batch of device_theta(), the smhm_*_a entries (a - 1) times them,
    the extra parameters' their own columns, and the Fisher matrix is J^T F J with J =
    blockdiag(device_jacobian(), I_D)."""
    from tabcorr_amd import Leauthaud11Model
    from tabcorr_amd.models import LEAUTHAUD11_KEYS
    tables, grid_keys, points = make_tables((4, 5), 9, 1, (3, 4), 'auto', 'two')
    tables = [dict(table, attrs=dict(table['attrs'], redshift=0.3)) for table in tables]
    interp = make_interpolator(tables, grid_keys, points)
    setup = oracle.interpolator_setup(tables, points)
    assert tuple(interp.keys) == ('log_eta', 'alpha_s')
    model = Leauthaud11Model(threshold=10.7, redshift=0.3, modulate_with_cenocc=True)
    model.param_dict['smhm_m1_a'] = 0.4
    model.param_dict['smhm_gamma_a'] = -0.6
    x = make_x(points, setup, 3, 'inside', 5)[2]
    for key, value in zip(interp.keys, x):
        model.param_dict[key] = value
    theta = model.device_theta()[np.newaxis]
    a = 1.0 / (1.0 + model.redshift)
    ngal, xi, dngal, dxi = interp.predict_batch_grad(theta, x[np.newaxis],
                                                     modulate_with_cenocc=True, family=FAMILY)
    expect = reference.jacobian_batch(tables, setup, points, theta, x[np.newaxis], modulate=True)
    assert reference.has_galaxies(expect)
    reference.check((ngal, xi, dngal, dxi), expect, 'model draw')
    keys = tuple(LEAUTHAUD11_KEYS) + tuple(interp.keys)
    one = interp.predict_grad(model)
    assert isinstance(one[0], float) and one[0] == ngal[0] and np.array_equal(one[1], xi[0])
    assert one[1].shape == (3, 4) and tuple(one[2]) == keys and tuple(one[3]) == keys
    column = {key: (j // 2 if j < 10 else j - 5) for j, key in enumerate(LEAUTHAUD11_KEYS)}
    column.update({key: N_PARAMS + d for d, key in enumerate(interp.keys)})
    for key in keys:
        factor = (a - 1.0) if key.startswith('smhm') and key.endswith('_a') else 1.0
        assert one[2][key] == factor * dngal[0, column[key]], key
        assert np.array_equal(one[3][key], factor * dxi[0, column[key]]), key
    _, precision = likelihood_inputs({'reference': expect}, False)
    batch = interp.fisher_batch(theta, x[np.newaxis], precision, modulate_with_cenocc=True,
                                family=FAMILY)
    got = interp.fisher(model, precision)
    assert isinstance(got[0], float) and got[0] == batch[0][0] == ngal[0]
    assert tuple(got[1]) == keys
    assert all(got[1][key] == one[2][key] for key in keys)
    jacobian = np.zeros((13, 18))
    jacobian[:11, :16] = model.device_jacobian()
    jacobian[11:, 16:] = np.eye(2)
    assert got[2].shape == (18, 18)
    assert np.array_equal(got[2], jacobian.T @ batch[2][0] @ jacobian)
    # a model without modulate_with_cenocc decides for itself
    plain = Leauthaud11Model(threshold=10.7, redshift=0.3, modulate_with_cenocc=False)
    plain.param_dict.update(model.param_dict)
    other = interp.predict_grad(plain)
    expect = interp.predict_batch_grad(theta, x[np.newaxis], family=FAMILY)
    assert other[0] == expect[0][0] != one[0]


# ---- refusals ------------------------------------------------------------------------------------

def test_refusals_leave_everything_usable():
    """Plain size and argument checks.  Mode auto, 128 bins, five r bins, one axis: the eleven
    parameters need 173 824 bytes of LDS and are refused, the five of Zheng07 need 87 296 and are
    served, and so is the forward call of the family; a float32 interpolator is refused."""
    assert (7 * 64 + 12 * 64 + 1 + 12 + 64 + 13 * 5) * D * 8 == 173824 > LDS_LIMIT
    tables, keys, points = make_tables((4, ), 64, 1, (5, ), 'auto', 'two')
    interp = make_interpolator(tables, keys, points)
    setup = oracle.interpolator_setup(tables, points)
    theta = reference.draws(5)
    x = make_x(points, setup, 5, 'inside', 5)
    with pytest.raises(NotImplementedError, match='LDS'):
        interp.predict_batch_grad(theta, x, family=FAMILY)
    with pytest.raises(NotImplementedError, match='LDS'):
        interp.chi2_fisher_batch(theta, x, np.zeros(5), np.eye(5), family=FAMILY)
    ngal, xi = interp.predict_batch(theta, x, family=FAMILY)
    expect = [reference.predict(tables, setup, t, xv) for t, xv in zip(theta, x)]
    assert_rel(ngal, np.array([e[0] for e in expect]), RTOL, 'forward ngal after the refusal')
    assert_rel(xi, np.array([e[1] for e in expect]), RTOL, 'forward xi after the refusal')
    zheng = synthetic.zheng07_draws(5, seed=2)
    got = interp.predict_batch_grad(zheng, x)
    forward = interp.predict_batch(zheng, x)
    assert_rel(got[0], forward[0], RTOL, 'Zheng07 ngal after the refusal')
    assert_rel(got[1], forward[1], RTOL, 'Zheng07 xi after the refusal')
    assert np.all(np.isfinite(got[2])) and np.all(np.isfinite(got[3]))
    # float32 tables
    tables, keys, points = make_tables((4, 5), 7, 1, (5, ), 'auto', 'two')
    single = make_interpolator(tables, keys, points, compute_dtype='float32')
    x = make_x(points, None, 5, 'inside', 5)
    with pytest.raises(NotImplementedError, match='float64'):
        single.predict_batch_grad(theta, x, family=FAMILY)
    with pytest.raises(NotImplementedError, match='float64'):
        single.fisher_batch(theta, x, np.eye(5), family=FAMILY)
    # the family is in the entry point: its flag, and every flag but modulate, is refused
    from tabcorr_amd import _lib
    interp = make_interpolator(tables, keys, points)
    device = interp.to_device()
    outputs = [np.empty(5), np.empty((5, 5)), np.empty((5, 13)), np.empty((5, 13, 5))]
    for flags in (_lib.FLAG_LEAUTHAUD11, _lib.FLAG_ASSEMBIAS, _lib.FLAG_SEPARATE_GAL_TYPE):
        with device.lock:
            status = device.lib.tc_interp_predict_grad_leauthaud11_batch(
                device.handle, _lib.as_double_p(theta), 14, _lib.as_double_p(x), 5, 10, flags,
                *[_lib.as_double_p(a) for a in outputs])
        assert status == _lib.TC_ERR_UNSUPPORTED
    with device.lock:
        status = device.lib.tc_interp_predict_grad_leauthaud11_batch(
            device.handle, _lib.as_double_p(theta), 11, _lib.as_double_p(x), 5, 10, 0,
            *[_lib.as_double_p(a) for a in outputs])
    assert status == _lib.TC_ERR_INVALID
    got = interp.predict_batch_grad(theta, x, family=FAMILY)
    forward = interp.predict_batch(theta, x, family=FAMILY)
    assert_rel(got[0], forward[0], RTOL, 'ngal after the refused flags')
    assert_rel(got[1], forward[1], RTOL, 'xi after the refused flags')
