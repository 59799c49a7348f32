"""The occupation seam of an interpolator without a GPU: the reference of the tests
(interp_vjp_reference.py) against the oracle's interpolator and its central differences, the LDS
budget of the two kernels through its host-only hook, the new symbols of the C ABI and the
argument checks of the Python layer."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interp_vjp_reference as reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

EPS = np.finfo(np.float64).eps
NEW_SYMBOLS = ['tc_interp_info', 'tc_interp_predict_occupation_vjp_batch',
               'tc_interp_predict_occupation_vjp_batch_device',
               'tc_interp_chi2_occupation_grad_batch',
               'tc_interp_chi2_occupation_grad_batch_device']


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def make_case(grid, mode, seed=7):
    """Tables of a synthetic grid in two interleaved classes (every other table has its own
    n_h), the oracle's setup and the reference's walk."""
    tables, keys, points = synthetic.synthetic_interpolator(grid, 4, 1, (5, ), mode, seed=seed)
    for k, table in enumerate(tables):
        if k % 2:
            table['gal_type'] = table['gal_type'].copy()
            table['gal_type']['n_h'] *= 1.3
    setup = oracle.interpolator_setup(tables, points)
    return tables, keys, points, setup, reference.Walk(tables, setup, points)


def draws(walk, n_draws, seed):
    """Per-class occupations (Zheng07 and random with exact zeros, in turn, drawn independently
    per class) and x inside the grid."""
    rng = np.random.default_rng(seed)
    n_bins = len(walk.tables[0]['gal_type'])
    low, high = walk.points.min(axis=0), walk.points.max(axis=0)
    out = []
    for d in range(n_draws):
        rows = []
        for k in walk.class_tables:
            if d % 2 == 0:
                theta = synthetic.zheng07_draws(1, seed=int(rng.integers(1 << 30)))[0]
                rows.append(oracle.mean_occupation(walk.tables[k], oracle.Zheng07(theta)))
            else:
                row = rng.uniform(0.1, 2.0, size=n_bins)
                row[rng.choice(n_bins, size=2, replace=False)] = 0.0
                rows.append(row)
        out.append((np.array(rows), rng.uniform(low, high)))
    return out


CASES = [((4, ), 'auto'), ((4, 5), 'auto'), ((4, 5), 'cross')]
IDS = ['auto-4', 'auto-4x5', 'cross-4x5']


@pytest.mark.parametrize('grid,mode', CASES, ids=IDS)
def test_reference_forward_is_the_oracles_interpolator(grid, mode):
    """(ngal, xi) of the reference against `oracle.interpolator_predict` at the same per-class
    occupations (mapped through setup['unique_inverse']), to 1e-13; the classes are two,
    interleaved, numbered by first appearance."""
    tables, _, _, setup, walk = make_case(grid, mode)
    assert list(walk.table_class) == [k % 2 for k in range(len(tables))]
    assert list(walk.class_tables) == [0, 1]
    for occupation, x in draws(walk, 6, seed=5):
        got = reference.vjp(walk, occupation, x, np.zeros(5))
        ngal, xi = reference.oracle_predict(tables, setup, walk.table_class, occupation, x)
        np.testing.assert_allclose(got['ngal'], ngal, rtol=1e-13)
        np.testing.assert_allclose(got['xi'], np.ravel(xi), rtol=1e-13)
    # outside the grid the outermost polynomial continues
    occupation, x = draws(walk, 1, seed=6)[0]
    x = walk.points.max(axis=0) + 0.05
    got = reference.vjp(walk, occupation, x, np.zeros(5))
    ngal, xi = reference.oracle_predict(tables, setup, walk.table_class, occupation, x)
    np.testing.assert_allclose(got['xi'], np.ravel(xi), rtol=1e-13)
    with pytest.raises(ValueError, match='extrapolation'):
        reference.oracle_predict(tables, setup, walk.table_class, occupation, x, extrapolate=False)


def central_differences(tables, setup, walk, occupation, x, h_n, h_x):
    """d(ngal, xi)/dn[v, i] (C, n_bins[, n_r]) and d(ngal, xi)/dx_d (D[, n_r]) by central
    differences of the oracle's interpolator at the per-class occupations."""
    def f(occ, xv):
        ngal, xi = reference.oracle_predict(tables, setup, walk.table_class, occ, xv)
        return ngal, np.ravel(xi)

    dn = np.zeros(occupation.shape), np.zeros(occupation.shape + (5, ))
    for index in np.ndindex(occupation.shape):
        e = np.zeros(occupation.shape)
        e[index] = h_n
        a, b = f(occupation + e, x), f(occupation - e, x)
        dn[0][index] = (a[0] - b[0]) / (2 * h_n)
        dn[1][index] = (a[1] - b[1]) / (2 * h_n)
    dx = np.zeros(len(x)), np.zeros((len(x), 5))
    for d in range(len(x)):
        e = np.zeros(len(x))
        e[d] = h_x
        a, b = f(occupation, x + e), f(occupation, x - e)
        dx[0][d] = (a[0] - b[0]) / (2 * h_x)
        dx[1][d] = (a[1] - b[1]) / (2 * h_x)
    return dn, dx


@pytest.mark.parametrize('grid,mode', CASES, ids=IDS)
def test_reference_vjp_matches_central_differences(grid, mode):
    """The rows of the Jacobian that the reference gives for unit cotangents (one r at a time,
    then g_ngal = 1 alone) against central differences of the oracle's interpolator in single
    occupation entries (step 1e-3, as tests/test_vjp_cpu.py) and in x (step 1e-4, as
    tests/test_interp_grad_cpu.py): |J - FD(h/2)| <= |FD(h) - FD(h/2)| + 8 eps S / (h/2),
    elementwise, with S the interpolated value's scale sum_t |c_t| |f_t| (never below max |f|):
    the allowance of those two tests, no free tolerance.  Every x is more than 4 h from the
    knots."""
    tables, _, _, setup, walk = make_case(grid, mode)
    h_n, h_x = 1e-3, 1e-4
    worst = 0.0
    for occupation, x in draws(walk, 4, seed=5):
        for d, xp in enumerate(setup['xp']):
            assert np.min(np.abs(xp - x[d])) > 4 * h_x
        coarse = central_differences(tables, setup, walk, occupation, x, h_n, h_x)
        fine = central_differences(tables, setup, walk, occupation, x, h_n / 2, h_x / 2)
        unit = reference.vjp(walk, occupation, x, np.zeros(5), 1.0)
        rows = [reference.vjp(walk, occupation, x, np.eye(5)[r]) for r in range(5)]
        jac_n = np.stack([row['g_occupation'] for row in rows], axis=-1)
        jac_x = np.stack([row['g_x'] for row in rows], axis=-1)
        # the sizes of the differenced values: the tables' own, with the absolute weights
        _, _, abs_c, _ = reference.interp_grad_reference.table_weights(setup, walk.points, x)
        per_table = walk.per_table(occupation, np.zeros(5), 0.0)
        size_ngal = abs_c @ np.array([r[0] for r in per_table])
        size_xi = np.max(abs_c @ np.abs(np.array([np.ravel(r[1]) for r in per_table])))
        for analytic, f1, f2, size, h in (
                (unit['g_occupation'], coarse[0][0], fine[0][0], size_ngal, h_n),
                (jac_n, coarse[0][1], fine[0][1], size_xi, h_n),
                (unit['g_x'], coarse[1][0], fine[1][0], size_ngal, h_x),
                (unit['dngal_dx'], coarse[1][0], fine[1][0], size_ngal, h_x),
                (jac_x, coarse[1][1], fine[1][1], size_xi, h_x)):
            bound = np.abs(f1 - f2) + 8 * EPS * size / (h / 2)
            worst = max(worst, np.max(np.abs(analytic - f2) / bound))
            assert np.all(np.abs(analytic - f2) <= bound)
        # a random cotangent is the same linear combination of those rows
        rng = np.random.default_rng(7)
        g_xi, g_ngal = rng.normal(size=5), rng.normal()
        combined = reference.vjp(walk, occupation, x, g_xi, g_ngal)
        assert np.all(np.abs(combined['g_occupation'] - (g_ngal * unit['g_occupation'] +
                                                         jac_n @ g_xi))
                      <= 32 * EPS * combined['g_occupation_scale'])
        assert np.all(np.abs(combined['g_x'] - (g_ngal * unit['g_x'] + jac_x @ g_xi))
                      <= 32 * EPS * combined['g_x_scale'])
    print('worst |J - FD(h/2)| / bound:', worst)


@pytest.mark.parametrize('grid,mode', CASES[1:], ids=IDS[1:])
def test_reference_chi2_gradient_is_the_vjp_of_its_cotangent(grid, mode):
    """chi2_grad = vjp with g = 2 P_sym (xi - data) of the interpolated xi and g_ngal = 0 (a
    non-symmetric precision pins the P_sym convention), and its chi2 is e^T P e."""
    _, _, _, _, walk = make_case(grid, mode)
    rng = np.random.default_rng(11)
    precision = np.eye(5) * 5 + rng.normal(size=(5, 5))
    for occupation, x in draws(walk, 2, seed=5):
        xi = reference.vjp(walk, occupation, x, np.zeros(5))['xi']
        data = xi * (1.0 + 0.05 * rng.normal(size=5))
        got = reference.chi2_grad(walk, occupation, x, data, precision)
        e = xi - data
        assert got['chi2'] == e @ precision @ e
        expect = reference.vjp(walk, occupation, x, (precision + precision.T) @ e)
        for name in ('g_occupation', 'g_x'):
            assert np.all(np.abs(got[name] - expect[name]) <= 32 * EPS * got[name + '_scale'])
            assert np.all(got[name + '_scale'] >= expect[name + '_scale'] * (1 - 32 * EPS))
        assert np.array_equal(got['dngal_dx'], expect['dngal_dx'])


# ---- the LDS budget ------------------------------------------------------------------------------

def lds_bytes(lib, mode, n_bins, n_r, n_dim):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    _lib.check(lib.tc_debug_interp_vjp_lds_bytes({'auto': 0, 'cross': 1}[mode], n_bins, n_r, n_dim,
                                                 ctypes.byref(got)))
    return got.value


def test_lds_budget_is_the_hand_counted_rows(lib):
    """Rows of 16 doubles (128 bytes).  Both kernels: per axis 32 weights and 32 derivative
    weights; per r bin the cotangent, the interpolated xi and n_dim accumulators of dxi/dx; four
    rows of per-draw sums.  Mode auto adds w of every bin and a row of zeros, per bin the table's
    sum_r g_r U_ri and the class accumulator, four per-wave partials of q_r and the class's share
    of xi per r bin; mode cross one slab of 64 bins and (1 + n_dim) products per r bin."""
    # 18 bins, 3 r bins, one axis
    common = 64 + (1 + 1 + 1) * 3 + 4
    assert lds_bytes(lib, 'auto', 18, 3, 1) == 128 * ((18 + 1) + 18 + 18 + 4 * 3 + 3 + common)
    assert lds_bytes(lib, 'cross', 18, 3, 1) == 128 * (64 + 2 * 3 + common)
    # 32 bins, 19 r bins, two axes
    common = 128 + (1 + 1 + 2) * 19 + 4
    assert lds_bytes(lib, 'auto', 32, 19, 2) == 128 * ((32 + 1) + 32 + 32 + 4 * 19 + 19 + common)
    assert lds_bytes(lib, 'cross', 1104, 19, 2) == 128 * (64 + 3 * 19 + common)
    # mode cross does not read n_bins: any number of bins is served
    assert lds_bytes(lib, 'cross', 1104, 13, 2) == lds_bytes(lib, 'cross', 5, 13, 2)
    # the first mode-auto shape beyond 160 KiB, one axis and three r bins (tests/
    # test_gpu_interp_vjp.py refuses it on the device): 3 n_bins + 1 + 15 + 77 rows of 1280
    limit = 160 * 1024
    first = next(n for n in range(1, 2000) if lds_bytes(lib, 'auto', n, 3, 1) > limit)
    assert first == 396 and 3 * 395 + 93 == 1278 and 3 * 396 + 93 > 1280
    assert lds_bytes(lib, 'auto', first - 1, 3, 1) <= limit
    from tabcorr_amd import _lib
    for bad in ((2, 18, 3, 1), (0, 0, 3, 1), (0, 18, 0, 1), (0, 18, 3, 0), (0, 18, 3, 9)):
        got = ctypes.c_int64(-1)
        assert lib.tc_debug_interp_vjp_lds_bytes(*bad, ctypes.byref(got)) == _lib.TC_ERR_INVALID


# ---- the C ABI and the Python layer ----------------------------------------------------------------

def test_library_exports_the_seam_symbols(lib):
    """Declared in the headers, present in the ctypes table and exported by the library."""
    from tabcorr_amd import _lib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    declared = entry.declared_symbols()
    for name in NEW_SYMBOLS + ['tc_debug_interp_vjp_lds_bytes']:
        assert name in declared
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES['tc_interp_predict_occupation_vjp_batch']) == 11
    assert len(_lib.SIGNATURES['tc_interp_chi2_occupation_grad_batch']) == 12


def test_entry_points_refuse_a_null_handle(lib):
    from tabcorr_amd import _lib
    empty = _lib.as_double_p(np.zeros(0))
    calls = [lib.tc_interp_predict_occupation_vjp_batch(None, empty, empty, 3, 0, None, empty,
                                                        empty, empty, empty, empty),
             lib.tc_interp_predict_occupation_vjp_batch_device(None, None, None, 3, 0, None, None,
                                                               None, None, None, None),
             lib.tc_interp_chi2_occupation_grad_batch(None, empty, empty, 3, 0, empty, empty,
                                                      empty, empty, empty, empty, empty),
             lib.tc_interp_chi2_occupation_grad_batch_device(None, None, None, 3, 0, empty, empty,
                                                             None, None, None, None, None),
             lib.tc_interp_info(None, None, None, None, None)]
    for status in calls:
        assert status == _lib.TC_ERR_INVALID
        with pytest.raises(ValueError):
            _lib.check(status)


def make_interpolator(tables, keys, points):
    from tabcorr_amd import Interpolator, TabCorr
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
                for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)})


def test_classes_occupations_and_class_weights_on_the_host(lib):
    """table_class / class_tables are the reference's classes by first appearance; mean_occupation
    is the oracle's per class; class_weights sums the host helper's c_t over a class -- all
    without a device."""
    tables, keys, points, setup, walk = make_case((4, 5), 'cross')
    interp = make_interpolator(tables, keys, points)
    assert np.array_equal(interp.table_class, walk.table_class)
    assert np.array_equal(interp.class_tables, walk.class_tables)
    from tabcorr_amd import Zheng07Model
    model = Zheng07Model(redshift=0.0)
    theta = [model.param_dict[key] for key in ('logMmin', 'sigma_logM', 'logM0', 'logM1', 'alpha')]
    occupation = interp.mean_occupation(model, check_consistency=False)
    assert occupation.shape == (2, len(tables[0]['gal_type']))
    for v, k in enumerate(walk.class_tables):
        np.testing.assert_allclose(
            occupation[v], oracle.mean_occupation(tables[k], oracle.Zheng07(theta)), rtol=1e-10)
    rng = np.random.default_rng(3)
    x = rng.uniform(points.min(axis=0) - 0.02, points.max(axis=0) + 0.02, size=(7, 2))
    got = interp.class_weights(x)
    assert got.shape == (7, 2)
    for d in range(7):
        c, _, abs_c, _ = reference.interp_grad_reference.table_weights(setup, points, x[d])
        for v in range(2):
            members = walk.table_class == v
            assert abs(got[d, v] - np.sum(c[members])) <= 64 * EPS * np.sum(abs_c[members])
    np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=1e-10)
    with pytest.raises(ValueError, match='x must have shape'):
        interp.class_weights(np.zeros((3, 3)))
    assert interp._device is None


@pytest.mark.parametrize('tpcf_shape', [(5, ), (3, 4)])
def test_seam_calls_reject_wrong_shapes_without_a_device(tpcf_shape):
    """The occupation array, x (its shape and its range), g_xi, g_ngal, data and precision: a
    ValueError of the four calls before any device is touched."""
    tables, keys, points = synthetic.synthetic_interpolator((4, 5), 4, 1, tpcf_shape, 'auto',
                                                            seed=7)
    for k, table in enumerate(tables):
        if k % 2:
            table['gal_type'] = table['gal_type'].copy()
            table['gal_type']['n_h'] *= 1.3
    interp = make_interpolator(tables, keys, points)
    n_bins, n_r = len(tables[0]['gal_type']), int(np.prod(tpcf_shape))
    good = np.ones((3, 2, n_bins))
    x = np.tile(points.mean(axis=0), (3, 1))
    good_g = np.zeros((3, ) + tpcf_shape)
    data, precision = np.zeros(tpcf_shape), np.eye(n_r)

    def all_four(occupation, x, match):
        for call in (lambda: interp.predict_occupation(occupation, x),
                     lambda: interp.predict_vjp(occupation, x, good_g),
                     lambda: interp.chi2_occupation(occupation, x, data, precision),
                     lambda: interp.chi2_grad_occupation(occupation, x, data, precision)):
            with pytest.raises(ValueError, match=match):
                call()

    # (n, n_bins) is for one class only; a class or a bin missing or too many
    for occupation in (np.ones((3, n_bins)), np.ones((3, 1, n_bins)), np.ones((3, 3, n_bins)),
                       np.ones((3, 2, n_bins + 1)), np.ones((2, n_bins)), np.ones(n_bins)):
        all_four(occupation, x, 'occupation')
    for bad_x in (x[:2], x[:, :1], np.hstack([x, x[:, :1]])):
        all_four(good, bad_x, 'x must have shape')
    for d in range(2):
        for value in (points[:, d].min() - 0.01, points[:, d].max() + 0.01, np.nan):
            outside = x.copy()
            outside[1, d] = value
            all_four(good, outside, 'extrapolation')
    for g_xi in (np.zeros((2, ) + tpcf_shape), np.zeros((3, n_r + 1)), np.zeros(tpcf_shape)):
        with pytest.raises(ValueError, match='g_xi'):
            interp.predict_vjp(good, x, g_xi)
    with pytest.raises(ValueError, match='g_xi'):
        interp.predict_vjp(good, x, None)
    for g_ngal in (np.zeros(2), np.zeros((3, 1)), 1.0):
        with pytest.raises(ValueError, match='g_ngal'):
            interp.predict_vjp(good, x, good_g, g_ngal)
    for bad_data, bad_precision in ((np.zeros(n_r + 1), precision), (data, np.eye(n_r + 1)),
                                    (data, np.ones(n_r * n_r))):
        with pytest.raises(ValueError, match='precision'):
            interp.chi2_grad_occupation(good, x, bad_data, bad_precision)
        with pytest.raises(ValueError, match='precision'):
            interp.chi2_occupation(good, x, bad_data, bad_precision)
    assert interp._device is None
    assert all(halotab._device is None for halotab in interp.tabcorr_list)
