"""The occupation seam of a joint without a GPU: the composed reference of the tests against the
single-table reference on the stacked table, the LDS budget hook, the new symbols of the C ABI and
the argument checks of the Python layer."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_reference  # noqa: E402
import joint_vjp_reference  # noqa: E402
import vjp_reference  # noqa: E402
from oracle import tabcorr_oracle as oracle  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402
from derivative_kit import D, RTOL, chi2_data  # noqa: E402

NEW_SYMBOLS = ['tc_joint_predict_occupation_vjp_batch',
               'tc_joint_predict_occupation_vjp_batch_device',
               'tc_joint_chi2_occupation_grad_batch', 'tc_joint_chi2_occupation_grad_batch_device']


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def occupations(table, n_draws):
    rng = np.random.default_rng(5)
    out = [oracle.mean_occupation(table, oracle.Zheng07(theta))
           for theta in synthetic.zheng07_draws(n_draws, seed=5)]
    random = rng.uniform(0.1, 2.0, size=(n_draws, len(table['gal_type'])))
    random[rng.uniform(size=random.shape) < 0.25] = 0.0
    return np.array(out + list(random))


@pytest.mark.parametrize('symmetric', [True, False], ids=['spd', 'nonsymmetric'])
@pytest.mark.parametrize('mode', ['auto', 'cross'])
def test_composed_reference_is_the_reference_of_the_stacked_table(mode, symmetric):
    """A joint of same-mode tables is one table whose tpcf matrices are concatenated along r: the
    composition of the per-table references gives that table's chi2, gradient and scale.  18 bins,
    parts (3, ) + (6, ): the gradients agree within a tenth of the allowance 1e-10 (|ref| + scale)
    (measured: 3e-7 of it) and chi2 to 1e-13 relative; the random-cotangent VJP likewise."""
    tables = joint_reference.make_tables(9, 2, [(mode, (3, )), (mode, (6, ))])
    one = joint_vjp_reference.stacked(tables)
    occupation = occupations(tables[0], 3)
    xi = np.concatenate([np.ravel(oracle.predict(t, occupation[1])[1]) for t in tables])
    data, precision = joint_reference.coupled_data(xi, symmetric)
    assert np.all(precision[:3, 3:] != 0.0)
    got = joint_vjp_reference.chi2_grad_batch(tables, occupation, data, precision)
    expect = vjp_reference.chi2_grad_batch(one, occupation, data, precision)
    assert np.all(expect[0] > 0.0) and all(np.all(np.isfinite(a)) for a in expect)
    np.testing.assert_allclose(got[0], expect[0], rtol=1e-13)
    np.testing.assert_allclose(got[1], expect[1], rtol=1e-13)
    np.testing.assert_allclose(got[4], expect[4].reshape(got[4].shape), rtol=1e-13)
    allowance = RTOL * (np.abs(expect[2]) + expect[3])
    worst = np.max(np.abs(got[2] - expect[2]) / allowance)
    print('chi2 gradient, composed against stacked: %.3g of the allowance' % worst)
    assert worst <= 0.1
    np.testing.assert_allclose(got[3], expect[3], rtol=1e-12)

    rng = np.random.default_rng(17)
    g, g_ngal = rng.normal(size=(len(occupation), 9)), rng.normal(size=len(occupation))
    got = joint_vjp_reference.vjp_batch(tables, occupation, g, g_ngal)
    expect = vjp_reference.vjp_batch(one, occupation, g, g_ngal)
    allowance = RTOL * (np.abs(expect[2]) + expect[3])
    worst = np.max(np.abs(got[2] - expect[2]) / allowance)
    print('VJP, composed against stacked: %.3g of the allowance' % worst)
    assert worst <= 0.1
    np.testing.assert_allclose(got[3], expect[3], rtol=1e-12)


def test_mixed_joint_reference_chi2_gradient_is_the_vjp_of_its_cotangent():
    """chi2_grad of a mixed joint = vjp with g = 2 P_sym (xi - data) over all N rows."""
    tables = joint_reference.make_tables(9, 2, [('auto', (3, )), ('cross', (5, ))])
    occupation = occupations(tables[0], 2)
    xi = np.concatenate([np.ravel(oracle.predict(t, occupation[0])[1]) for t in tables])
    data, precision = chi2_data(xi, False)
    ngal, chi2, dchi2, scale, xis = joint_vjp_reference.chi2_grad_batch(
        tables, occupation, data, precision)
    g = (xis - data) @ (precision + precision.T)
    expect = joint_vjp_reference.vjp_batch(tables, occupation, g)
    assert np.array_equal(ngal, expect[0]) and np.array_equal(xis, expect[1])
    assert np.all(np.abs(dchi2 - expect[2]) <= 16 * np.finfo(float).eps * scale)


def joint_vjp_lds_bytes(n_bins, n_r_total, n_r_auto):
    """The documented budget of vjp_joint_kernel (csrc/joint.h), in rows of D doubles: w of every
    bin and one row of zeros, the auto tables' sum_r g_r U_ri of every bin; four partial q_r per
    auto row, later (P e) of all rows; the cotangent and xi of all rows; ngal and two sums."""
    return (2 * n_bins + 1 + max(4 * n_r_auto, n_r_total) + 2 * n_r_total + 3) * D * 8


def test_budget_hook_matches_the_formula(lib):
    from tabcorr_amd import _lib
    for n_bins, n_r_total, n_r_auto in ((18, 8, 3), (36, 8, 0), (60, 38, 19), (60, 38, 38),
                                        (1, 1, 0), (631, 2, 1), (632, 2, 2)):
        got = ctypes.c_int64(-1)
        _lib.check(lib.tc_debug_joint_vjp_lds_bytes(n_bins, n_r_total, n_r_auto,
                                                    ctypes.byref(got)))
        assert got.value == joint_vjp_lds_bytes(n_bins, n_r_total, n_r_auto)
    # the reference pair of tests/golden (60 bins, 19 auto rows of N = 38): 34.5 KiB; were all
    # of its rows those of mode-auto tables, 44 KiB
    assert joint_vjp_lds_bytes(60, 38, 19) == 35328 and joint_vjp_lds_bytes(60, 38, 38) == 45056
    for bad in ((0, 1, 0), (5, 0, 0), (5, 2, 3), (5, 2, -1)):
        assert lib.tc_debug_joint_vjp_lds_bytes(*bad, ctypes.byref(got)) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_joint_vjp_lds_bytes(5, 2, 1, None) == _lib.TC_ERR_INVALID


def test_library_exports_the_joint_vjp_symbols(lib):
    """Declared in the headers, present in the ctypes table and exported by the library."""
    from tabcorr_amd import _lib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    declared = entry.declared_symbols()
    for name in NEW_SYMBOLS + ['tc_debug_joint_vjp_lds_bytes']:
        assert name in declared
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    for name in NEW_SYMBOLS:
        assert len(_lib.SIGNATURES[name]) == 9


def test_joint_vjp_entry_points_refuse_a_null_handle(lib):
    from tabcorr_amd import _lib
    empty = _lib.as_double_p(np.zeros(0))
    calls = [lib.tc_joint_predict_occupation_vjp_batch(None, empty, 3, 0, None, empty, empty,
                                                       empty, empty),
             lib.tc_joint_predict_occupation_vjp_batch_device(None, None, 3, 0, None, None, None,
                                                              None, None),
             lib.tc_joint_chi2_occupation_grad_batch(None, empty, 3, 0, empty, empty, empty,
                                                     empty, empty),
             lib.tc_joint_chi2_occupation_grad_batch_device(None, None, 3, 0, empty, empty, None,
                                                            None, None)]
    for status in calls:
        assert status == _lib.TC_ERR_INVALID
        with pytest.raises(ValueError, match='joint handle is NULL'):
            _lib.check(status)


def test_joint_vjp_calls_reject_wrong_shapes_without_a_device():
    """Occupation columns, g_xis as a list and flat, g_ngal, data and precision: a ValueError of
    the four methods before any device is touched."""
    from tabcorr_amd import JointLikelihood, TabCorr
    tables = joint_reference.make_tables(3, 2, [('auto', (3, )), ('cross', (2, 2))])
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
                for t in tables]
    joint = JointLikelihood(halotabs)
    n_bins, n = len(tables[0]['gal_type']), joint.n_r_total
    assert n == 7
    good = np.ones((3, n_bins))
    good_list = [np.zeros((3, 3)), np.zeros((3, 2, 2))]
    good_data, good_precision = np.zeros(n), np.eye(n)
    for occupation in (np.ones((3, n_bins + 1)), np.ones(n_bins - 1), np.ones((3, n_bins, 1))):
        for call in (lambda: joint.predict_occupation(occupation),
                     lambda: joint.predict_vjp(occupation, good_list),
                     lambda: joint.chi2_occupation(occupation, good_data, good_precision),
                     lambda: joint.chi2_grad_occupation(occupation, good_data, good_precision)):
            with pytest.raises(ValueError, match='occupation'):
                call()
    for g_xis in ([np.zeros((3, 3))], [np.zeros((3, 3)), np.zeros((3, 4))],
                  [np.zeros((2, 3)), np.zeros((2, 2, 2))], [np.zeros((3, 2, 2)), np.zeros((3, 3))],
                  np.zeros((3, n + 1)), np.zeros((2, n)), np.zeros(n), np.zeros((3, n, 1)), None):
        with pytest.raises(ValueError, match='g_xis'):
            joint.predict_vjp(good, g_xis)
    # un-batched: the parts have the bare tpcf_shape, the flat form is (N, )
    for g_xis in (good_list, np.zeros((1, n))):
        with pytest.raises(ValueError, match='g_xis'):
            joint.predict_vjp(good[0], g_xis)
    for g_ngal in (np.zeros(2), np.zeros((3, 1)), 1.0):
        for g_xis in (good_list, np.zeros((3, n))):
            with pytest.raises(ValueError, match='g_ngal'):
                joint.predict_vjp(good, g_xis, g_ngal)
    for data, precision in ((np.zeros(n + 1), good_precision), (good_data, np.eye(n + 1)),
                            ([np.zeros(3), np.zeros(5)], good_precision),
                            (good_data, np.ones(n * n))):
        for call in (joint.chi2_occupation, joint.chi2_grad_occupation):
            with pytest.raises(ValueError, match='data'):
                call(good, data, precision)
    assert joint._device is None and all(h._device is None for h in halotabs)
