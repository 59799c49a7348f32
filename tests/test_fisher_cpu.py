"""The Fisher-matrix calls without a GPU: the argument checks of the Python layer (a wrong shape
is a ValueError before any device is touched), the refusal of a model that is not plain Zheng07,
the four C entry points without a handle, and the reference helper on a case with a known
answer."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fisher_reference  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def make_table(tpcf_shape=(5, )):
    from tabcorr_amd import TabCorr
    table = synthetic.synthetic_table(7, 1, tpcf_shape, 'auto', seed=3)
    return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                               table['attrs'])


def make_interpolator(grid=(4, 5), tpcf_shape=(5, )):
    from tabcorr_amd import Interpolator, TabCorr
    tables, keys, points = synthetic.synthetic_interpolator(grid, 4, 1, tpcf_shape, 'auto', seed=7)
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
                for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)}), points


def bad_operands(tpcf_shape):
    """(data, precision) pairs that do not fit n_r: one of the two is wrong in each."""
    n_r = int(np.prod(tpcf_shape))
    data, precision = np.zeros(tpcf_shape), np.eye(n_r)
    return [(np.zeros(n_r + 1), precision), (np.zeros(n_r - 1), precision),
            (np.zeros((n_r, 2)), precision), (data, np.eye(n_r + 1)),
            (data, np.ones((n_r, n_r + 1))), (data, np.ones(n_r * n_r)),
            (data, np.ones((n_r, n_r, 1)))]


@pytest.mark.parametrize('tpcf_shape', [(5, ), (3, 4)])
def test_table_calls_reject_wrong_shapes_before_any_device_is_touched(tpcf_shape):
    halotab = make_table(tpcf_shape)
    n_r = int(np.prod(tpcf_shape))
    theta = synthetic.zheng07_draws(3, seed=2)
    data, precision = np.zeros(tpcf_shape), np.eye(n_r)
    for columns in (7, 4):                       # the assembly-bias layout, a short one
        with pytest.raises(ValueError, match='theta'):
            halotab.chi2_fisher_batch(np.zeros((3, columns)), data, precision)
        with pytest.raises(ValueError, match='theta'):
            halotab.fisher_batch(np.zeros((3, columns)), precision)
    for bad_data, bad_precision in bad_operands(tpcf_shape):
        with pytest.raises(ValueError, match='precision'):
            halotab.chi2_fisher_batch(theta, bad_data, bad_precision)
        if bad_precision.shape != precision.shape:
            with pytest.raises(ValueError, match='precision'):
                halotab.fisher_batch(theta, bad_precision)
    assert halotab._device is None


@pytest.mark.parametrize('tpcf_shape', [(5, ), (3, 4)])
def test_interpolator_calls_reject_wrong_shapes_before_any_device_is_touched(tpcf_shape):
    interp, points = make_interpolator(tpcf_shape=tpcf_shape)
    n_r = int(np.prod(tpcf_shape))
    theta = synthetic.zheng07_draws(3, seed=2)
    x = np.tile(points.mean(axis=0), (3, 1))
    data, precision = np.zeros(tpcf_shape), np.eye(n_r)

    def both(theta, x, **kwargs):
        with pytest.raises(ValueError):
            interp.chi2_fisher_batch(theta, x, data, precision, **kwargs)
        with pytest.raises(ValueError):
            interp.fisher_batch(theta, x, precision, **kwargs)

    for columns in (7, 4):
        both(np.zeros((3, columns)), x)
    both(theta, x[:2])                           # one row of x missing
    both(theta, x[:, :1])                        # one column of x missing
    both(theta, np.hstack([x, x[:, :1]]))        # one column too many
    outside = x.copy()
    outside[1, 0] = points[:, 0].max() + 0.01
    both(theta, outside)
    with pytest.raises(ValueError, match='extrapolation'):
        interp.fisher_batch(theta, outside, precision, extrapolate=False)
    for bad_data, bad_precision in bad_operands(tpcf_shape):
        with pytest.raises(ValueError, match='precision'):
            interp.chi2_fisher_batch(theta, x, bad_data, bad_precision)
        if bad_precision.shape != precision.shape:
            with pytest.raises(ValueError, match='precision'):
                interp.fisher_batch(theta, x, bad_precision)
    assert interp._device is None
    assert all(halotab._device is None for halotab in interp.tabcorr_list)


def test_fisher_of_a_model_needs_a_plain_zheng07_model():
    """An assembly-bias model is a NotImplementedError of `fisher`, for a table and for an
    interpolator (where a missing extra parameter is a ValueError), before any device is
    touched."""
    from tabcorr_amd import Zheng07Model
    halotab = make_table()
    biased = Zheng07Model(redshift=0.0, sec_haloprop_key='halo_nfw_conc')
    with pytest.raises(NotImplementedError, match='plain Zheng07'):
        halotab.fisher(biased, np.eye(5), check_consistency=False)
    assert halotab._device is None

    interp, points = make_interpolator()
    model = Zheng07Model(redshift=0.0)
    with pytest.raises(ValueError, match='log_eta'):
        interp.fisher(model, np.eye(5), check_consistency=False)
    for d, key in enumerate(interp.keys):
        biased.param_dict[key] = points[:, d].mean()
    with pytest.raises(NotImplementedError, match='plain Zheng07'):
        interp.fisher(biased, np.eye(5), check_consistency=False)
    assert interp._device is None
    assert all(halotab._device is None for halotab in interp.tabcorr_list)


def test_c_entry_points_refuse_a_call_without_a_handle(lib):
    from tabcorr_amd import _lib
    empty = np.zeros(0)
    theta = synthetic.zheng07_draws(3, seed=2)
    p = _lib.as_double_p
    status = lib.tc_chi2_fisher_zheng07_batch(None, p(theta), 5, 3, 10, 0, *[p(empty)] * 7)
    assert status == _lib.TC_ERR_INVALID
    with pytest.raises(ValueError):
        _lib.check(status)
    assert lib.tc_chi2_fisher_zheng07_batch_device(
        None, None, 5, 3, 10, 0, p(empty), p(empty), None, None, None, None,
        None) == _lib.TC_ERR_INVALID
    assert lib.tc_interp_chi2_fisher_zheng07_batch(
        None, p(theta), 5, p(empty), 3, 10, 0, *[p(empty)] * 7) == _lib.TC_ERR_INVALID
    assert lib.tc_interp_chi2_fisher_zheng07_batch_device(
        None, None, 5, None, 3, 10, 0, p(empty), p(empty), None, None, None, None,
        None) == _lib.TC_ERR_INVALID


def test_reference_on_a_case_with_a_known_answer():
    """The helper's einsum and its allowance: with the identity for a precision matrix F is the
    Gram matrix of the Jacobian columns, a non-symmetric precision enters through P_sym alone,
    and the allowance of an exact Jacobian (a = 0) is the parity bar on the terms of the sum."""
    rng = np.random.default_rng(4)
    dxi = rng.normal(size=(3, 5, 7))
    assert np.allclose(fisher_reference.fisher(dxi, np.eye(7)),
                       dxi @ dxi.transpose(0, 2, 1), rtol=1e-13, atol=1e-13)
    precision = rng.normal(size=(7, 7))
    got = fisher_reference.fisher(dxi, precision)
    assert np.allclose(got, fisher_reference.fisher(dxi, precision.T), rtol=1e-13, atol=1e-13)
    assert np.allclose(got, got.transpose(0, 2, 1), rtol=1e-13, atol=1e-13)
    skew = precision - precision.T
    assert np.all(np.abs(fisher_reference.fisher(dxi, skew)) < 1e-13)
    allow = fisher_reference.allowance(dxi, np.zeros_like(dxi), np.eye(7))
    assert np.allclose(allow, 1e-10 * np.abs(dxi) @ np.abs(dxi).transpose(0, 2, 1), rtol=1e-13)
