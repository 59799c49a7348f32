"""Reference Jacobian of an interpolator's (ngal, xi) with respect to (theta, x) for the Leauthaud11
family: the eleven differentiated parameters (`tabcorr_amd.models.LEAUTHAUD11_GRAD_KEYS`, the
first eleven of the fourteen theta columns) and the D extra parameters, in NumPy from
`leauthaud11_grad_reference.jacobian` per table and `interp_grad_reference.table_weights`, built
the way `interp_grad_reference.jacobian` is.  A helper of the interpolator's Leauthaud11 gradient
tests, not a test module.

The checks are those of interp_grad_reference.py (`check`, `usable`, `first`) on the dict this
module returns: the same keys, the same scale rules, 11 for 5.
"""

import numpy as np

import interp_grad_reference
import leauthaud11_grad_reference
from oracle import tabcorr_oracle as oracle

N_PARAMS = leauthaud11_grad_reference.N_PARAMS
check, usable, first = (interp_grad_reference.check, interp_grad_reference.usable,
                        interp_grad_reference.first)


def draws(n_draws):
    """The draws of every test of this family's interpolator gradients:
    `leauthaud11_grad_reference.stress_draws(n, seed=5)`."""
    return leauthaud11_grad_reference.stress_draws(n_draws, seed=5)


def jacobian(tables, setup, points, theta, x, n_gauss_prim=10, modulate=False):
    """Of one draw (theta (14), x (D)), as the dict of `interp_grad_reference.jacobian`: ngal, xi
    (tpcf_shape), dngal (11 + D), dxi (11 + D, ) + tpcf_shape and their scales -- ngal_scale,
    xi_scale: sum_t |c_t| |(ngal_t, xi_t)|; dngal_scale, dxi_scale: theta columns sum_t |c_t|
    (|dngal_{t,k}|, scale_{t,k} of `leauthaud11_grad_reference.jacobian`), x columns
    sum_t |dc_t/dx_d| |(ngal_t, xi_{t,r})|, with |c_t| and |dc_t| the products of the sums of
    absolute polynomial terms."""
    with interp_grad_reference.occupations_once_per_class(tables, setup) as cache:
        per_table = [leauthaud11_grad_reference.jacobian(table, theta, n_gauss_prim, modulate)
                     for table in tables]
        cache.clear()
    ngal_t = np.array([r[0] for r in per_table])             # (K)
    xi_t = np.array([r[1] for r in per_table])               # (K, ) + shape
    dngal_t = np.array([r[2] for r in per_table])            # (K, 11)
    dxi_t = np.array([r[3] for r in per_table])              # (K, 11) + shape
    scale_t = np.array([r[4] for r in per_table])            # (K, 11)
    c, dc, abs_c, abs_dc = interp_grad_reference.table_weights(setup, points, x)
    ones = (1, ) * (xi_t.ndim - 1)
    return {
        'ngal': c @ ngal_t,
        'xi': np.tensordot(c, xi_t, 1),
        'dngal': np.concatenate([c @ dngal_t, dc @ ngal_t]),
        'dxi': np.concatenate([np.tensordot(c, dxi_t, 1), np.tensordot(dc, xi_t, 1)]),
        'ngal_scale': abs_c @ np.abs(ngal_t),
        'xi_scale': np.tensordot(abs_c, np.abs(xi_t), 1),
        'dngal_scale': np.concatenate([abs_c @ np.abs(dngal_t), abs_dc @ np.abs(ngal_t)]),
        'dxi_scale': np.concatenate([
            (abs_c @ scale_t).reshape((N_PARAMS, ) + ones) * np.ones(xi_t.shape[1:]),
            np.tensordot(abs_dc, np.abs(xi_t), 1)]),
        'ngal_tables': ngal_t,
    }


def jacobian_batch(tables, setup, points, theta, x, n_gauss_prim=10, modulate=False):
    results = [jacobian(tables, setup, points, t, xv, n_gauss_prim, modulate)
               for t, xv in zip(np.atleast_2d(theta), np.atleast_2d(x))]
    return {key: np.array([r[key] for r in results]) for key in results[0]}


def has_galaxies(reference):
    """Whether every table has galaxies in every draw and all of the reference is finite: what
    the tests assert of ALL their draws (none is left out of a comparison)."""
    return bool(np.all(reference['ngal_tables'] > 0.0)) and usable(reference)


def predict(tables, setup, theta, x, n_gauss_prim=10, modulate=False):
    """(ngal, xi) of one draw from the oracle's interpolator, x clamped to the outermost
    polynomial: for central differences."""
    return oracle.interpolator_predict(tables, setup, oracle.Leauthaud11(theta, modulate), x,
                                       n_gauss_prim=n_gauss_prim, extrapolate=True)
