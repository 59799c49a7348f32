"""Reference Fisher matrix of the likelihood, F[k, l] = dxi_k^T P_sym dxi_l with P_sym = (P + P^T)
/ 2, in NumPy from a reference Jacobian (`grad_reference.jacobian_batch` for a table,
`interp_grad_reference.jacobian_batch` for an interpolator), and its allowance.  A helper of the
Fisher tests, not a test module.

The allowance is the gradient suites' own bar carried through the bilinear form, no new number:
they allow |error of dxi_k[r]| <= a_k[r] = 1e-10 (|dxi_k[r]| + scale_k[r]), so

    allow[k, l] = sum_rs |P_sym[r, s]| (a_k[r] |dxi_l[s]| + |dxi_k[r]| a_l[s])
                  + 1e-10 sum_rs |P_sym[r, s] dxi_k[r] dxi_l[s]|

-- the first-order effect of the two factors' errors plus the parity bar on the terms of the sum
itself.
"""

import numpy as np

RTOL = 1e-10                         # the project's parity bar


def flatten(dxi):
    """(n, Q) + tpcf_shape -> (n, Q, n_r)."""
    return dxi.reshape(dxi.shape[0], dxi.shape[1], -1)


def table_jacobian(reference):
    """dxi (n, 5, n_r) and its allowance a (n, 5, n_r) from a `grad_reference.jacobian_batch`
    result: a = 1e-10 (|dxi| + scale_k)."""
    dxi = flatten(reference[3])
    return dxi, RTOL * (np.abs(dxi) + reference[4][:, :, None])


def interp_jacobian(reference):
    """dxi (n, 5 + D, n_r) and its allowance from an `interp_grad_reference.jacobian_batch`
    result: a = 1e-10 (|dxi| + dxi_scale)."""
    dxi = flatten(reference['dxi'])
    return dxi, RTOL * (np.abs(dxi) + flatten(reference['dxi_scale']))


def fisher(dxi, precision):
    """F (n, Q, Q) = einsum('kr,rs,ls', dxi, P_sym, dxi) per draw."""
    p_sym = 0.5 * (precision + precision.T)
    return np.einsum('nkr,rs,nls->nkl', dxi, p_sym, dxi)


def allowance(dxi, a, precision):
    abs_p = np.abs(0.5 * (precision + precision.T))
    abs_dxi = np.abs(dxi)
    return (np.einsum('nkr,rs,nls->nkl', a, abs_p, abs_dxi) +
            np.einsum('nkr,rs,nls->nkl', abs_dxi, abs_p, a) +
            RTOL * np.einsum('nkr,rs,nls->nkl', abs_dxi, abs_p, abs_dxi))


def check(got, dxi, a, precision, what):
    """`got` (n, Q, Q) against the reference of the first n draws of (dxi, a).  Prints the
    largest error in units of the allowance and returns it with the allowance."""
    n = len(got)
    dxi, a = dxi[:n], a[:n]
    expect = fisher(dxi, precision)
    allow = allowance(dxi, a, precision)
    assert got.shape == expect.shape, (what, got.shape, expect.shape)
    error = np.abs(got - expect)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(error == 0.0, 0.0, error / allow)
    worst = float(np.max(ratio))
    print('%s: max |fisher - reference| / allowance = %.3g' % (what, worst))
    assert np.all(error <= allow), (what, worst)
    return worst, allow
