"""A joint fit of w_p and DeltaSigma over a grid of simulations, with a covariance that couples
the two probes: 128 Levenberg-Marquardt searches at once for the five Zheng07 parameters AND the
two extra parameters x of the grid.  Two synthetic interpolators over the same 4 x 4 grid (w_p:
mode auto; DeltaSigma: mode cross; one ``gal_type`` table) stand for the reference's ``wp`` /
``ds`` pair; (ngal, w_p, DeltaSigma) of a known (theta, x) are the data.  Every step of all
searches is ONE ``JointInterpolator.chi2_fisher_batch`` call -- the occupations of every class of
halo tables once, both members' contractions at every grid node, chi2, its gradient and the
Gauss-Newton normal matrix over all seven parameters against the full (N, N) precision matrix from
one kernel launch -- plus a batched ``np.linalg.solve``.  Two ``Interpolator`` calls could not
apply the off-diagonal blocks at all, nor form that matrix.  NumPy only.

    python examples/example_joint_interp_fit.py
"""

import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
from tabcorr_amd import Interpolator, JointInterpolator, TabCorr, synthetic  # noqa: E402

N_SEARCHES = 128


def make_interpolator(mode, tpcf_shape):
    """One member: a 4 x 4 grid of synthetic tables of 24 bins; the same seed gives every member
    the same gal_type table."""
    tables, keys, points = synthetic.synthetic_interpolator((4, 4), 12, 1, tpcf_shape, mode,
                                                            seed=40)
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
                for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)})


joint = JointInterpolator([make_interpolator('auto', (7, )), make_interpolator('cross', (7, ))])
n, n_wp = joint.n_r_total, joint.slices[0].stop
keys = ('logMmin', 'sigma_logM', 'logM0', 'logM1', 'alpha') + tuple(joint.keys)
x_low = np.array([xp[0] for xp in joint.interpolators[0].xp])
x_high = np.array([xp[-1] for xp in joint.interpolators[0].xp])

truth = np.concatenate([[12.02, 0.26, 11.38, 13.31, 1.06], x_low + 0.37 * (x_high - x_low)])
LOW = np.concatenate([truth[:5] - [0.4, 0.15, 0.5, 0.4, 0.3], x_low])
HIGH = np.concatenate([truth[:5] + [0.4, 0.3, 0.5, 0.4, 0.3], x_high])
ngal_true, xis_true, _, _ = joint.predict_batch_grad(truth[:5], truth[5:])
ngal_true = ngal_true[0]
data = np.concatenate([xi[0].ravel() for xi in xis_true])
sigma_ngal = 0.05 * ngal_true
# 5 per cent errors on every bin, neighbouring bins correlated -- and every w_p bin with the
# DeltaSigma bin of the same radius: the covariance has off-diagonal blocks
sigma = 0.05 * np.abs(data)
index = np.arange(n)
radius = np.where(index < n_wp, index, index - n_wp)
same_probe = (index[:, np.newaxis] < n_wp) == (index[np.newaxis, :] < n_wp)
correlation = np.where(same_probe, 0.5, 0.3)**(1.0 + np.abs(radius[:, np.newaxis] -
                                                           radius[np.newaxis, :]))
correlation[index, index] = 1.0
precision = np.linalg.inv(correlation * sigma[:, np.newaxis] * sigma[np.newaxis, :])
assert np.any(precision[:n_wp, n_wp:] != 0.0)


def likelihood(parameters):
    """chi2, half its gradient and its Gauss-Newton normal matrix over (theta, x) for every row,
    from ONE call.  The ngal term is added here from dngal: an outer product completes it."""
    ngal, chi2, dngal, dchi2, fisher = joint.chi2_fisher_batch(
        parameters[:, :5], parameters[:, 5:], data, precision)
    pull = (ngal - ngal_true) / sigma_ngal
    slope = dngal / sigma_ngal
    chi2 = chi2 + pull**2
    half_gradient = 0.5 * dchi2 + pull[:, np.newaxis] * slope
    normal = fisher + slope[:, :, np.newaxis] * slope[:, np.newaxis, :]
    bad = ~(np.isfinite(chi2) & np.all(np.isfinite(half_gradient), axis=1) &
            np.all(np.isfinite(normal), axis=(1, 2)))
    chi2[bad], half_gradient[bad], normal[bad] = np.inf, 0.0, np.eye(len(keys))
    return chi2, half_gradient, normal


rng = np.random.default_rng(7)
parameters = rng.uniform(LOW, HIGH, size=(N_SEARCHES, len(keys)))
chi2, half_gradient, normal = likelihood(parameters)
damping = np.full(N_SEARCHES, 1e-2)
print('start   best chi2 = %10.3e  median = %10.3e' % (np.min(chi2), np.median(chi2)))
for step in range(300):
    # Levenberg-Marquardt: (N + damping diag(N)) delta = -grad / 2, for every search at once
    diagonal = np.einsum('nkk->nk', normal)
    diagonal = np.where(diagonal > 0.0, diagonal, 1.0)
    damped = normal + np.einsum('n,nk,kl->nkl', damping, diagonal, np.eye(len(keys)))
    delta = np.linalg.solve(damped, -half_gradient[:, :, np.newaxis])[:, :, 0]
    trial = np.clip(parameters + delta, LOW, HIGH)
    chi2_trial, half_gradient_trial, normal_trial = likelihood(trial)
    better = chi2_trial < chi2
    parameters[better], chi2[better] = trial[better], chi2_trial[better]
    half_gradient[better], normal[better] = half_gradient_trial[better], normal_trial[better]
    damping = np.where(better, np.maximum(damping / 3.0, 1e-9), np.minimum(damping * 4.0, 1e12))
    if step % 20 == 19:
        print('step %3d best chi2 = %10.3e  median = %10.3e  searches below 1e-6: %d' % (
            step + 1, np.min(chi2), np.median(chi2), np.sum(chi2 < 1e-6)))
    if np.min(chi2) < 1e-16:
        break

best = int(np.argmin(chi2))
print('%d of %d searches ended below chi2 = 1e-6; the best one after %d steps:' % (
    np.sum(chi2 < 1e-6), N_SEARCHES, step + 1))

# Fisher forecast over (theta, x) at the best fit: the data-free form of the same launch
ngal, dngal, fisher = joint.fisher_batch(parameters[best, :5], parameters[best, 5:], precision)
total = fisher[0] + np.outer(dngal[0], dngal[0]) / sigma_ngal**2
errors = np.sqrt(np.diag(np.linalg.inv(total)))
for key, fit, true, error in zip(keys, parameters[best], truth, errors):
    print('%-11s fit %9.5f   truth %9.5f   forecast 1 sigma %8.5f' % (key, fit, true, error))
assert chi2[best] < 1e-6, 'none of the searches converged'
