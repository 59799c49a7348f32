"""A joint fit of w_p and DeltaSigma with a covariance that couples the two probes: 256
Levenberg-Marquardt searches at once for the five Zheng07 parameters.  (ngal, w_p, DeltaSigma) of
a known parameter vector are the data; every step of all searches is ONE
``JointLikelihood.chi2_fisher_batch`` call -- the occupations once per draw, both tables'
contractions, chi2, its gradient and the Gauss-Newton normal matrix against the full (N, N)
precision matrix from one kernel launch -- plus a batched ``np.linalg.solve``.  The two tables'
own calls could not apply the off-diagonal blocks on the device at all.  NumPy only.

    python examples/example_joint_fit.py
"""

import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
from tabcorr_amd import JointLikelihood, TabCorr  # noqa: E402

KEYS = ('logMmin', 'sigma_logM', 'logM0', 'logM1', 'alpha')
LOW = np.array([11.0, 0.05, 10.5, 12.0, 0.5])
HIGH = np.array([14.0, 1.0, 13.5, 15.0, 1.6])
N_SEARCHES = 256


def read_npz(fname):
    """A table kept as arrays: gal_type columns gt_*, tpcf_matrix, tpcf_shape and attrs."""
    data = np.load(fname)
    columns = [key[3:] for key in data.files if key.startswith('gt_')]
    gal_type = np.zeros(len(data['gt_n_h']), dtype=[(c, data['gt_' + c].dtype) for c in columns])
    for c in columns:
        gal_type[c] = data['gt_' + c]
    return TabCorr.from_arrays(gal_type, data['tpcf_matrix'].astype(np.float64),
                               data['tpcf_shape'], json.loads(str(data['attrs'])))


# the two tables of one halo catalogue: the same gal_type table, mode auto and mode cross
golden = os.path.join(REPO, 'tests', 'golden')
halotab_wp = read_npz(os.path.join(golden, 'bolplanck_wp.npz'))
halotab_ds = read_npz(os.path.join(golden, 'bolplanck_ds.npz'))
joint = JointLikelihood([halotab_wp, halotab_ds])
n = joint.n_r_total

truth = np.array([12.02, 0.26, 11.38, 13.31, 1.06])
ngal_true, xis_true, _, _ = joint.predict_batch_grad(truth)
ngal_true = ngal_true[0]
data = np.concatenate([xi[0].ravel() for xi in xis_true])
sigma_ngal = 0.05 * ngal_true
# 5 per cent errors on every bin, neighbouring bins correlated -- and every w_p bin with the
# DeltaSigma bin of the same radius: the covariance has off-diagonal blocks
sigma = 0.05 * np.abs(data)
index = np.arange(n)
n_wp = joint.slices[0].stop
radius = np.where(index < n_wp, index, index - n_wp)
same_probe = (index[:, np.newaxis] < n_wp) == (index[np.newaxis, :] < n_wp)
correlation = np.where(same_probe, 0.5, 0.3)**(1.0 + np.abs(radius[:, np.newaxis] -
                                                           radius[np.newaxis, :]))
correlation[index, index] = 1.0
covariance = correlation * sigma[:, np.newaxis] * sigma[np.newaxis, :]
precision = np.linalg.inv(covariance)
assert np.any(precision[:n_wp, n_wp:] != 0.0)


def likelihood(theta):
    """chi2, half its gradient and its Gauss-Newton normal matrix for every row of theta, from
    ONE call.  The ngal term is added here from dngal: an outer product completes the matrix."""
    ngal, chi2, dngal, dchi2, fisher = joint.chi2_fisher_batch(theta, data, precision)
    pull = (ngal - ngal_true) / sigma_ngal
    slope = dngal / sigma_ngal
    chi2 = chi2 + pull**2
    half_gradient = 0.5 * dchi2 + pull[:, np.newaxis] * slope
    normal = fisher + slope[:, :, np.newaxis] * slope[:, np.newaxis, :]
    # a start without galaxies (or a step into such a place) has no finite likelihood: it counts
    # as infinitely bad and does not move
    bad = ~(np.isfinite(chi2) & np.all(np.isfinite(half_gradient), axis=1) &
            np.all(np.isfinite(normal), axis=(1, 2)))
    chi2[bad], half_gradient[bad], normal[bad] = np.inf, 0.0, np.eye(5)
    return chi2, half_gradient, normal


rng = np.random.default_rng(7)
theta = rng.uniform(LOW, HIGH, size=(N_SEARCHES, 5))
chi2, half_gradient, normal = likelihood(theta)
damping = np.full(N_SEARCHES, 1e-2)
print('start   best chi2 = %10.3e  median = %10.3e' % (np.min(chi2), np.median(chi2)))
for step in range(200):
    # Levenberg-Marquardt: (N + damping diag(N)) delta = -grad / 2, for every search at once
    diagonal = np.einsum('nkk->nk', normal)
    diagonal = np.where(diagonal > 0.0, diagonal, 1.0)
    damped = normal + np.einsum('n,nk,kl->nkl', damping, diagonal, np.eye(5))
    delta = np.linalg.solve(damped, -half_gradient[:, :, np.newaxis])[:, :, 0]
    trial = np.clip(theta + delta, LOW, HIGH)
    chi2_trial, half_gradient_trial, normal_trial = likelihood(trial)
    better = chi2_trial < chi2
    theta[better], chi2[better] = trial[better], chi2_trial[better]
    half_gradient[better], normal[better] = half_gradient_trial[better], normal_trial[better]
    damping = np.where(better, np.maximum(damping / 3.0, 1e-9), np.minimum(damping * 4.0, 1e12))
    if step % 10 == 9:
        print('step %3d best chi2 = %10.3e  median = %10.3e  searches below 1e-6: %d' % (
            step + 1, np.min(chi2), np.median(chi2), np.sum(chi2 < 1e-6)))
    if np.min(chi2) < 1e-16:
        break

best = int(np.argmin(chi2))
print('%d of %d searches ended below chi2 = 1e-6; the best one after %d steps:' % (
    np.sum(chi2 < 1e-6), N_SEARCHES, step + 1))

# Fisher forecast at the best fit, joint and per probe: the data-free form of the same launch
ngal, dngal, fisher = joint.fisher_batch(theta[best], precision)
total = fisher[0] + np.outer(dngal[0], dngal[0]) / sigma_ngal**2
errors = np.sqrt(np.diag(np.linalg.inv(total)))
for key, fit, true, error in zip(KEYS, theta[best], truth, errors):
    print('%-11s fit %9.5f   truth %9.5f   forecast 1 sigma %8.5f' % (key, fit, true, error))
assert chi2[best] < 1e-6, 'none of the searches converged'
assert np.all(np.abs(theta[best] - truth) < 1e-3 * errors), 'the best search missed the truth'
