"""256 Levenberg-Marquardt searches over the SEVEN parameters of Zheng07 decorated with assembly
bias, and a Fisher forecast at the best fit -- examples/example_fisher.py on a synthetic table cut
into two secondary-percentile halves: (ngal, w_p) of a known parameter vector are the data, and
every step of all searches is ONE ``chi2_fisher_batch(..., assembias=True)`` call: chi2, its
gradient and the (7, 7) Gauss-Newton normal matrix of every search from one kernel launch, plus a
batched ``np.linalg.solve``.  NumPy only.

    python examples/example_fisher_assembias.py
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tabcorr_amd import TabCorr, synthetic  # noqa: E402
from tabcorr_amd.models import ZHENG07_ASSEMBIAS_KEYS as KEYS  # noqa: E402

# (the strengths stay inside the clip at +-1, beyond which their derivative is zero)
LOW = np.array([11.0, 0.05, 10.5, 12.0, 0.5, -0.95, -0.95])
HIGH = np.array([14.0, 1.0, 13.5, 15.0, 1.6, 0.95, 0.95])
N_SEARCHES = 256
N = len(KEYS)

table = synthetic.synthetic_table(25, 2, (19, ), 'auto', seed=0)
halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                              table['attrs'])

truth = np.array([12.02, 0.26, 11.38, 13.31, 1.06, 0.4, -0.3])
ngal_true, wp_true = halotab.predict_batch(truth, assembias=True)
ngal_true, wp_true = ngal_true[0], wp_true[0]
sigma_ngal = 0.05 * ngal_true               # 5 per cent errors on ngal and on every w_p bin
precision = np.diag(1.0 / (0.05 * np.abs(wp_true))**2)


def likelihood(theta):
    """chi2, half its gradient and its Gauss-Newton normal matrix for every row of theta, from
    ONE call.  The library's part is the w_p term; the ngal term is added here from dngal: an
    outer product completes the matrix."""
    ngal, chi2, dngal, dchi2, fisher = halotab.chi2_fisher_batch(theta, wp_true, precision,
                                                                 assembias=True)
    pull = (ngal - ngal_true) / sigma_ngal
    slope = dngal / sigma_ngal
    chi2 = chi2 + pull**2
    half_gradient = 0.5 * dchi2 + pull[:, np.newaxis] * slope
    normal = fisher + slope[:, :, np.newaxis] * slope[:, np.newaxis, :]
    # a start without galaxies (or a step into such a place) has no finite likelihood: it counts
    # as infinitely bad and does not move
    bad = ~(np.isfinite(chi2) & np.all(np.isfinite(half_gradient), axis=1) &
            np.all(np.isfinite(normal), axis=(1, 2)))
    chi2[bad], half_gradient[bad], normal[bad] = np.inf, 0.0, np.eye(N)
    return chi2, half_gradient, normal


rng = np.random.default_rng(7)
theta = rng.uniform(LOW, HIGH, size=(N_SEARCHES, N))
chi2, half_gradient, normal = likelihood(theta)
damping = np.full(N_SEARCHES, 1e-2)
print('start   best chi2 = %10.3e  median = %10.3e' % (np.min(chi2), np.median(chi2)))
for step in range(300):
    # Levenberg-Marquardt: (N + damping diag(N)) delta = -grad / 2, for every search at once (a
    # parameter without any effect, logM0 below every halo, keeps a unit diagonal and stays)
    diagonal = np.einsum('nkk->nk', normal)
    diagonal = np.where(diagonal > 0.0, diagonal, 1.0)
    damped = normal + np.einsum('n,nk,kl->nkl', damping, diagonal, np.eye(N))
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

# Fisher forecast at the best fit: the data-free form of the same launch.  2 F is the
# Gauss-Newton Hessian of chi2, so the parameter covariance is F^-1 (with the ngal term added).
ngal, dngal, fisher = halotab.fisher_batch(theta[best], precision, assembias=True)
total = fisher[0] + np.outer(dngal[0], dngal[0]) / sigma_ngal**2
errors = np.sqrt(np.diag(np.linalg.inv(total)))
for key, fit, true, error in zip(KEYS, theta[best], truth, errors):
    print('%-44s fit %9.5f   truth %9.5f   forecast 1 sigma %8.5f' % (key, fit, true, error))
assert chi2[best] < 1e-6, 'none of the searches converged'
assert np.all(np.abs(theta[best] - truth) < 1e-3 * errors), 'the best search missed the truth'
