"""64 Levenberg-Marquardt searches over the ELEVEN parameters of the Leauthaud et al. (2011)
occupation AND the extra parameter x of an interpolator -- examples/example_fisher_leauthaud11.py
behind an `Interpolator`: (ngal, w_p) of a known (theta, x) on a small synthetic grid are the data,
and every step of all searches is ONE ``chi2_fisher_batch(..., family='leauthaud11')`` call: chi2,
its gradient and the (12, 12) Gauss-Newton normal matrix over (theta, x) of every search from one
kernel launch, plus a batched ``np.linalg.solve``.  Central differences would cost 24 forward calls
per step.  NumPy only; runs in seconds.

    python examples/example_interp_fisher_leauthaud11.py

w_p and ngal alone do not pin twelve parameters: the searches end in the valley of the likelihood
(chi2 falls by many orders of magnitude), not all at the truth, and the forecast says which
directions the data leave open.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tabcorr_amd import Interpolator, TabCorr, synthetic  # noqa: E402
from tabcorr_amd.models import LEAUTHAUD11_GRAD_KEYS  # noqa: E402

N_SEARCHES = 64
MODULATE = True                          # halotools' default for this family

# a grid of five tables of 2 x 12 mass bins and ten w_p bins along one extra parameter
tables, grid_keys, points = synthetic.synthetic_interpolator((5, ), 12, 1, (10, ), 'auto', seed=3)
interp = Interpolator(
    [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
     for t in tables], {key: points[:, d] for d, key in enumerate(grid_keys)})
KEYS = tuple(LEAUTHAUD11_GRAD_KEYS) + tuple(interp.keys)
N_MODEL, N = len(LEAUTHAUD11_GRAD_KEYS), len(KEYS)

# threshold, h and h_s (the last three device columns) are inputs, not fitted
truth_theta = synthetic.LEAUTHAUD11_CENTRE.copy()
inputs = truth_theta[N_MODEL:]
truth = np.concatenate([truth_theta[:N_MODEL], [0.1]])
LOW = np.concatenate([truth[:N_MODEL] - synthetic.LEAUTHAUD11_WIDTH[:N_MODEL], points.min(axis=0)])
HIGH = np.concatenate([truth[:N_MODEL] + synthetic.LEAUTHAUD11_WIDTH[:N_MODEL], points.max(axis=0)])


def draws(parameters):
    """(theta (n, 14), x (n, 1)) of the rows of `parameters` (n, 12)."""
    parameters = np.atleast_2d(parameters)
    return (np.hstack([parameters[:, :N_MODEL], np.tile(inputs, (len(parameters), 1))]),
            np.ascontiguousarray(parameters[:, N_MODEL:]))


ngal_true, wp_true = interp.predict_batch(*draws(truth), family='leauthaud11',
                                          modulate_with_cenocc=MODULATE)
ngal_true, wp_true = ngal_true[0], wp_true[0]
sigma_ngal = 0.05 * ngal_true               # 5 per cent errors on ngal and on every w_p bin
precision = np.diag(1.0 / (0.05 * np.abs(wp_true))**2)


def likelihood(parameters):
    """chi2, half its gradient and its Gauss-Newton normal matrix for every row of `parameters`,
    from ONE call.  The library's part is the w_p term; the ngal term is added here from dngal: an
    outer product completes the matrix."""
    ngal, chi2, dngal, dchi2, fisher = interp.chi2_fisher_batch(
        *draws(parameters), wp_true, precision, family='leauthaud11',
        modulate_with_cenocc=MODULATE)
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
start = chi2.copy()
damping = np.full(N_SEARCHES, 1e-2)
print('start    best chi2 = %10.3e  median = %10.3e' % (np.min(chi2), np.median(chi2)))
for step in range(200):
    # Levenberg-Marquardt: (N + damping diag(N)) delta = -grad / 2, for every search at once
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
    if step % 20 == 19:
        print('step %3d best chi2 = %10.3e  median = %10.3e  searches below 1e-3: %d' % (
            step + 1, np.min(chi2), np.median(chi2), np.sum(chi2 < 1e-3)))

best = int(np.argmin(chi2))
print('%d of %d searches ended below chi2 = 1e-3 (%d data points); the best one:' % (
    np.sum(chi2 < 1e-3), N_SEARCHES, len(wp_true) + 1))

# Fisher forecast at the truth: the data-free form of the same launch.  2 F is the Gauss-Newton
# Hessian of chi2, so the parameter covariance is F^-1 (with the ngal term added) -- where the data
# pin all twelve directions; the smallest eigenvalues name the ones they leave open.
ngal, dngal, fisher = interp.fisher_batch(*draws(truth), precision, family='leauthaud11',
                                          modulate_with_cenocc=MODULATE)
total = fisher[0] + np.outer(dngal[0], dngal[0]) / sigma_ngal**2
scale = np.sqrt(np.diag(total))
eigenvalues = np.linalg.eigvalsh(total / np.outer(scale, scale))
for key, fit, true, s in zip(KEYS, theta[best], truth, scale):
    print('%-10s fit %9.5f   truth %9.5f   1 sigma with the others fixed %9.5f' % (
        key, fit, true, 1.0 / s))
print('eigenvalues of the scaled normal matrix: %s' % np.array2string(eigenvalues, precision=2))
assert np.all(chi2 <= start), 'a search got worse'
assert chi2[best] < 1e-3, 'none of the searches reached the valley'
