"""Best fit by a damped Gauss-Newton search with analytic gradients: (ngal, w_p) of a known
parameter vector are the data, the fit starts elsewhere and finds its way back with one
``predict_batch_grad`` call per step -- the value and the whole Jacobian in one kernel launch
instead of 6 or 11 differenced ``predict_batch`` calls.  NumPy only.

    python examples/example_bestfit.py tests/golden/bolplanck_wp.hdf5
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tabcorr_amd import TabCorr  # noqa: E402

KEYS = ('logMmin', 'sigma_logM', 'logM0', 'logM1', 'alpha')
LOW = np.array([11.0, 0.05, 10.5, 12.0, 0.5])
HIGH = np.array([14.0, 1.0, 13.5, 15.0, 1.6])

fname = sys.argv[1] if len(sys.argv) > 1 else 'tests/golden/bolplanck_wp.hdf5'
halotab = TabCorr.read(fname)

truth = np.array([12.02, 0.26, 11.38, 13.31, 1.06])
ngal_true, wp_true = halotab.predict_batch(truth)
data = np.concatenate([ngal_true, wp_true[0]])
sigma = 0.05 * np.abs(data)                 # 5 per cent errors on ngal and on every w_p bin


def residuals(theta):
    """Residuals in units of the errors and their Jacobian, from ONE gradient call."""
    ngal, wp, dngal, dwp = halotab.predict_batch_grad(theta)
    model = np.concatenate([ngal, wp[0]])
    jacobian = np.vstack([dngal[0], dwp[0].T])          # (1 + n_r, 5)
    return (model - data) / sigma, jacobian / sigma[:, np.newaxis]


theta = np.array([12.4, 0.45, 11.9, 13.6, 0.9])
r, jac = residuals(theta)
chi2 = r @ r
damping = 1e-2
print('start  chi2 = %10.3f  theta =' % chi2, np.round(theta, 4))
for step in range(60):
    # Levenberg-Marquardt: (J^T J + damping diag(J^T J)) delta = -J^T r
    normal = jac.T @ jac
    delta = np.linalg.solve(normal + damping * np.diag(np.diag(normal)), -jac.T @ r)
    trial = np.clip(theta + delta, LOW, HIGH)
    r_trial, jac_trial = residuals(trial)
    chi2_trial = r_trial @ r_trial
    if np.isfinite(chi2_trial) and chi2_trial < chi2:
        improvement = chi2 - chi2_trial
        theta, r, jac, chi2 = trial, r_trial, jac_trial, chi2_trial
        damping = max(damping / 3.0, 1e-9)
        print('step %2d chi2 = %10.3e  theta =' % (step, chi2), np.round(theta, 4))
        if improvement < 1e-12 * max(chi2, 1e-12) or chi2 < 1e-16:
            break
    else:
        damping *= 4.0

print('truth                     theta =', truth)
for key, fit, true in zip(KEYS, theta, truth):
    print('%-11s fit %9.5f   truth %9.5f' % (key, fit, true))
assert chi2 < 1e-6, 'the search did not converge'
