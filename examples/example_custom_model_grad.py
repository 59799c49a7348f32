"""Gradient of chi2 for a model the analytic-gradient calls do not cover: the seven parameters of
the Zheng07 model with assembly bias, through the occupation seam.

    d chi2 / d theta_k = sum_i (d chi2 / d n_i) (d n_i / d theta_k)

``chi2_grad_occupation`` gives d chi2 / d n for ANY occupation model in one kernel launch; the
model's own d n / d theta is ``n_bins`` smooth numbers per parameter -- here from 14 cheap
``mean_occupation_batch`` calls (occupations only, no contraction), for a custom model from its
own derivative or an autodiff framework.  Printed next to central differences of ``chi2_batch``,
which cost 14 full predictions.  NumPy only.

    python examples/example_custom_model_grad.py tests/golden/bolplanck_wp.hdf5
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tabcorr_amd import TabCorr  # noqa: E402

KEYS = ('logMmin', 'sigma_logM', 'logM0', 'logM1', 'alpha', 'A_cen', 'A_sat')

fname = sys.argv[1] if len(sys.argv) > 1 else 'tests/golden/bolplanck_wp.hdf5'
halotab = TabCorr.read(fname)

truth = np.array([12.02, 0.26, 11.38, 13.31, 1.06, 0.3, -0.2])
_, wp_true = halotab.predict_batch(truth, assembias=True)
data = wp_true[0].ravel()
precision = np.diag(1.0 / (0.05 * np.abs(data))**2)    # 5 per cent errors on every bin

theta = np.array([12.10, 0.30, 11.50, 13.40, 1.00, 0.5, -0.4])
h = 1e-4

# 1. d n / d theta_k by central differences of the occupations: 14 occupation-only calls
steps = h * np.eye(len(theta))
plus = halotab.mean_occupation_batch(theta + steps, assembias=True)
minus = halotab.mean_occupation_batch(theta - steps, assembias=True)
dn_dtheta = (plus - minus) / (2 * h)                   # (7, n_bins)

# 2. ONE call for chi2 and d chi2 / d n, then a matrix product
occupation = halotab.mean_occupation_batch(theta, assembias=True)[0]
ngal, chi2, dchi2_dn = halotab.chi2_grad_occupation(occupation, data, precision)
gradient = dn_dtheta @ dchi2_dn

# 3. what a user without the seam pays: 14 full predictions
differences = (halotab.chi2_batch(theta + steps, data, precision, assembias=True)[1] -
               halotab.chi2_batch(theta - steps, data, precision, assembias=True)[1]) / (2 * h)

print('ngal = %.6e   chi2 = %.6f' % (ngal, chi2))
print('%-11s %16s %16s %10s' % ('parameter', 'through the seam', 'differences', 'rel. diff'))
for key, seam, diff in zip(KEYS, gradient, differences):
    print('%-11s %16.8e %16.8e %10.1e' % (key, seam, diff, abs(seam - diff) / max(abs(diff), 1e-300)))
assert np.allclose(gradient, differences, rtol=1e-4,
                   atol=1e-6 * np.max(np.abs(differences))), 'the two gradients disagree'
