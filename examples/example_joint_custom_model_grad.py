"""Gradient of the JOINT (w_p, DeltaSigma) chi2 for a family the joint's analytic-gradient calls do
not cover: the eleven parameters of the Leauthaud et al. (2011) occupation, through the occupation
seam of `JointLikelihood`.

    d chi2 / d theta_k = sum_i (d chi2 / d n_i) (d n_i / d theta_k)

``JointLikelihood.chi2_grad_occupation`` gives chi2 of the concatenated data vector against the
full precision matrix -- whose off-diagonal blocks couple the probes -- and d chi2 / d n for ANY
occupation model in ONE kernel launch for both tables; the model's own d n / d theta is ``n_bins``
smooth numbers per parameter, here from 22 cheap ``mean_occupation_batch(...,
family='leauthaud11')`` calls (occupations only, no contraction).  Printed next to central
differences of ``chi2_occupation`` at the same 22 occupations.  NumPy only.

    python examples/example_joint_custom_model_grad.py tests/golden/bolplanck_wp.hdf5 \\
        tests/golden/bolplanck_ds.hdf5
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tabcorr_amd import JointLikelihood, TabCorr, synthetic  # noqa: E402
from tabcorr_amd.models import LEAUTHAUD11_GRAD_KEYS as KEYS  # noqa: E402

N = len(KEYS)
MODULATE = True                          # halotools' default for this family
OCCUPATION = dict(family='leauthaud11', modulate_with_cenocc=MODULATE)

names = sys.argv[1:3] if len(sys.argv) > 2 else ['tests/golden/bolplanck_wp.hdf5',
                                                 'tests/golden/bolplanck_ds.hdf5']
halotab_wp, halotab_ds = (TabCorr.read(name) for name in names)
joint = JointLikelihood([halotab_wp, halotab_ds])

# the data: the prediction of a known parameter vector (threshold, h and h_s, the last three device
# columns, are inputs, not fitted); 5 per cent errors, and the two probes correlated bin by bin
truth = synthetic.LEAUTHAUD11_CENTRE.copy()
_, xis = joint.predict_occupation(halotab_wp.mean_occupation_batch(truth, **OCCUPATION)[0])
data = np.concatenate([np.ravel(xi) for xi in xis])
sigma = 0.05 * np.abs(data)
correlation = np.eye(len(data))
first = joint.slices[0].stop
for r in range(min(first, len(data) - first)):
    correlation[r, first + r] = correlation[first + r, r] = 0.3
precision = np.linalg.inv(correlation * np.outer(sigma, sigma))

theta = truth.copy()
theta[:N] += 0.3 * synthetic.LEAUTHAUD11_WIDTH[:N] * np.cos(np.arange(N))
h = 1e-4 * np.maximum(np.abs(theta[:N]), 1.0)

# 1. d n / d theta_k by central differences of the occupations: 22 occupation-only calls
steps = np.zeros((N, len(theta)))
steps[np.arange(N), np.arange(N)] = h
plus = halotab_wp.mean_occupation_batch(theta + steps, **OCCUPATION)
minus = halotab_wp.mean_occupation_batch(theta - steps, **OCCUPATION)
dn_dtheta = (plus - minus) / (2 * h[:, np.newaxis])    # (11, n_bins)

# 2. ONE call for chi2 of both probes and d chi2 / d n, then a matrix product
occupation = halotab_wp.mean_occupation_batch(theta, **OCCUPATION)[0]
ngal, chi2, dchi2_dn = joint.chi2_grad_occupation(occupation, data, precision)
gradient = dn_dtheta @ dchi2_dn

# 3. central differences of chi2 itself at the same occupations
differences = (joint.chi2_occupation(plus, data, precision)[1] -
               joint.chi2_occupation(minus, data, precision)[1]) / (2 * h)

print('ngal = %.6e   chi2 = %.6f' % (ngal, chi2))
print('%-14s %16s %16s %10s' % ('parameter', 'through the seam', 'differences', 'rel. diff'))
for key, seam, diff in zip(KEYS, gradient, differences):
    print('%-14s %16.8e %16.8e %10.1e' % (key, seam, diff,
                                          abs(seam - diff) / max(abs(diff), 1e-300)))
assert np.allclose(gradient, differences, rtol=1e-4,
                   atol=1e-6 * np.max(np.abs(differences))), 'the two gradients disagree'
