"""A hand-written HOD fitted THROUGH AN INTERPOLATOR by gradient descent over (theta, x): the
occupation seam of `Interpolator`, for a model that is none of the device families.

    d chi2 / d theta_k = sum_v sum_i (d chi2 / d n_vi) (d n_vi / d theta_k),   d chi2 / d x_d

``Interpolator.chi2_grad_occupation`` gives chi2 of the interpolated prediction, d chi2 / d n for
every class of halo tables and d chi2 / d x in ONE kernel launch for all the tables of the grid;
the model's own d n / d theta -- here by central differences of `Interpolator.mean_occupation`,
which evaluates the Python callbacks on the host -- is ``n_bins`` smooth numbers per parameter and
class, and the chain rule is a matrix product on the host.  NumPy only.

    python examples/example_interp_custom_model_grad.py tests/golden/ds_efficient.hdf5
"""

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tabcorr_amd import Interpolator  # noqa: E402

erf = np.vectorize(math.erf, otypes=[np.float64])
KEYS = ('logMmin', 'sigma', 'logM1', 'alpha')


class PowerLawHOD:
    """A smooth step of centrals and a pure power law of satellites: four parameters, no cut-off
    mass -- not Zheng07, not Leauthaud11.  The callbacks have the signature of
    ``tabcorr/tabcorr.py:556-563``."""

    def __init__(self, theta):
        self.theta = np.asarray(theta, dtype=np.float64)

    def mean_occupation_centrals(self, prim_haloprop, **kwargs):
        log_m_min, sigma = self.theta[:2]
        return 0.5 * (1.0 + erf((np.log10(prim_haloprop) - log_m_min) / sigma))

    def mean_occupation_satellites(self, prim_haloprop, **kwargs):
        log_m1, alpha = self.theta[2:]
        return (np.asarray(prim_haloprop) / 10.0**log_m1)**alpha


name = sys.argv[1] if len(sys.argv) > 1 else 'tests/golden/ds_efficient.hdf5'
interp = Interpolator.read(name)
n_dim = len(interp.keys)
low = np.array([xp[0] for xp in interp.xp])
high = np.array([xp[-1] for xp in interp.xp])


def occupation_of(theta):
    """(C, n_bins): the model's mean occupations for every class of halo tables, on the host."""
    return interp.mean_occupation(PowerLawHOD(theta), check_consistency=False)


# the data: the prediction of a known (theta, x) with 5 per cent errors
truth_theta = np.array([12.9, 0.4, 14.0, 1.0])
truth_x = low + 0.6 * (high - low)
_, xi = interp.predict_occupation(occupation_of(truth_theta)[np.newaxis], truth_x[np.newaxis])
data = xi[0]
precision = np.diag(1.0 / (0.05 * np.abs(np.ravel(data)))**2)


def chi2_and_gradient(theta, x):
    """chi2 and its gradient over (theta, x): 2 x 4 host evaluations of the occupations, ONE
    launch, one matrix product."""
    h = 1e-4 * np.maximum(np.abs(theta), 1.0)
    dn_dtheta = np.array([(occupation_of(theta + step) - occupation_of(theta - step)) / (2 * size)
                          for step, size in zip(np.diag(h), h)])       # (4, C, n_bins)
    _, chi2, dchi2_dn, dchi2_dx, _ = interp.chi2_grad_occupation(
        occupation_of(theta)[np.newaxis], x[np.newaxis], data, precision)
    return chi2[0], np.concatenate([np.tensordot(dn_dtheta, dchi2_dn[0], 2), dchi2_dx[0]])


def chi2_of(theta, x):
    return interp.chi2_occupation(occupation_of(theta)[np.newaxis], x[np.newaxis], data,
                                  precision)[1][0]


theta = truth_theta + np.array([0.08, 0.05, -0.1, 0.06])
x = low + 0.45 * (high - low)

# the gradient next to central differences of chi2 itself
chi2, gradient = chi2_and_gradient(theta, x)
steps = 1e-5 * np.maximum(np.abs(np.concatenate([theta, x])), 1.0)
differences = []
for k, step in enumerate(steps):
    shift = np.zeros(len(steps))
    shift[k] = step
    differences.append((chi2_of(theta + shift[:4], x + shift[4:]) -
                        chi2_of(theta - shift[:4], x - shift[4:])) / (2 * step))
print('chi2 = %.6f at the start' % chi2)
print('%-14s %16s %16s %10s' % ('parameter', 'through the seam', 'differences', 'rel. diff'))
for key, seam, diff in zip(KEYS + tuple(interp.keys), gradient, differences):
    print('%-14s %16.8e %16.8e %10.1e' % (key, seam, diff,
                                          abs(seam - diff) / max(abs(diff), 1e-300)))
assert np.allclose(gradient, differences, rtol=1e-3,
                   atol=1e-5 * np.max(np.abs(differences))), 'the two gradients disagree'

# gradient descent with a backtracking step, every parameter in units of its own scale; x stays
# inside the grid
scale = np.concatenate([np.array([0.1, 0.1, 0.1, 0.1]), high - low])
start, rate = chi2, 1.0
for iteration in range(40):
    direction = -gradient * scale**2
    while rate > 1e-12:
        trial = np.concatenate([theta, x]) + rate * direction / np.linalg.norm(gradient * scale)
        trial[4:] = np.clip(trial[4:], low, high)
        trial_chi2 = chi2_of(trial[:4], trial[4:])
        if trial_chi2 < chi2:
            break
        rate *= 0.5
    else:
        break
    theta, x = trial[:4], trial[4:]
    chi2, gradient = chi2_and_gradient(theta, x)
    rate *= 2.0
    if iteration % 5 == 0:
        print('iteration %2d  chi2 = %12.6f  theta = %s  x = %s' % (iteration, chi2, theta, x))
print('chi2 = %.6f after the descent (%.6f at the start)' % (chi2, start))
print('theta = %s (truth %s)' % (theta, truth_theta))
print('x     = %s (truth %s)' % (x, truth_x))
assert chi2 < 0.1 * start, 'the descent did not reduce chi2'
