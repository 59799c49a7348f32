"""The ensemble MCMC of example_joint_mcmc.py over a grid of simulations: the walkers move in the
five Zheng07 parameters AND the grid's extra parameters x, against w_p and DeltaSigma with a
covariance that couples the two probes.  Two synthetic interpolators over the same grid (w_p: mode
auto; DeltaSigma: mode cross; one ``gal_type`` table) stand for the reference's ``wp`` / ``ds``
pair.  All walkers of a half-step are ONE batch and one kernel launch:
`JointInterpolator.chi2_batch(theta, x, data, precision)` evaluates the occupations of every class
of halo tables once per walker, both members' predictions at every grid node and chi2 against the
full (N, N) precision matrix, and returns `(ngal, chi2)` per walker -- no derivative is computed
for a sampler that would throw it away.

    python examples/example_joint_interp_mcmc.py [--walkers 512] [--steps 100] [--n-prim 12]

A plain affine-invariant stretch move (Goodman & Weare 2010) in NumPy, as in example_mcmc.py.
"""

import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, REPO)
from tabcorr_amd import Interpolator, JointInterpolator, TabCorr, synthetic  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('--walkers', type=int, default=512)
parser.add_argument('--steps', type=int, default=100)
parser.add_argument('--n-prim', type=int, default=12, help='mass bins per galaxy type')
args = parser.parse_args()


def make_interpolator(mode, tpcf_shape):
    """One member: a grid of four synthetic tables; the same seed gives every member the same
    gal_type table."""
    tables, keys, points = synthetic.synthetic_interpolator((4, ), args.n_prim, 1, tpcf_shape,
                                                            mode, seed=40)
    halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
                for t in tables]
    return Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)})


joint = JointInterpolator([make_interpolator('auto', (7, )), make_interpolator('cross', (7, ))])
n, n_wp = joint.n_r_total, joint.slices[0].stop
n_dim = len(joint.keys)
keys = ('logMmin', 'sigma_logM', 'logM0', 'logM1', 'alpha') + tuple(joint.keys)
x_low = np.array([xp[0] for xp in joint.interpolators[0].xp])
x_high = np.array([xp[-1] for xp in joint.interpolators[0].xp])
rng = np.random.default_rng(0)

# mock data: the prediction of a fiducial (theta, x) with 5 % errors that are correlated between
# neighbouring bins and, bin by bin, between the two probes
truth = np.concatenate([[12.02, 0.26, 11.38, 13.31, 1.06], x_low + 0.37 * (x_high - x_low)])
ngal_true, xis_true = joint.predict_batch(truth[np.newaxis, :5], truth[np.newaxis, 5:])
xi_true = np.concatenate([np.ravel(xi[0]) for xi in xis_true])
sigma = 0.05 * np.abs(xi_true)
index = np.arange(n)
radius = np.where(index < n_wp, index, index - n_wp)
same_probe = (index[:, np.newaxis] < n_wp) == (index[np.newaxis, :] < n_wp)
distance = np.abs(radius[:, np.newaxis] - radius[np.newaxis, :])
correlation = np.where(same_probe, 0.4**distance, 0.3 * 0.4**distance)
covariance = correlation * sigma[:, np.newaxis] * sigma[np.newaxis, :]
data = xi_true + np.linalg.cholesky(covariance) @ rng.normal(size=n)
precision = np.linalg.inv(covariance)
assert np.any(precision[:n_wp, n_wp:] != 0.0)        # the probes are coupled
low = np.concatenate([truth[:5] - [0.4, 0.15, 0.5, 0.4, 0.3], x_low])
high = np.concatenate([truth[:5] + [0.4, 0.3, 0.5, 0.4, 0.3], x_high])


def log_probability(parameters):
    """All walkers at once: one call into the library, one launch, per half-step."""
    inside = np.all((parameters >= low) & (parameters <= high), axis=1)
    clipped = np.clip(parameters, low, high)
    ngal, chi2 = joint.chi2_batch(clipped[:, :5], clipped[:, 5:], data, precision)
    chi2 = chi2 + ((ngal - ngal_true[0]) / (0.05 * ngal_true[0]))**2
    return np.where(inside & np.isfinite(chi2), -0.5 * chi2, -np.inf)


n_walkers, n_steps = args.walkers, args.steps
walkers = np.clip(truth + 0.02 * (high - low) * rng.normal(size=(n_walkers, len(keys))), low, high)
logp = log_probability(walkers)
start = time.perf_counter()
n_accepted = 0
for step in range(n_steps):
    for half in (0, 1):                                # update one half against the other
        mine = np.arange(half, n_walkers, 2)
        others = walkers[np.arange(1 - half, n_walkers, 2)]
        z = (1 + rng.uniform(size=len(mine)))**2 / 2   # g(z) ~ 1 / sqrt(z) on [1/2, 2]
        partner = others[rng.integers(0, len(others), len(mine))]
        proposal = partner + z[:, np.newaxis] * (walkers[mine] - partner)
        logp_new = log_probability(proposal)
        accept = (np.log(rng.uniform(size=len(mine))) <
                  (len(keys) - 1) * np.log(z) + logp_new - logp[mine])
        walkers[mine[accept]] = proposal[accept]
        logp[mine[accept]] = logp_new[accept]
        n_accepted += int(accept.sum())
elapsed = time.perf_counter() - start
print('%d walkers x %d steps = %d joint likelihood evaluations (N = %d, %d parameters) in %.2f s '
      '(%.3g per second), acceptance %.2f' % (
          n_walkers, n_steps, n_walkers * n_steps, n, len(keys), elapsed,
          n_walkers * n_steps / max(elapsed, 1e-9), n_accepted / (n_walkers * n_steps)))
for name, mean, std, true in zip(keys, walkers.mean(axis=0), walkers.std(axis=0), truth):
    print('%-11s %.3f +- %.3f   (truth %.3f)' % (name, mean, std, true))
