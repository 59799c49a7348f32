"""The ensemble MCMC of example_mcmc.py on the data vector the reference's author fits: w_p and
DeltaSigma of one halo table (docs/guides/overview.rst:86-92), with a covariance that couples the
two probes.  All walkers of a half-step are ONE batch and one kernel launch:
`JointLikelihood.chi2_batch(theta, data, precision)` evaluates the occupations once per walker,
both tables' predictions and chi2 against the full (N, N) precision matrix, and returns
`(ngal, chi2)` per walker.

    python examples/example_joint_mcmc.py tests/golden/bolplanck_wp.hdf5 \
        tests/golden/bolplanck_ds.hdf5

A plain affine-invariant stretch move (Goodman & Weare 2010) in NumPy, as in example_mcmc.py.
Under `torchrun --nproc-per-node N`, `tabcorr_amd.parallel.chi2_batch_sharded(joint, ...)` calls
the same method on every rank's share of the walkers.
"""

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tabcorr_amd import JointLikelihood, TabCorr  # noqa: E402

names = sys.argv[1:3] if len(sys.argv) > 2 else ['tests/golden/bolplanck_wp.hdf5',
                                                 'tests/golden/bolplanck_ds.hdf5']
joint = JointLikelihood([TabCorr.read(name) for name in names])
rng = np.random.default_rng(0)

# mock data: the prediction of a fiducial model with 5 % errors that are correlated between
# neighbouring bins and, bin by bin, between the two probes
truth = np.array([12.1, 0.3, 11.8, 13.2, 1.05])      # logMmin, sigma_logM, logM0, logM1, alpha
ngal_true, xis_true = joint.predict_batch(truth[np.newaxis])
xi_true = np.concatenate([np.ravel(xi[0]) for xi in xis_true])
n = joint.n_r_total
sigma = 0.05 * np.abs(xi_true)
index = np.concatenate([np.arange(part.stop - part.start) for part in joint.slices])
probe = np.concatenate([np.full(part.stop - part.start, k) for k, part in enumerate(joint.slices)])
same_probe = probe[:, np.newaxis] == probe[np.newaxis, :]
distance = np.abs(index[:, np.newaxis] - index[np.newaxis, :])
correlation = np.where(same_probe, 0.4**distance, 0.3 * 0.4**distance)
covariance = correlation * sigma[:, np.newaxis] * sigma[np.newaxis, :]
data = xi_true + np.linalg.cholesky(covariance) @ rng.normal(size=n)
precision = np.linalg.inv(covariance)
first = joint.slices[0].stop
assert np.any(precision[:first, first:] != 0.0)      # the probes are coupled
low = np.array([11.0, 0.05, 10.5, 12.0, 0.5])
high = np.array([13.5, 1.0, 13.0, 14.5, 1.6])


def log_probability(theta):
    """All walkers at once: one call into the library, one launch, per half-step."""
    inside = np.all((theta >= low) & (theta <= high), axis=1)
    ngal, chi2 = joint.chi2_batch(np.clip(theta, low, high), data, precision)
    chi2 = chi2 + ((ngal - ngal_true[0]) / (0.05 * ngal_true[0]))**2
    return np.where(inside & np.isfinite(chi2), -0.5 * chi2, -np.inf)


n_walkers, n_steps = 2048, 200
walkers = truth + 0.02 * rng.normal(size=(n_walkers, 5))
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
        accept = np.log(rng.uniform(size=len(mine))) < 4 * np.log(z) + logp_new - logp[mine]
        walkers[mine[accept]] = proposal[accept]
        logp[mine[accept]] = logp_new[accept]
        n_accepted += int(accept.sum())
elapsed = time.perf_counter() - start
print('%d walkers x %d steps = %d joint likelihood evaluations (N = %d) in %.2f s (%.3g per '
      'second), acceptance %.2f' % (n_walkers, n_steps, n_walkers * n_steps, n, elapsed,
                                    n_walkers * n_steps / elapsed,
                                    n_accepted / (n_walkers * n_steps)))
for name, mean, std, true in zip(('logMmin', 'sigma_logM', 'logM0', 'logM1', 'alpha'),
                                 walkers.mean(axis=0), walkers.std(axis=0), truth):
    print('%-10s %.3f +- %.3f   (truth %.3f)' % (name, mean, std, true))
