"""Reference of a joint of interpolators built over one grid: the per-member references
(`interp_grad_reference.jacobian_batch`, `assembias_grad_reference.interp_jacobian_batch`)
concatenated along r in member order, and chi2, its gradient and the Fisher matrix of the joint
data vector over the 5 + D columns (theta, x) by the formulas and allowances of
`joint_reference.chi2_reference` and `fisher_reference`.  A helper of the joint-interpolator tests,
not a test module.

No new tolerance: everything is RTOL = 1e-10 relative plus 1e-10 of the scale of the terms that
cancel, each row with the scale of ITS member.
"""

import numpy as np

import assembias_grad_reference
import fisher_reference
import interp_grad_reference
import joint_reference
from oracle import tabcorr_oracle as oracle
from tabcorr_amd import synthetic

RTOL = joint_reference.RTOL


def make_members(grid, n_prim, n_sec, parts, classes='one', seed=40, assembias=False):
    """The members of a synthetic joint: `parts` = [(mode, tpcf_shape), ...], every member from
    synthetic_interpolator(grid, n_prim, n_sec, tpcf_shape, mode, seed) -- one seed, so that the
    members share their gal_type table -- as (tables, keys, points).  classes: 'one', or 'two'
    (every other GRID NODE in list order has another n_h, in every member alike).  assembias: a bin
    at the split sits at percentile 0.5 exactly (assembias_grad_reference.synthetic_table)."""
    members = []
    for mode, shape in parts:
        tables, keys, points = synthetic.synthetic_interpolator(grid, n_prim, n_sec, tuple(shape),
                                                                mode, seed=seed)
        for k, table in enumerate(tables):
            table['gal_type'] = table['gal_type'].copy()
            if classes == 'two':
                table['gal_type']['n_h'] *= 1.0 + 0.2 * (k % 2)
            if assembias:
                percentile = table['gal_type']['sec_haloprop_percentile']
                percentile[np.abs(percentile - 0.5) < 1e-9] = 0.5
        members.append((tables, keys, points))
    for tables, keys, points in members[1:]:
        assert keys == members[0][1] and np.array_equal(points, members[0][2])
        for mine, theirs in zip(tables, members[0][0]):
            assert mine['gal_type'].tobytes() == theirs['gal_type'].tobytes()
    return members


def permuted(member, order):
    tables, keys, points = member
    return [tables[k] for k in order], keys, points[order]


def jacobian_batch(members, theta, x, n_gauss_prim=10, modulate=False, assembias=False,
                   shared=True):
    """The dict of `interp_grad_reference.jacobian_batch` with the members' r bins flattened and
    concatenated: ngal (n), xi (n, N), dngal (n, Q), dxi (n, Q, N) and their `*_scale`.  shared:
    assert that the members' ngal and dngal agree (not under
    `assembias_grad_reference.rounding_of_centrals`, which moves every evaluation at random)."""
    parts = []
    for tables, _, points in members:
        setup = oracle.interpolator_setup(tables, points)
        if assembias:
            parts.append(assembias_grad_reference.interp_jacobian_batch(
                tables, setup, points, theta, x, n_gauss_prim, modulate))
        else:
            parts.append(interp_grad_reference.jacobian_batch(
                tables, setup, points, theta, x, n_gauss_prim, modulate))
    n = len(np.atleast_2d(theta))
    for part in parts[1:] if shared else []:
        # one grid of halo tables: the members' ngal and dngal are the same numbers
        for name in ('ngal', 'dngal', 'ngal_scale', 'dngal_scale'):
            assert np.array_equal(part[name], parts[0][name], equal_nan=True), name
    out = {name: parts[0][name] for name in ('ngal', 'dngal', 'ngal_scale', 'dngal_scale')}
    for name in ('xi', 'xi_scale'):
        out[name] = np.concatenate([part[name].reshape(n, -1) for part in parts], axis=1)
    for name in ('dxi', 'dxi_scale'):
        out[name] = np.concatenate([fisher_reference.flatten(part[name]) for part in parts],
                                   axis=2)
    return out


def usable(reference):
    return interp_grad_reference.usable(reference)


def first(reference, n):
    return interp_grad_reference.first(reference, n)


def flat(got, n_r_total):
    """(ngal, xis, dngal, dxis) of `JointInterpolator.predict_batch_grad` on the joint axis."""
    ngal, xis, dngal, dxis = got
    n, n_cols = dngal.shape
    xi = np.concatenate([part.reshape(n, -1) for part in xis], axis=1)
    dxi = np.concatenate([part.reshape(n, n_cols, -1) for part in dxis], axis=2)
    assert xi.shape == (n, n_r_total) and dxi.shape == (n, n_cols, n_r_total)
    return ngal, xi, dngal, dxi


def check_prediction(got, reference, what):
    """ngal, xi (n, N), dngal, dxi (n, Q, N) against the first n draws of the reference."""
    return interp_grad_reference.check(got, first(reference, len(got[0])), what)


def as_joint_tuple(reference):
    """The reference as `joint_reference` reads one: (ngal, xi, dngal, dxi, scale)."""
    return (reference['ngal'], reference['xi'], reference['dngal'], reference['dxi'],
            reference['dxi_scale'])


def chi2_reference(reference, data, precision):
    """chi2 (n), dchi2 (n, Q) and their allowances (`joint_reference.chi2_reference`)."""
    return joint_reference.chi2_reference(as_joint_tuple(reference), data, precision)


def check_chi2(got, reference, data, precision, what):
    """ngal, chi2, dngal, dchi2 of a likelihood call against the reference."""
    ngal, chi2, dngal, dchi2 = got[:4]
    n = len(ngal)
    expect = first(reference, n)
    joint_reference.check_chi2(chi2, dchi2, as_joint_tuple(expect), data, precision, what)
    for name, value in (('ngal', ngal), ('dngal', dngal)):
        allowance = RTOL * np.abs(expect[name]) + RTOL * expect[name + '_scale']
        assert np.all(np.abs(value - expect[name]) <= allowance), (what, name)


def check_fisher(fisher, reference, precision, what):
    dxi, a = joint_reference.fisher_jacobian(as_joint_tuple(reference))
    worst, _ = fisher_reference.check(fisher, dxi, a, precision, what)
    assert np.array_equal(fisher, fisher.transpose(0, 2, 1)), what
    return worst
