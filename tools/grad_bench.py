#!/usr/bin/env python3
"""Cost of an analytic-gradient call next to the forward call it replaces several of.

    python tools/grad_bench.py [--draws 10000] [--seconds 1.0] [--notes profiles/grad_notes.md]

BASELINE configs[1] (50 x 2 bins, 19 r values, 10^4 draws, float64) and the shape of the
reference's example table (30 x 2 bins, 19 r values), device-resident and pipelined over the
handle's lanes as bench.py's timed region is: us per tc_predict_zheng07_batch_device call (the
forward path), per tc_predict_grad_zheng07_batch_device call and per
tc_chi2_grad_zheng07_batch_device call, from the same run.  The bar is what a user without
gradients pays: one-sided differences cost 6 forward calls, central ones 11.

The interpolator leg times Interpolator.chi2_grad_batch (host arrays in and out) against what a
user pays today for the same derivatives with respect to (theta, x): 2 (5 + D) calls of
Interpolator.chi2_batch, the forward path, timed in the same run -- on a 5 x 5 grid of 100-bin
tables in mode auto and on the mode-cross shape of the reference's AbacusSummit interpolator (4
tables over one axis, 1104 bins, 13 r values).

The occupation-VJP leg times TabCorr.predict_vjp and TabCorr.chi2_grad_occupation (host arrays
in and out) against predict(ndarray) on the same occupations -- the forward seam they
differentiate -- and against predict_batch_grad, on the two table shapes above.

The Fisher leg (--only fisher; not part of the default run) times chi2_fisher_batch -- chi2, its
gradient and the Fisher matrix of every draw from one launch -- next to chi2_grad_batch and next
to what a user pays for the same matrix without it: predict_batch_grad plus the NumPy einsum over
the Jacobian it brings back (jacobian_route_us).  Host arrays in and out, on the two table shapes
and the two interpolator shapes above and on a mode-cross table with the 148 r bins of the LDS
limit (where the n_r^2 terms of an entry are most); for the tables also the two device-pointer
entries, device-resident and pipelined, where the kernel's own increase shows.

The assembly-bias leg (--only assembias; not part of the default run) times the gradients of the
decorated model, predict_batch_grad(assembias=True) and chi2_grad_batch(assembias=True), on
two-percentile tables of 100 and 60 bins next to the plain predict_batch_grad on the same table
and next to what they replace: 14 calls of predict_batch(assembias=True), the central
differences over seven parameters.  Device-resident and pipelined, as the first leg, and through
the host-array methods.  The expectation is about 8/6 of the plain gradient -- eight quantities
for six in the dot products and the LDS rows, the matrix stream unchanged.

The Leauthaud11 leg (--only leauthaud11; not part of the default run) times the gradients of
that family, predict_batch_grad(family='leauthaud11') and chi2_fisher_batch(...), on BASELINE
configs[1] and on the bolplanck w_p table of tests/golden next to what they replace -- 22 calls
of predict_batch(family='leauthaud11'), the central differences over eleven parameters -- and
next to the Zheng07 gradient on the same table.  Device-resident and pipelined, as the first leg,
with and without modulate_with_cenocc (one Newton solve more per satellite node).  The
expectation is about twice the Zheng07 gradient's matrix work, twelve dot products per row for
six, and node loops that the Newton solves dominate.

Prints one JSON line and, with --notes, appends the figures to that file.  --only vjp, --only
fisher, --only assembias, --only leauthaud11: that leg alone.
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench_legs import Device, sustained, time_calls   # noqa: E402


def measure(name, n_prim, n_sec, n_r, n_draws, seconds):
    from tabcorr_amd import TabCorr, _lib, synthetic
    table = synthetic.synthetic_table(n_prim, n_sec, (n_r, ), 'auto', seed=0)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                  table['attrs'])
    device = halotab.to_device()
    lib, handle = device.lib, device.handle
    memory = Device(lib, _lib)
    theta = synthetic.zheng07_draws(n_draws, seed=1)
    d_theta = memory.upload(theta)
    d_ngal, d_xi = memory.malloc(n_draws), memory.malloc(n_draws * n_r)
    d_dngal, d_dxi = memory.malloc(n_draws * 5), memory.malloc(n_draws * 5 * n_r)
    d_chi2, d_dchi2 = memory.malloc(n_draws), memory.malloc(n_draws * 5)
    rng = np.random.default_rng(3)
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))

    def forward():
        _lib.check(lib.tc_predict_zheng07_batch_device(handle, d_theta, 5, n_draws, 10, 0,
                                                       d_ngal, d_xi))

    def gradient():
        _lib.check(lib.tc_predict_grad_zheng07_batch_device(handle, d_theta, 5, n_draws, 10, 0,
                                                            d_ngal, d_xi, d_dngal, d_dxi))

    def chi2_gradient():
        _lib.check(lib.tc_chi2_grad_zheng07_batch_device(
            handle, d_theta, 5, n_draws, 10, 0, _lib.as_double_p(data),
            _lib.as_double_p(precision), d_ngal, d_chi2, d_dngal, d_dchi2))

    def synchronize():
        _lib.check(lib.tc_table_synchronize(handle))

    try:
        result = {'table': name, 'n_bins': 2 * n_prim * n_sec, 'n_r': n_r, 'n_draws': n_draws}
        # forward, gradient, forward again: the two forward figures bracket the drift of the run
        result['forward_us'] = sustained(forward, synchronize, seconds) * 1e6
        result['grad_us'] = sustained(gradient, synchronize, seconds) * 1e6
        result['chi2_grad_us'] = sustained(chi2_gradient, synchronize, seconds) * 1e6
        result['forward_again_us'] = sustained(forward, synchronize, seconds) * 1e6
        forward_us = 0.5 * (result['forward_us'] + result['forward_again_us'])
        result['grad_over_forward'] = result['grad_us'] / forward_us
        result['chi2_grad_over_forward'] = result['chi2_grad_us'] / forward_us
        workgroups, waves, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        splits = ctypes.c_int()
        gradient()
        synchronize()
        _lib.check(lib.tc_table_last_launch(handle, ctypes.byref(workgroups), ctypes.byref(waves),
                                            ctypes.byref(splits), ctypes.byref(lds)))
        result['grad_workgroups'] = workgroups.value
        result['grad_lds_bytes'] = lds.value
    finally:
        synchronize()
        memory.free_all()
    return result


def measure_assembias(name, n_prim, n_r, n_draws, seconds):
    from tabcorr_amd import TabCorr, _lib, synthetic
    table = synthetic.synthetic_table(n_prim, 2, (n_r, ), 'auto', seed=0)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                  table['attrs'])
    device = halotab.to_device()
    lib, handle = device.lib, device.handle
    memory = Device(lib, _lib)
    rng = np.random.default_rng(3)
    plain = synthetic.zheng07_draws(n_draws, seed=1)
    theta = np.ascontiguousarray(np.hstack([plain, rng.uniform(-1.0, 1.0, (n_draws, 2))]))
    d_theta, d_plain = memory.upload(theta), memory.upload(plain)
    d_ngal, d_xi = memory.malloc(n_draws), memory.malloc(n_draws * n_r)
    d_dngal, d_dxi = memory.malloc(n_draws * 7), memory.malloc(n_draws * 7 * n_r)
    d_chi2, d_dchi2 = memory.malloc(n_draws), memory.malloc(n_draws * 7)
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    operands = (_lib.as_double_p(data), _lib.as_double_p(precision))

    def forward():
        _lib.check(lib.tc_predict_zheng07_batch_device(handle, d_theta, 7, n_draws, 10,
                                                       _lib.FLAG_ASSEMBIAS, d_ngal, d_xi))

    def gradient():
        _lib.check(lib.tc_predict_grad_assembias_batch_device(handle, d_theta, 7, n_draws, 10, 0,
                                                              d_ngal, d_xi, d_dngal, d_dxi))

    def chi2_gradient():
        _lib.check(lib.tc_chi2_grad_assembias_batch_device(
            handle, d_theta, 7, n_draws, 10, 0, *operands, d_ngal, d_chi2, d_dngal, d_dchi2,
            None))

    def plain_gradient():
        _lib.check(lib.tc_predict_grad_zheng07_batch_device(handle, d_plain, 5, n_draws, 10, 0,
                                                            d_ngal, d_xi, d_dngal, d_dxi))

    def synchronize():
        _lib.check(lib.tc_table_synchronize(handle))

    result = {'table': name, 'n_bins': 4 * n_prim, 'n_r': n_r, 'n_draws': n_draws}
    try:
        # forward first and last: the two figures bracket the drift of the run
        for key, call in (('forward_us', forward), ('grad_us', gradient),
                          ('chi2_grad_us', chi2_gradient), ('plain_grad_us', plain_gradient),
                          ('forward_again_us', forward)):
            result[key] = sustained(call, synchronize, seconds) * 1e6
    finally:
        synchronize()
        memory.free_all()
    forward_us = 0.5 * (result['forward_us'] + result['forward_again_us'])
    result['differences_us'] = 14 * forward_us
    result['grad_over_plain_grad'] = result['grad_us'] / result['plain_grad_us']
    result['differences_over_grad'] = result['differences_us'] / result['grad_us']
    # the same through the methods, host arrays in and out
    host = [('host_forward_us', lambda: halotab.predict_batch(theta, assembias=True)),
            ('host_grad_us', lambda: halotab.predict_batch_grad(theta, assembias=True)),
            ('host_chi2_grad_us',
             lambda: halotab.chi2_grad_batch(theta, data, precision, assembias=True)),
            ('host_plain_grad_us', lambda: halotab.predict_batch_grad(plain)),
            ('host_forward_again_us', lambda: halotab.predict_batch(theta, assembias=True))]
    for key, call in host:
        result[key] = time_calls(call, seconds) * 1e6
    result['host_differences_us'] = 7 * (result['host_forward_us'] +
                                         result['host_forward_again_us'])
    return result


def measure_leauthaud11(name, halotab, modulate, n_draws, seconds):
    from tabcorr_amd import _lib, synthetic
    device = halotab.to_device()
    lib, handle = device.lib, device.handle
    n_r = device.n_r
    memory = Device(lib, _lib)
    theta = np.ascontiguousarray(synthetic.leauthaud11_draws(n_draws, seed=1))
    plain = synthetic.zheng07_draws(n_draws, seed=1)
    d_theta, d_plain = memory.upload(theta), memory.upload(plain)
    d_ngal, d_xi = memory.malloc(n_draws), memory.malloc(n_draws * n_r)
    d_dngal, d_dxi = memory.malloc(n_draws * 11), memory.malloc(n_draws * 11 * n_r)
    d_chi2, d_dchi2 = memory.malloc(n_draws), memory.malloc(n_draws * 11)
    d_fisher = memory.malloc(n_draws * 121)
    rng = np.random.default_rng(3)
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    operands = (_lib.as_double_p(data), _lib.as_double_p(precision))
    flags = _lib.FLAG_MODULATE_WITH_CENOCC if modulate else 0

    def forward():
        _lib.check(lib.tc_predict_zheng07_batch_device(
            handle, d_theta, 14, n_draws, 10, flags | _lib.FLAG_LEAUTHAUD11, d_ngal, d_xi))

    def gradient():
        _lib.check(lib.tc_predict_grad_leauthaud11_batch_device(
            handle, d_theta, 14, n_draws, 10, flags, d_ngal, d_xi, d_dngal, d_dxi))

    def chi2_fisher():
        _lib.check(lib.tc_chi2_grad_leauthaud11_batch_device(
            handle, d_theta, 14, n_draws, 10, flags, *operands, d_ngal, d_chi2, d_dngal, d_dchi2,
            d_fisher))

    def zheng07_gradient():
        _lib.check(lib.tc_predict_grad_zheng07_batch_device(handle, d_plain, 5, n_draws, 10,
                                                            flags, d_ngal, d_xi, d_dngal, d_dxi))

    def synchronize():
        _lib.check(lib.tc_table_synchronize(handle))

    result = {'table': name, 'n_bins': len(halotab.gal_type), 'n_r': n_r, 'n_draws': n_draws,
              'modulate': bool(modulate)}
    try:
        # forward first and last: the two figures bracket the drift of the run
        for key, call in (('forward_us', forward), ('grad_us', gradient),
                          ('chi2_fisher_us', chi2_fisher), ('zheng07_grad_us', zheng07_gradient),
                          ('forward_again_us', forward)):
            result[key] = sustained(call, synchronize, seconds) * 1e6
        # the gradient kernel alone, from the launches' own events
        milliseconds, mean, count = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
        _lib.check(lib.tc_table_timer_begin(handle, 1))
        gradient()
        synchronize()
        _lib.check(lib.tc_table_timer_end(handle, ctypes.byref(milliseconds)))
        _lib.check(lib.tc_table_kernel_time(handle, ctypes.byref(count), ctypes.byref(mean)))
        result['grad_kernel_us'] = count.value * mean.value * 1e3
        workgroups, waves, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        splits = ctypes.c_int()
        _lib.check(lib.tc_table_last_launch(handle, ctypes.byref(workgroups), ctypes.byref(waves),
                                            ctypes.byref(splits), ctypes.byref(lds)))
        result['grad_lds_bytes'] = lds.value
    finally:
        synchronize()
        memory.free_all()
    forward_us = 0.5 * (result['forward_us'] + result['forward_again_us'])
    result['differences_us'] = 22 * forward_us
    result['differences_over_grad'] = result['differences_us'] / result['grad_us']
    result['differences_over_chi2_fisher'] = result['differences_us'] / result['chi2_fisher_us']
    result['grad_over_zheng07_grad'] = result['grad_us'] / result['zheng07_grad_us']
    return result


def write_leauthaud11_notes(notes, results, n_draws):
    notes.write('\n## tools/grad_bench.py --only leauthaud11, %d draws per call\n\n' % n_draws)
    notes.write('Device-resident, pipelined, us per call.\n\n')
    notes.write('| table | bins | modulate | forward(leauthaud11) us | gradient us (kernel alone) | '
                'chi2 + Fisher us | 22 forward calls us | Zheng07 gradient us | '
                '22 forward / gradient | 22 forward / chi2 + Fisher | gradient / Zheng07 gradient '
                '| LDS bytes |\n')
    notes.write('|---|---|---|---|---|---|---|---|---|---|---|---|\n')
    for r in results:
        notes.write('| %s | %d | %s | %.1f, %.1f after | %.1f (%.1f) | %.1f | %.1f | %.1f | %.2f | '
                    '%.2f | %.2f | %d |\n' % (
                        r['table'], r['n_bins'], 'yes' if r['modulate'] else 'no',
                        r['forward_us'], r['forward_again_us'], r['grad_us'], r['grad_kernel_us'],
                        r['chi2_fisher_us'], r['differences_us'], r['zheng07_grad_us'],
                        r['differences_over_grad'], r['differences_over_chi2_fisher'],
                        r['grad_over_zheng07_grad'], r['grad_lds_bytes']))


def write_assembias_notes(notes, results, n_draws):
    notes.write('\n## tools/grad_bench.py --only assembias, %d draws per call\n\n' % n_draws)
    notes.write('Device-resident, pipelined (host arrays in and out in brackets), us per call; '
                'expectation: decorated / plain gradient about 8/6 = 1.33.\n\n')
    notes.write('| table | bins | forward(assembias) us | gradient(assembias) us | '
                'chi2 gradient(assembias) us | plain gradient us | 14 forward calls us | '
                'decorated / plain gradient | 14 forward / gradient |\n')
    notes.write('|---|---|---|---|---|---|---|---|---|\n')
    for r in results:
        notes.write('| %s | %d | %.1f, %.1f after [%.1f, %.1f after] | %.1f [%.1f] | %.1f [%.1f] '
                    '| %.1f [%.1f] | %.1f [%.1f] | %.3f | %.2f |\n' % (
                        r['table'], r['n_bins'], r['forward_us'], r['forward_again_us'],
                        r['host_forward_us'], r['host_forward_again_us'], r['grad_us'],
                        r['host_grad_us'], r['chi2_grad_us'], r['host_chi2_grad_us'],
                        r['plain_grad_us'], r['host_plain_grad_us'], r['differences_us'],
                        r['host_differences_us'], r['grad_over_plain_grad'],
                        r['differences_over_grad']))


def measure_interpolator(name, grid, n_prim, n_sec, n_r, mode, n_draws, seconds):
    from tabcorr_amd import Interpolator, TabCorr, synthetic
    tables, keys, points = synthetic.synthetic_interpolator(grid, n_prim, n_sec, (n_r, ), mode,
                                                            seed=0)
    interp = Interpolator(
        [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
         for t in tables], {key: points[:, d] for d, key in enumerate(keys)})
    theta = synthetic.zheng07_draws(n_draws, seed=1)
    rng = np.random.default_rng(3)
    x = rng.uniform(points.min(axis=0), points.max(axis=0), size=(n_draws, len(keys)))
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    n_columns = 5 + len(keys)

    def forward():
        interp.chi2_batch(theta, x, data, precision)

    def gradient():
        interp.chi2_grad_batch(theta, x, data, precision)

    result = {'interpolator': name, 'grid': list(grid), 'mode': mode,
              'n_bins': len(tables[0]['gal_type']), 'n_r': n_r, 'n_draws': n_draws,
              'forward_calls_replaced': 2 * n_columns}
    # forward, gradient, forward again: the two forward figures bracket the drift of the run
    result['chi2_us'] = time_calls(forward, seconds) * 1e6
    result['chi2_grad_us'] = time_calls(gradient, seconds) * 1e6
    result['chi2_again_us'] = time_calls(forward, seconds) * 1e6
    forward_us = 0.5 * (result['chi2_us'] + result['chi2_again_us'])
    result['differences_us'] = 2 * n_columns * forward_us
    result['chi2_grad_over_chi2'] = result['chi2_grad_us'] / forward_us
    result['differences_over_chi2_grad'] = result['differences_us'] / result['chi2_grad_us']
    device = interp.to_device()
    gradient()                      # (the launch tc_table_last_launch reports)
    workgroups, waves, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    splits = ctypes.c_int()
    from tabcorr_amd import _lib
    _lib.check(device.lib.tc_table_last_launch(
        device.tables[0].handle, ctypes.byref(workgroups), ctypes.byref(waves),
        ctypes.byref(splits), ctypes.byref(lds)))
    result['chi2_grad_workgroups'] = workgroups.value
    result['chi2_grad_lds_bytes'] = lds.value
    return result


def measure_occupation_vjp(name, n_prim, n_sec, n_r, n_draws, seconds):
    from tabcorr_amd import TabCorr, synthetic
    table = synthetic.synthetic_table(n_prim, n_sec, (n_r, ), 'auto', seed=0)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                  table['attrs'])
    theta = synthetic.zheng07_draws(n_draws, seed=1)
    occupation = halotab.mean_occupation_batch(theta)
    rng = np.random.default_rng(3)
    g_xi, g_ngal = rng.normal(size=(n_draws, n_r)), rng.normal(size=n_draws)
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    calls = [('predict_occupation_us', lambda: halotab.predict(occupation)),
             ('predict_vjp_us', lambda: halotab.predict_vjp(occupation, g_xi, g_ngal)),
             ('chi2_grad_occupation_us',
              lambda: halotab.chi2_grad_occupation(occupation, data, precision)),
             ('predict_batch_grad_us', lambda: halotab.predict_batch_grad(theta)),
             # the forward figure again: the two bracket the drift of the run
             ('predict_occupation_again_us', lambda: halotab.predict(occupation))]
    result = {'table': name, 'n_bins': occupation.shape[1], 'n_r': n_r, 'n_draws': n_draws}
    for key, call in calls:
        result[key] = time_calls(call, seconds) * 1e6
    forward_us = 0.5 * (result['predict_occupation_us'] + result['predict_occupation_again_us'])
    result['vjp_over_forward'] = result['predict_vjp_us'] / forward_us
    result['chi2_grad_over_forward'] = result['chi2_grad_occupation_us'] / forward_us
    result['vjp_over_batch_grad'] = result['predict_vjp_us'] / result['predict_batch_grad_us']
    # the main kernel alone (the forward path: its contraction kernel), from the launches' own
    # events
    from tabcorr_amd import _lib
    device = halotab.to_device()
    for key, call in calls[:3]:
        milliseconds, mean, count = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
        with device.lock:
            _lib.check(device.lib.tc_table_timer_begin(device.handle, 1))
        call()
        with device.lock:
            _lib.check(device.lib.tc_table_timer_end(device.handle, ctypes.byref(milliseconds)))
            _lib.check(device.lib.tc_table_kernel_time(device.handle, ctypes.byref(count),
                                                       ctypes.byref(mean)))
        result[key.replace('_us', '_kernels_us')] = count.value * mean.value * 1e3
    return result


def fisher_calls(target, theta, x, n_r, seconds):
    """The three host-array figures of the Fisher leg for a table (x None) or an interpolator."""
    rng = np.random.default_rng(3)
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    p_sym = 0.5 * (precision + precision.T)
    draws = (theta, ) if x is None else (theta, x)

    def jacobian_route():
        dxi = target.predict_batch_grad(*draws)[3]
        return np.einsum('nkr,rs,nls->nkl', dxi, p_sym, dxi, optimize=True)

    calls = [('chi2_grad_us', lambda: target.chi2_grad_batch(*draws, data, precision)),
             ('chi2_fisher_us', lambda: target.chi2_fisher_batch(*draws, data, precision)),
             ('jacobian_route_us', jacobian_route),
             # the first figure again: the two bracket the drift of the run
             ('chi2_grad_again_us', lambda: target.chi2_grad_batch(*draws, data, precision))]
    result = {key: time_calls(call, seconds) * 1e6 for key, call in calls}
    # the two routes give the same matrix (to rounding: the orders of the sums differ)
    fisher = target.chi2_fisher_batch(*draws, data, precision)[4]
    expect = jacobian_route()
    finite = np.isfinite(expect) & np.isfinite(fisher)
    result['routes_max_difference'] = float(np.max(
        np.abs(fisher - expect)[finite] / np.max(np.abs(expect[finite]))))
    chi2_grad_us = 0.5 * (result['chi2_grad_us'] + result['chi2_grad_again_us'])
    result['chi2_fisher_over_chi2_grad'] = result['chi2_fisher_us'] / chi2_grad_us
    result['jacobian_route_over_chi2_fisher'] = (result['jacobian_route_us'] /
                                                 result['chi2_fisher_us'])
    return result, data, precision


def measure_fisher(name, n_prim, n_sec, n_r, n_draws, seconds, mode='auto'):
    from tabcorr_amd import TabCorr, _lib, synthetic
    table = synthetic.synthetic_table(n_prim, n_sec, (n_r, ), mode, seed=0)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                  table['attrs'])
    theta = synthetic.zheng07_draws(n_draws, seed=1)
    result = {'table': name, 'n_bins': 2 * n_prim * n_sec, 'n_r': n_r, 'n_draws': n_draws}
    figures, data, precision = fisher_calls(halotab, theta, None, n_r, seconds)
    result.update(figures)
    # the device-pointer entries, device-resident and pipelined over the handle's lanes
    device = halotab.to_device()
    lib, handle = device.lib, device.handle
    memory = Device(lib, _lib)
    d_theta = memory.upload(theta)
    d_ngal, d_chi2 = memory.malloc(n_draws), memory.malloc(n_draws)
    d_dngal, d_dchi2 = memory.malloc(n_draws * 5), memory.malloc(n_draws * 5)
    d_fisher = memory.malloc(n_draws * 25)
    operands = (_lib.as_double_p(data), _lib.as_double_p(precision))

    def chi2_gradient():
        _lib.check(lib.tc_chi2_grad_zheng07_batch_device(
            handle, d_theta, 5, n_draws, 10, 0, *operands, d_ngal, d_chi2, d_dngal, d_dchi2))

    def chi2_fisher():
        _lib.check(lib.tc_chi2_fisher_zheng07_batch_device(
            handle, d_theta, 5, n_draws, 10, 0, *operands, d_ngal, d_chi2, d_dngal, d_dchi2,
            d_fisher))

    def synchronize():
        _lib.check(lib.tc_table_synchronize(handle))

    try:
        result['chi2_grad_device_us'] = sustained(chi2_gradient, synchronize, seconds) * 1e6
        result['chi2_fisher_device_us'] = sustained(chi2_fisher, synchronize, seconds) * 1e6
        result['chi2_grad_device_again_us'] = sustained(chi2_gradient, synchronize, seconds) * 1e6
        result['chi2_fisher_over_chi2_grad_device'] = result['chi2_fisher_device_us'] / (
            0.5 * (result['chi2_grad_device_us'] + result['chi2_grad_device_again_us']))
    finally:
        synchronize()
        memory.free_all()
    return result


def measure_fisher_interpolator(name, grid, n_prim, n_sec, n_r, mode, n_draws, seconds):
    from tabcorr_amd import Interpolator, TabCorr, synthetic
    tables, keys, points = synthetic.synthetic_interpolator(grid, n_prim, n_sec, (n_r, ), mode,
                                                            seed=0)
    interp = Interpolator(
        [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
         for t in tables], {key: points[:, d] for d, key in enumerate(keys)})
    theta = synthetic.zheng07_draws(n_draws, seed=1)
    x = np.random.default_rng(3).uniform(points.min(axis=0), points.max(axis=0),
                                         size=(n_draws, len(keys)))
    result = {'interpolator': name, 'grid': list(grid), 'mode': mode,
              'n_bins': len(tables[0]['gal_type']), 'n_r': n_r, 'n_draws': n_draws,
              'n_columns': 5 + len(keys)}
    result.update(fisher_calls(interp, theta, x, n_r, seconds)[0])
    return result


def write_fisher_notes(notes, tables, interpolators, n_draws):
    notes.write('\n## tools/grad_bench.py --only fisher, %d draws per call, host arrays in and '
                'out\n\n' % n_draws)
    notes.write('| shape | bins | Q | chi2_grad us | chi2_fisher us | jacobian route us | '
                'chi2_fisher / chi2_grad | jacobian route / chi2_fisher | '
                'device-pointer entries: chi2_grad, chi2_fisher us (ratio) |\n')
    notes.write('|---|---|---|---|---|---|---|---|---|\n')
    for r in tables + interpolators:
        device = '-'
        if 'chi2_fisher_device_us' in r:
            device = '%.1f (%.1f after), %.1f (%.3f)' % (
                r['chi2_grad_device_us'], r['chi2_grad_device_again_us'],
                r['chi2_fisher_device_us'], r['chi2_fisher_over_chi2_grad_device'])
        notes.write('| %s | %d | %d | %.1f (%.1f after) | %.1f | %.1f | %.3f | %.2f | %s |\n' % (
            r.get('table', r.get('interpolator')), r['n_bins'], r.get('n_columns', 5),
            r['chi2_grad_us'], r['chi2_grad_again_us'], r['chi2_fisher_us'],
            r['jacobian_route_us'], r['chi2_fisher_over_chi2_grad'],
            r['jacobian_route_over_chi2_fisher'], device))


def write_vjp_notes(notes, results, n_draws):
    notes.write('\n## tools/grad_bench.py, occupation VJP, %d draws per call, host arrays in '
                'and out\n\n' % n_draws)
    notes.write('| table | bins | predict(ndarray) us | predict_vjp us | chi2_grad_occupation us | '
                'predict_batch_grad us | VJP / forward | chi2 gradient / forward | '
                'main kernel alone: forward, VJP, chi2 gradient us |\n')
    notes.write('|---|---|---|---|---|---|---|---|---|\n')
    for r in results:
        notes.write('| %s | %d | %.1f (%.1f after) | %.1f | %.1f | %.1f | %.2f | %.2f | '
                    '%.1f, %.1f, %.1f |\n' % (
                        r['table'], r['n_bins'], r['predict_occupation_us'],
                        r['predict_occupation_again_us'], r['predict_vjp_us'],
                        r['chi2_grad_occupation_us'], r['predict_batch_grad_us'],
                        r['vjp_over_forward'], r['chi2_grad_over_forward'],
                        r['predict_occupation_kernels_us'], r['predict_vjp_kernels_us'],
                        r['chi2_grad_occupation_kernels_us']))


def main():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--draws', type=int, default=10000)
    parser.add_argument('--seconds', type=float, default=1.0)
    parser.add_argument('--notes', default=None, help='append the figures to this file')
    parser.add_argument('--only', choices=['vjp', 'fisher', 'assembias', 'leauthaud11'],
                        default=None,
                        help='one leg alone')
    args = parser.parse_args()
    if args.only == 'leauthaud11':
        from tabcorr_amd import TabCorr, synthetic
        table = synthetic.synthetic_table(50, 1, (19, ), 'auto', seed=0)
        tables = [('BASELINE configs[1]',
                   TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                       table['tpcf_shape'], table['attrs'])),
                  ('bolplanck w_p table',
                   TabCorr.read(os.path.join(REPO, 'tests', 'golden', 'bolplanck_wp.hdf5')))]
        results = [measure_leauthaud11(name, halotab, modulate, args.draws, args.seconds)
                   for name, halotab in tables for modulate in (False, True)]
        print(json.dumps({'leauthaud11_metric': 'us per call, device-resident, pipelined',
                          'leauthaud11': results}))
        if args.notes:
            with open(args.notes, 'a') as notes:
                write_leauthaud11_notes(notes, results, args.draws)
        return
    if args.only == 'assembias':
        results = [measure_assembias('two percentiles, 100 bins', 25, 19, args.draws,
                                     args.seconds),
                   measure_assembias('two percentiles, 60 bins', 15, 19, args.draws,
                                     args.seconds)]
        print(json.dumps({'assembias_metric': 'us per call, device-resident, pipelined; host_*: '
                                              'host arrays in and out',
                          'assembias': results}))
        if args.notes:
            with open(args.notes, 'a') as notes:
                write_assembias_notes(notes, results, args.draws)
        return
    if args.only == 'fisher':
        tables = [measure_fisher('BASELINE configs[1]', 50, 1, 19, args.draws, args.seconds),
                  measure_fisher("reference example table's shape", 30, 1, 19, args.draws,
                                 args.seconds),
                  # where the n_r^2 terms of an entry are most: the r bins of the LDS limit
                  measure_fisher('mode cross, 148 r bins (the LDS limit)', 9, 2, 148, args.draws,
                                 args.seconds, mode='cross')]
        interpolators = [
            measure_fisher_interpolator('5 x 5 grid of 100-bin tables', (5, 5), 50, 1, 19, 'auto',
                                        args.draws, args.seconds),
            measure_fisher_interpolator("AbacusSummit interpolator's shape", (4, ), 276, 2, 13,
                                        'cross', args.draws, args.seconds)]
        print(json.dumps({'fisher_metric': 'us per call, host arrays in and out; *_device_us: '
                                           'device-resident, pipelined',
                          'fisher_tables': tables, 'fisher_interpolators': interpolators}))
        if args.notes:
            with open(args.notes, 'a') as notes:
                write_fisher_notes(notes, tables, interpolators, args.draws)
        return
    vjp = [measure_occupation_vjp('BASELINE configs[1]', 50, 1, 19, args.draws, args.seconds),
           measure_occupation_vjp("reference example table's shape", 30, 1, 19, args.draws,
                                  args.seconds)]
    if args.only == 'vjp':
        print(json.dumps({'occupation_vjp_metric': 'us per call, host arrays in and out',
                          'occupation_vjp': vjp}))
        if args.notes:
            with open(args.notes, 'a') as notes:
                write_vjp_notes(notes, vjp, args.draws)
        return
    results = [measure('BASELINE configs[1]', 50, 1, 19, args.draws, args.seconds),
               measure("reference example table's shape", 30, 1, 19, args.draws, args.seconds)]
    interpolators = [
        measure_interpolator('5 x 5 grid of 100-bin tables', (5, 5), 50, 1, 19, 'auto', args.draws,
                             args.seconds),
        measure_interpolator("AbacusSummit interpolator's shape", (4, ), 276, 2, 13, 'cross',
                             args.draws, args.seconds)]
    print(json.dumps({'metric': 'us per call, device-resident, pipelined', 'results': results,
                      'interpolator_metric': 'us per call, host arrays in and out',
                      'interpolators': interpolators,
                      'occupation_vjp_metric': 'us per call, host arrays in and out',
                      'occupation_vjp': vjp}))
    if args.notes:
        with open(args.notes, 'a') as notes:
            notes.write('\n## tools/grad_bench.py, %d draws per call\n\n' % args.draws)
            notes.write('| table | bins | forward us | gradient us | chi2 gradient us | '
                        'gradient / forward | chi2 gradient / forward |\n')
            notes.write('|---|---|---|---|---|---|---|\n')
            for r in results:
                notes.write('| %s | %d | %.1f (%.1f after) | %.1f | %.1f | %.2f | %.2f |\n' % (
                    r['table'], r['n_bins'], r['forward_us'], r['forward_again_us'],
                    r['grad_us'], r['chi2_grad_us'], r['grad_over_forward'],
                    r['chi2_grad_over_forward']))
            notes.write('\nInterpolator.chi2_grad_batch against 2 (5 + D) calls of '
                        'Interpolator.chi2_batch, host arrays in and out:\n\n')
            notes.write('| interpolator | bins | chi2_batch us | chi2_grad_batch us | '
                        '2 (5 + D) chi2_batch us | gradient / forward | differences / gradient | '
                        'LDS bytes |\n')
            notes.write('|---|---|---|---|---|---|---|---|\n')
            for r in interpolators:
                notes.write('| %s | %d | %.1f (%.1f after) | %.1f | %.1f (%d calls) | %.2f | %.2f '
                            '| %d |\n' % (
                                r['interpolator'], r['n_bins'], r['chi2_us'], r['chi2_again_us'],
                                r['chi2_grad_us'], r['differences_us'],
                                r['forward_calls_replaced'], r['chi2_grad_over_chi2'],
                                r['differences_over_chi2_grad'], r['chi2_grad_lds_bytes']))
            write_vjp_notes(notes, vjp, args.draws)


if __name__ == '__main__':
    main()
