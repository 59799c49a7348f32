"""Time of the interpolator's likelihood-plus-Fisher call of the Leauthaud11 family at 10^4 draws,
device-resident: tc_interp_chi2_grad_leauthaud11_batch_device with the Fisher matrix
(`Interpolator.chi2_fisher_batch(..., family='leauthaud11')`), on tests/golden/ds_efficient.hdf5
(mode cross, K = 4, 1104 bins, 13 r bins) and on a 4 x 4 grid of mode-auto tables (synthetic, 60
bins, 19 r bins).  Next to it what a user could assemble by hand before the call existed: the K
member tables' own tc_chi2_grad_leauthaud11_batch_device launches with their Fisher matrices, one
after the other -- WITHOUT the host combination of the K results over the spline, so the sum
favours that route.  Wall clock around CALLS calls and a synchronize after WARM warm-up calls; the
tables' launches are timed before and after the interpolator's, REPEATS times each: the medians and
the run-to-run spread (max - min).  Prints one JSON line
(profiles/interp_leauthaud11_grad_notes.md).

    python tools/interp_leauthaud11_grad_bench.py [n_draws [auto | cross]]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tabcorr_amd import Interpolator, TabCorr, _lib, synthetic  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
ONLY = sys.argv[2] if len(sys.argv) > 2 else None
CALLS, WARM, REPEATS = 20, 5, 3
N_PARAMS = 11
lib = _lib.load()
rng = np.random.default_rng(3)


def upload(array):
    array = np.ascontiguousarray(array, dtype=np.float64)
    ptr = ctypes.c_void_p()
    _lib.check(lib.tc_device_malloc(ctypes.byref(ptr), max(array.nbytes, 8)))
    _lib.check(lib.tc_memcpy_h2d(ptr, array.ctypes.data_as(ctypes.c_void_p), array.nbytes))
    return ptr


def timed(call, synchronize):
    for _ in range(WARM):
        call()
    synchronize()
    runs = []
    for _ in range(REPEATS):
        start = time.perf_counter()
        for _ in range(CALLS):
            call()
        synchronize()
        runs.append((time.perf_counter() - start) / CALLS * 1e6)
    return {'us_per_call': float(np.median(runs)), 'spread_us': max(runs) - min(runs),
            'runs_us': runs}


def kernel_time(handle, call, synchronize):
    """The launches' own events, through the first table's timer."""
    elapsed, mean, count = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
    _lib.check(lib.tc_table_timer_begin(handle, 1))
    for _ in range(CALLS):
        call()
    synchronize()
    _lib.check(lib.tc_table_timer_end(handle, ctypes.byref(elapsed)))
    _lib.check(lib.tc_table_kernel_time(handle, ctypes.byref(count), ctypes.byref(mean)))
    return {'kernel_us': mean.value * 1e3, 'launches': count.value}


def measure(interp):
    device = interp.to_device()
    n_tables = len(interp.tabcorr_list)
    n_bins = len(interp.tabcorr_list[0].gal_type)
    n_r, n_dim = len(interp.tabcorr_list[0].tpcf_matrix), len(interp.keys)
    n_cols = N_PARAMS + n_dim
    theta = synthetic.leauthaud11_draws(N, seed=5)
    x = np.stack([rng.uniform(xp[0], xp[-1], N) for xp in interp.xp], axis=-1)
    # (the time does not depend on the values of the likelihood's operands)
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    d_theta, d_x = upload(theta), upload(x)
    outputs = [upload(np.zeros(N)), upload(np.zeros(N)), upload(np.zeros((N, n_cols))),
               upload(np.zeros((N, n_cols))), upload(np.zeros((N, n_cols, n_cols)))]

    def one_launch():
        _lib.check(lib.tc_interp_chi2_grad_leauthaud11_batch_device(
            device.handle, d_theta, 14, d_x, N, 10, _lib.FLAG_MODULATE_WITH_CENOCC,
            _lib.as_double_p(data), _lib.as_double_p(precision), *outputs))

    def wait():
        _lib.check(lib.tc_interp_synchronize(device.handle))

    per_table = [[upload(np.zeros(N)), upload(np.zeros(N)), upload(np.zeros((N, N_PARAMS))),
                  upload(np.zeros((N, N_PARAMS))), upload(np.zeros((N, N_PARAMS, N_PARAMS)))]
                 for _ in range(n_tables)]

    def tables():
        for k, table in enumerate(device.tables):
            _lib.check(lib.tc_chi2_grad_leauthaud11_batch_device(
                table.handle, d_theta, 14, N, 10, _lib.FLAG_MODULATE_WITH_CENOCC,
                _lib.as_double_p(data), _lib.as_double_p(precision), *per_table[k]))

    def wait_tables():
        for table in device.tables:
            _lib.check(lib.tc_table_synchronize(table.handle))

    first = device.tables[0].handle
    result = {'n_tables': n_tables, 'n_classes': len(interp.class_tables), 'n_bins': n_bins,
              'n_r': n_r, 'n_dim': n_dim, 'tables_before': timed(tables, wait_tables),
              'chi2_fisher': timed(one_launch, wait),
              'tables_after': timed(tables, wait_tables)}
    result['chi2_fisher'].update(kernel_time(first, one_launch, wait))
    return result


results = {'n_draws': N}
if ONLY in (None, 'cross'):
    results['ds_efficient'] = measure(Interpolator.read(
        os.path.join(REPO, 'tests', 'golden', 'ds_efficient.hdf5')))
if ONLY in (None, 'auto'):
    tables, keys, points = synthetic.synthetic_interpolator((4, 4), 30, 1, (19, ), 'auto', seed=3)
    results['auto_4x4'] = measure(Interpolator(
        [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
         for t in tables], {key: points[:, d] for d, key in enumerate(keys)}))
print(json.dumps(results))
