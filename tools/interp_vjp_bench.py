"""Time of the occupation seam of an interpolator at 10^4 draws, device-resident:
tc_interp_chi2_occupation_grad_batch_device with the gradients (chi2_grad_occupation) and without
(chi2_occupation), on tests/golden/ds_efficient.hdf5 (mode cross, K = 4, 1104 bins) and on a 4 x 4
grid of mode-auto tables (synthetic, 100 bins, 19 r bins).  Next to it the same work the only way
the tables' own seam can do it: K tc_predict_occupation_vjp_batch_device launches, one per table,
and the spline over the K results in NumPy on the host (the transfers between the two are NOT
counted).  Wall clock around CALLS calls and a synchronize after WARM warm-up calls, REPEATS times:
the median and the run-to-run spread (max - min); the K launches are timed before and after the
interpolator's calls.  Prints one JSON line (profiles/interp_vjp_notes.md).

    python tools/interp_vjp_bench.py [n_draws [auto | cross]]
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
CALLS, WARM, REPEATS = 20, 5, 5
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
    n_classes, n_tables = len(interp.class_tables), len(interp.tabcorr_list)
    n_bins = len(interp.tabcorr_list[0].gal_type)
    n_r, n_dim = len(interp.tabcorr_list[0].tpcf_matrix), len(interp.keys)
    # (the time does not depend on the values: positive occupations, every draw with galaxies)
    occupation = rng.uniform(0.1, 2.0, size=(N, n_classes, n_bins))
    x = np.stack([rng.uniform(xp[0], xp[-1], N) for xp in interp.xp], axis=-1)
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    d_occupation, d_x = upload(occupation), upload(x)
    d_ngal, d_chi2 = upload(np.zeros(N)), upload(np.zeros(N))
    d_docc, d_dx, d_dngal = upload(np.zeros(occupation.shape)), upload(np.zeros(x.shape)), \
        upload(np.zeros(x.shape))

    def seam(gradient=True):
        outputs = (d_docc, d_dx, d_dngal) if gradient else (None, None, None)
        _lib.check(lib.tc_interp_chi2_occupation_grad_batch_device(
            device.handle, d_occupation, d_x, N, 0, _lib.as_double_p(data),
            _lib.as_double_p(precision), d_ngal, d_chi2, *outputs))

    def wait():
        _lib.check(lib.tc_interp_synchronize(device.handle))

    # the tables' own seam: one launch per table on that table's class of occupations
    class_rows = [upload(occupation[:, v]) for v in range(n_classes)]
    g_xi = upload(rng.normal(size=(N, n_r)))
    per_table = [(upload(np.zeros(N)), upload(np.zeros((N, n_r))), upload(np.zeros((N, n_bins))))
                 for _ in range(n_tables)]

    def tables():
        for k, table in enumerate(device.tables):
            _lib.check(lib.tc_predict_occupation_vjp_batch_device(
                table.handle, class_rows[interp.table_class[k]], N, 0, None, g_xi,
                *per_table[k]))

    def wait_tables():
        for table in device.tables:
            _lib.check(lib.tc_table_synchronize(table.handle))

    xi_t = rng.normal(size=(n_tables, N, n_r))

    def host_spline():
        weights = interp.class_weights(x)                 # the spline weights of every draw
        return weights, np.einsum('kdr,dk->dr', xi_t, np.ones((N, n_tables)))

    start = time.perf_counter()
    host_spline()
    spline_us = (time.perf_counter() - start) * 1e6
    first = device.tables[0].handle
    result = {'n_tables': n_tables, 'n_classes': n_classes, 'n_bins': n_bins, 'n_r': n_r,
              'n_dim': n_dim, 'tables_before': timed(tables, wait_tables),
              'chi2_grad_occupation': timed(seam, wait),
              'chi2_occupation': timed(lambda: seam(False), wait),
              'tables_after': timed(tables, wait_tables), 'host_spline_us': spline_us}
    result['chi2_grad_occupation'].update(kernel_time(first, seam, wait))
    result['chi2_occupation'].update(kernel_time(first, lambda: seam(False), wait))
    return result


results = {'n_draws': N}
if ONLY in (None, 'cross'):
    results['ds_efficient'] = measure(Interpolator.read(
        os.path.join(REPO, 'tests', 'golden', 'ds_efficient.hdf5')))
if ONLY in (None, 'auto'):
    tables, keys, points = synthetic.synthetic_interpolator((4, 4), 50, 1, (19, ), 'auto', seed=3)
    results['auto_4x4'] = measure(Interpolator(
        [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
         for t in tables], {key: points[:, d] for d, key in enumerate(keys)}))
print(json.dumps(results))
