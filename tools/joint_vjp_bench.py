"""Time of the occupation seam of a joint on the real pair (tests/golden/bolplanck_wp +
bolplanck_ds, 60 bins, N = 38) at 10^4 draws: tc_joint_chi2_occupation_grad_batch_device with the
gradient (chi2_grad_occupation) and without (chi2_occupation), against the two tables' own
tc_chi2_occupation_grad_batch_device calls on the same occupations.  Device events around 20 calls
after warm-up, REPEATS times: the median and the run-to-run spread (max - min) of each, and the
mean of the launches' own events.  Prints one JSON line (profiles/joint_vjp_notes.md).

    python tools/joint_vjp_bench.py joint          # this tree: the joint calls and the tables' calls
    python tools/joint_vjp_bench.py tables DIR     # the tables' calls with the package of the
                                                   # checkout DIR (the commit before the joint seam)
"""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
which = sys.argv[1]
assert which in ('joint', 'tables')
sys.path.insert(0, os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else REPO)
sys.path.insert(1, os.path.join(REPO, 'tests'))
import tabcorr_amd  # noqa: E402
from tabcorr_amd import TabCorr, _lib  # noqa: E402
from util import load_golden, table_from_golden  # noqa: E402

assert os.path.dirname(os.path.dirname(tabcorr_amd.__file__)) == sys.path[0]
N, CALLS, WARM, REPEATS = 10000, 20, 5, 5
tables = [table_from_golden(load_golden(name)) for name in ('bolplanck_wp', 'bolplanck_ds')]
halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
            for t in tables]
n_bins = len(tables[0]['gal_type'])
rng = np.random.default_rng(3)
# (the time does not depend on the values: positive occupations, every draw with galaxies)
occupation = np.ascontiguousarray(rng.uniform(0.1, 2.0, size=(N, n_bins)))
lib = _lib.load()


def malloc(count):
    ptr = ctypes.c_void_p()
    _lib.check(lib.tc_device_malloc(ctypes.byref(ptr), count * 8))
    return ptr


d_occupation = malloc(occupation.size)
_lib.check(lib.tc_memcpy_h2d(d_occupation, occupation.ctypes.data_as(ctypes.c_void_p),
                             occupation.nbytes))
d_ngal, d_chi2, d_docc = malloc(N), malloc(N), malloc(N * n_bins)


def operands(n_r):
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    return data, precision


def timed(handle, call, synchronize):
    """us per call from device events around CALLS calls, REPEATS times, and the kernels' own
    events of the last repeat."""
    for _ in range(WARM):
        call()
    synchronize()
    elapsed, mean, count = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
    runs = []
    for _ in range(REPEATS):
        _lib.check(lib.tc_table_timer_begin(handle, 1))
        for _ in range(CALLS):
            call()
        synchronize()
        _lib.check(lib.tc_table_timer_end(handle, ctypes.byref(elapsed)))
        _lib.check(lib.tc_table_kernel_time(handle, ctypes.byref(count), ctypes.byref(mean)))
        runs.append(elapsed.value / CALLS * 1e3)
    return {'us_per_call': float(np.median(runs)), 'spread_us': max(runs) - min(runs),
            'runs_us': runs, 'kernel_us': mean.value * 1e3, 'launches': count.value}


result = {'which': which, 'n_draws': N}
devices = [h.to_device() for h in halotabs]
for name, device in zip(('wp', 'ds'), devices):
    kept = operands(device.n_r)

    def call(device=device, kept=kept):
        _lib.check(lib.tc_chi2_occupation_grad_batch_device(
            device.handle, d_occupation, N, 0, _lib.as_double_p(kept[0]),
            _lib.as_double_p(kept[1]), d_ngal, d_chi2, d_docc))

    result['table_' + name] = timed(
        device.handle, call,
        lambda device=device: _lib.check(lib.tc_table_synchronize(device.handle)))
result['tables_us'] = sum(result['table_' + name]['us_per_call'] for name in ('wp', 'ds'))
result['tables_spread_us'] = sum(result['table_' + name]['spread_us'] for name in ('wp', 'ds'))
if which == 'joint':
    from tabcorr_amd import JointLikelihood
    # the pair, and each table alone in a joint: what the joint's own walk costs
    for label, members in (('joint', halotabs), ('joint_wp', halotabs[:1]),
                           ('joint_ds', halotabs[1:])):
        member = JointLikelihood(members)
        handle = member.to_device().handle
        kept = operands(member.n_r_total)

        def call_grad(handle=handle, kept=kept, gradient=d_docc):
            _lib.check(lib.tc_joint_chi2_occupation_grad_batch_device(
                handle, d_occupation, N, 0, _lib.as_double_p(kept[0]), _lib.as_double_p(kept[1]),
                d_ngal, d_chi2, gradient))

        wait = lambda handle=handle: _lib.check(lib.tc_joint_synchronize(handle))
        timer = members[0].to_device().handle
        result[label + '_chi2_grad_occupation'] = timed(timer, call_grad, wait)
        result[label + '_chi2_occupation'] = timed(
            timer, lambda call_grad=call_grad: call_grad(gradient=None), wait)
print(json.dumps(result))
