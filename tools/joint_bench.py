"""Time of tc_joint_chi2_grad_batch_device (with fisher) on the real pair (tests/golden/bolplanck_wp
+ bolplanck_ds, N = 38) at 10^4 draws against the two tables' own tc_chi2_grad_zheng07_batch_device
calls: device events around 20 calls after warm-up, and the mean of the launches' own events.
Prints one JSON line (profiles/joint_notes.md).

    python tools/joint_bench.py joint            # this tree: the joint calls and the tables' calls
    python tools/joint_bench.py tables DIR       # the tables' calls with the package of the
                                                 # checkout DIR (the commit before the joint)
    python tools/joint_bench.py forward [DIR]    # the forward form (profiles/joint_forward_notes.md):
                                                 # tc_joint_chi2_batch_device against (A) the joint's
                                                 # chi2_grad entry with fisher = NULL and (B) the two
                                                 # tables' own tc_chi2_zheng07_batch_device calls; a
                                                 # checkout DIR without the forward entries gives A and B
"""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
which = sys.argv[1]
assert which in ('joint', 'tables', 'forward')
sys.path.insert(0, os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else REPO)
sys.path.insert(1, os.path.join(REPO, 'tests'))
import tabcorr_amd  # noqa: E402
from tabcorr_amd import TabCorr, _lib, synthetic  # noqa: E402
from util import load_golden, table_from_golden  # noqa: E402

assert os.path.dirname(os.path.dirname(tabcorr_amd.__file__)) == sys.path[0]
N, CALLS, WARM = 10000, 20, 5
tables = [table_from_golden(load_golden(name)) for name in ('bolplanck_wp', 'bolplanck_ds')]
halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'], t['attrs'])
            for t in tables]
theta = np.ascontiguousarray(synthetic.zheng07_draws(N, seed=1))
lib = _lib.load()


def malloc(count):
    ptr = ctypes.c_void_p()
    _lib.check(lib.tc_device_malloc(ctypes.byref(ptr), count * 8))
    return ptr


d_theta = malloc(theta.size)
_lib.check(lib.tc_memcpy_h2d(d_theta, theta.ctypes.data_as(ctypes.c_void_p), theta.nbytes))
d_ngal, d_chi2, d_dngal, d_dchi2, d_fisher = (malloc(N), malloc(N), malloc(5 * N), malloc(5 * N),
                                              malloc(25 * N))
rng = np.random.default_rng(3)


def operands(n_r):
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    return data, precision


def timed(handle, call, synchronize):
    """ms per call from device events around CALLS calls, and the kernels' own events."""
    for _ in range(WARM):
        call()
    synchronize()
    elapsed, mean, count = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
    _lib.check(lib.tc_table_timer_begin(handle, 1))
    for _ in range(CALLS):
        call()
    synchronize()
    _lib.check(lib.tc_table_timer_end(handle, ctypes.byref(elapsed)))
    _lib.check(lib.tc_table_kernel_time(handle, ctypes.byref(count), ctypes.byref(mean)))
    return {'us_per_call': elapsed.value / CALLS * 1e3, 'kernel_us': mean.value * 1e3,
            'launches': count.value}


result = {'which': which, 'n_draws': N}
devices = [h.to_device() for h in halotabs]
if which == 'forward':
    from tabcorr_amd import JointLikelihood
    joint = JointLikelihood(halotabs).to_device()
    data, precision = operands(38)
    sync = lambda: _lib.check(lib.tc_joint_synchronize(joint.handle))

    def call_grad():
        _lib.check(lib.tc_joint_chi2_grad_batch_device(
            joint.handle, d_theta, 5, N, 10, 0, _lib.as_double_p(data),
            _lib.as_double_p(precision), d_ngal, d_chi2, d_dngal, d_dchi2, None))

    result['A_joint_chi2_grad'] = timed(devices[0].handle, call_grad, sync)
    for name, device in zip(('wp', 'ds'), devices):
        kept = operands(device.n_r)

        def call(device=device, kept=kept):
            _lib.check(lib.tc_chi2_zheng07_batch_device(
                device.handle, d_theta, 5, N, 10, 0, _lib.as_double_p(kept[0]),
                _lib.as_double_p(kept[1]), d_ngal, d_chi2))

        result['table_chi2_' + name] = timed(
            device.handle, call,
            lambda device=device: _lib.check(lib.tc_table_synchronize(device.handle)))
    result['B_tables_chi2_us'] = sum(result['table_chi2_' + name]['us_per_call']
                                     for name in ('wp', 'ds'))
    if hasattr(lib, 'tc_joint_chi2_batch_device'):
        d_xi = malloc(N * 38)
        # the pair, and each table alone in a joint: what the matrix and the chains cost
        for label, members in (('joint', halotabs), ('joint_wp', halotabs[:1]),
                               ('joint_ds', halotabs[1:])):
            member = JointLikelihood(members)
            handle = member.to_device().handle
            kept = operands(member.n_r_total)

            def call_chi2(handle=handle, kept=kept):
                _lib.check(lib.tc_joint_chi2_batch_device(
                    handle, d_theta, 5, N, 10, 0, _lib.as_double_p(kept[0]),
                    _lib.as_double_p(kept[1]), d_ngal, d_chi2))

            def call_predict(handle=handle):
                _lib.check(lib.tc_joint_predict_batch_device(handle, d_theta, 5, N, 10, 0, d_ngal,
                                                             d_xi))

            wait = lambda handle=handle: _lib.check(lib.tc_joint_synchronize(handle))
            timer = members[0].to_device().handle
            result[label + '_chi2'] = timed(timer, call_chi2, wait)
            result[label + '_predict'] = timed(timer, call_predict, wait)
    print(json.dumps(result))
    sys.exit(0)
for name, device in zip(('wp', 'ds'), devices):
    data, precision = operands(device.n_r)
    kept = (data, precision)

    def call(device=device, kept=kept):
        _lib.check(lib.tc_chi2_grad_zheng07_batch_device(
            device.handle, d_theta, 5, N, 10, 0, _lib.as_double_p(kept[0]),
            _lib.as_double_p(kept[1]), d_ngal, d_chi2, d_dngal, d_dchi2))

    result['table_' + name] = timed(
        device.handle, call,
        lambda device=device: _lib.check(lib.tc_table_synchronize(device.handle)))
    if which == 'joint':
        def call_fisher(device=device, kept=kept):
            _lib.check(lib.tc_chi2_fisher_zheng07_batch_device(
                device.handle, d_theta, 5, N, 10, 0, _lib.as_double_p(kept[0]),
                _lib.as_double_p(kept[1]), d_ngal, d_chi2, d_dngal, d_dchi2, d_fisher))
        result['table_fisher_' + name] = timed(
            device.handle, call_fisher,
            lambda device=device: _lib.check(lib.tc_table_synchronize(device.handle)))
if which == 'joint':
    from tabcorr_amd import JointLikelihood
    joint = JointLikelihood(halotabs).to_device()
    data, precision = operands(38)

    def call_joint():
        _lib.check(lib.tc_joint_chi2_grad_batch_device(
            joint.handle, d_theta, 5, N, 10, 0, _lib.as_double_p(data),
            _lib.as_double_p(precision), d_ngal, d_chi2, d_dngal, d_dchi2, d_fisher))

    result['joint_fisher'] = timed(devices[0].handle, call_joint,
                                   lambda: _lib.check(lib.tc_joint_synchronize(joint.handle)))
if which == 'joint':
    d_xi, d_dxi = malloc(N * 38), malloc(N * 5 * 38)

    def call_predict():
        _lib.check(lib.tc_joint_predict_grad_batch_device(
            joint.handle, d_theta, 5, N, 10, 0, d_ngal, d_xi, d_dngal, d_dxi))

    def call_no_fisher():
        _lib.check(lib.tc_joint_chi2_grad_batch_device(
            joint.handle, d_theta, 5, N, 10, 0, _lib.as_double_p(data),
            _lib.as_double_p(precision), d_ngal, d_chi2, d_dngal, d_dchi2, None))

    sync = lambda: _lib.check(lib.tc_joint_synchronize(joint.handle))
    result['joint_predict'] = timed(devices[0].handle, call_predict, sync)
    result['joint_chi2_grad'] = timed(devices[0].handle, call_no_fisher, sync)
    # fewer draws: 512 workgroups of 16 fit the chip in one round at two workgroups per CU
    N = 8192
    result['joint_fisher_8192'] = timed(devices[0].handle, call_joint, sync)
    for name, device in zip(('wp', 'ds'), devices):
        kept = operands(device.n_r)

        def call_fisher(device=device, kept=kept):
            _lib.check(lib.tc_chi2_fisher_zheng07_batch_device(
                device.handle, d_theta, 5, N, 10, 0, _lib.as_double_p(kept[0]),
                _lib.as_double_p(kept[1]), d_ngal, d_chi2, d_dngal, d_dchi2, d_fisher))
        result['table_fisher_%s_8192' % name] = timed(
            device.handle, call_fisher,
            lambda device=device: _lib.check(lib.tc_table_synchronize(device.handle)))
print(json.dumps(result))
