"""Time of tc_joint_interp_chi2_grad_batch_device (without and with the Fisher matrix) at 10^4 draws
against the two members' own tc_interp_chi2_grad_zheng07_batch_device calls -- all a user could do
before, and without the off-diagonal blocks of the covariance --, for two pairs:

    synthetic   (w_p: mode auto, 19 r; DeltaSigma: mode cross, 19 r) on 5 x 5 grids of 100 bins:
                the rows form;
    abacus      tests/golden/ds_efficient.hdf5 (4 tables of 1104 bins, mode cross) and a second
                member of its first five r rows: the slab form.

Device events around 20 calls after warm-up, and the mean of the launches' own events; three
repeats each.  Prints one JSON line (profiles/joint_notes.md).

    python tools/joint_interp_bench.py joint         # this tree: the joint's and the members' calls
    python tools/joint_interp_bench.py members DIR   # the members' calls with the package of the
                                                     # checkout DIR (the commit before the joint)
    python tools/joint_interp_bench.py forward [DIR] # the forward form (profiles/
                                                     # joint_interp_forward_notes.md):
                                                     # tc_joint_interp_chi2_batch_device against A,
                                                     # the joint's chi2_grad call without the Fisher
                                                     # matrix, and B, the sum of the members' own
                                                     # tc_interp_chi2_zheng07_batch_device calls;
                                                     # with the package of a checkout DIR that has
                                                     # no forward form yet: A and B alone
"""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
which = sys.argv[1]
assert which in ('joint', 'members', 'forward')
sys.path.insert(0, os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else REPO)
import tabcorr_amd  # noqa: E402
from tabcorr_amd import Interpolator, TabCorr, _lib, synthetic  # noqa: E402

assert os.path.dirname(os.path.dirname(tabcorr_amd.__file__)) == sys.path[0]
N, CALLS, WARM, REPEATS = 10000, 20, 5, 3
lib = _lib.load()
rng = np.random.default_rng(3)


def synthetic_pair():
    members = []
    for mode in ('auto', 'cross'):
        tables, keys, points = synthetic.synthetic_interpolator((5, 5), 50, 1, (19, ), mode,
                                                                seed=40)
        halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'],
                                        t['attrs']) for t in tables]
        members.append(Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)}))
    return members, np.ascontiguousarray(synthetic.zheng07_draws(N, seed=1))


def abacus_pair():
    first = Interpolator.read(os.path.join(REPO, 'tests', 'golden', 'ds_efficient.hdf5'))
    halotabs = [TabCorr.from_arrays(t.gal_type, 3.0 * np.asarray(t.tpcf_matrix)[:5], (5, ),
                                    t.attrs) for t in first.tabcorr_list]
    second = Interpolator(halotabs, {key: first.points[:, d] for d, key in enumerate(first.keys)})
    theta = synthetic.zheng07_draws(N, seed=9)
    theta[:, 0] = rng.uniform(12.5, 13.3, N)
    theta[:, 3] = rng.uniform(13.6, 14.4, N)
    return [first, second], np.ascontiguousarray(theta)


def malloc(count):
    ptr = ctypes.c_void_p()
    _lib.check(lib.tc_device_malloc(ctypes.byref(ptr), count * 8))
    return ptr


def upload(array):
    ptr = malloc(array.size)
    _lib.check(lib.tc_memcpy_h2d(ptr, array.ctypes.data_as(ctypes.c_void_p), array.nbytes))
    return ptr


def operands(n_r):
    data = np.ascontiguousarray(rng.uniform(0.5, 1.5, n_r))
    precision = np.ascontiguousarray(np.eye(n_r) + 0.01 * rng.normal(size=(n_r, n_r)))
    return data, precision


def timed(handle, call, synchronize):
    """us per call from device events around CALLS calls and the kernels' own events, REPEATS
    times."""
    out = {'us_per_call': [], 'kernel_us': []}
    for _ in range(WARM):
        call()
    synchronize()
    for _ in range(REPEATS):
        elapsed, mean, count = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
        _lib.check(lib.tc_table_timer_begin(handle, 1))
        for _ in range(CALLS):
            call()
        synchronize()
        _lib.check(lib.tc_table_timer_end(handle, ctypes.byref(elapsed)))
        _lib.check(lib.tc_table_kernel_time(handle, ctypes.byref(count), ctypes.byref(mean)))
        out['us_per_call'].append(round(elapsed.value / CALLS * 1e3, 1))
        out['kernel_us'].append(round(mean.value * 1e3, 1))
        out['launches'] = count.value
    return out


def measure_forward(members, d_theta, d_x, d_ngal, d_chi2, d_dngal, d_dchi2):
    """B: every member's own forward likelihood; A: the joint's chi2 and gradient, no Fisher
    matrix; and the joint's forward likelihood where the package has it."""
    from tabcorr_amd import JointInterpolator
    result = {}
    for m, interp in enumerate(members):
        device = interp.to_device()
        kept = operands(device.tables[0].n_r)

        def call(device=device, kept=kept):
            _lib.check(lib.tc_interp_chi2_zheng07_batch_device(
                device.handle, d_theta, 5, d_x, N, 10, 0, _lib.as_double_p(kept[0]),
                _lib.as_double_p(kept[1]), d_ngal, d_chi2))

        def sync(device=device):
            _lib.check(lib.tc_interp_synchronize(device.handle))

        result['B_member_%d_chi2' % m] = timed(device.tables[0].handle, call, sync)
    joint = JointInterpolator(members)
    device = joint.to_device()
    data, precision = operands(joint.n_r_total)
    handle = members[0].to_device().tables[0].handle

    def sync():
        _lib.check(lib.tc_joint_interp_synchronize(device.handle))

    def call_grad():
        _lib.check(lib.tc_joint_interp_chi2_grad_batch_device(
            device.handle, d_theta, 5, d_x, N, 10, 0, _lib.as_double_p(data),
            _lib.as_double_p(precision), d_ngal, d_chi2, d_dngal, d_dchi2, None))

    result['A_joint_chi2_grad'] = timed(handle, call_grad, sync)
    entry = _lib.FORWARD_ENTRIES.get(('joint_interp', 'chi2', 'device'))
    if entry is not None:
        forward = getattr(lib, entry)

        def call_forward():
            _lib.check(forward(device.handle, d_theta, 5, d_x, N, 10, 0, _lib.as_double_p(data),
                               _lib.as_double_p(precision), d_ngal, d_chi2))

        result['joint_chi2_forward'] = timed(handle, call_forward, sync)
    return result


def measure(members, theta):
    n_dim = len(members[0].keys)
    x = np.ascontiguousarray(np.stack([rng.uniform(xp[0], xp[-1], N) for xp in members[0].xp],
                                      axis=-1))
    n_cols = 5 + n_dim
    d_theta, d_x = upload(theta), upload(x)
    d_ngal, d_chi2, d_dngal, d_dchi2 = malloc(N), malloc(N), malloc(n_cols * N), malloc(n_cols * N)
    if which == 'forward':
        result = measure_forward(members, d_theta, d_x, d_ngal, d_chi2, d_dngal, d_dchi2)
        for ptr in (d_theta, d_x, d_ngal, d_chi2, d_dngal, d_dchi2):
            lib.tc_device_free(ptr)
        return result
    d_fisher = malloc(n_cols * n_cols * N)
    result = {}
    for m, interp in enumerate(members):
        device = interp.to_device()
        kept = operands(device.tables[0].n_r)

        def call(device=device, kept=kept):
            _lib.check(lib.tc_interp_chi2_grad_zheng07_batch_device(
                device.handle, d_theta, 5, d_x, N, 10, 0, _lib.as_double_p(kept[0]),
                _lib.as_double_p(kept[1]), d_ngal, d_chi2, d_dngal, d_dchi2))

        def call_fisher(device=device, kept=kept):
            _lib.check(lib.tc_interp_chi2_fisher_zheng07_batch_device(
                device.handle, d_theta, 5, d_x, N, 10, 0, _lib.as_double_p(kept[0]),
                _lib.as_double_p(kept[1]), d_ngal, d_chi2, d_dngal, d_dchi2, d_fisher))

        def sync(device=device):
            _lib.check(lib.tc_interp_synchronize(device.handle))

        result['member_%d_chi2_grad' % m] = timed(device.tables[0].handle, call, sync)
        result['member_%d_chi2_fisher' % m] = timed(device.tables[0].handle, call_fisher, sync)
    if which == 'joint':
        from tabcorr_amd import JointInterpolator
        joint = JointInterpolator(members)
        device = joint.to_device()
        data, precision = operands(joint.n_r_total)

        def call_joint(fisher):
            _lib.check(lib.tc_joint_interp_chi2_grad_batch_device(
                device.handle, d_theta, 5, d_x, N, 10, 0, _lib.as_double_p(data),
                _lib.as_double_p(precision), d_ngal, d_chi2, d_dngal, d_dchi2, fisher))

        def sync():
            _lib.check(lib.tc_joint_interp_synchronize(device.handle))

        handle = members[0].to_device().tables[0].handle
        result['joint_chi2_grad'] = timed(handle, lambda: call_joint(None), sync)
        result['joint_chi2_fisher'] = timed(handle, lambda: call_joint(d_fisher), sync)
    for ptr in (d_theta, d_x, d_ngal, d_chi2, d_dngal, d_dchi2, d_fisher):
        lib.tc_device_free(ptr)
    return result


print(json.dumps({'which': which, 'n_draws': N, 'synthetic': measure(*synthetic_pair()),
                  'abacus': measure(*abacus_pair())}))
