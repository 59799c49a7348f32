"""Scaffolding shared by the derivative suites on the device (test_gpu_grad.py,
test_gpu_interp_grad.py, test_gpu_vjp.py)."""

import ctypes

import numpy as np
import pytest

from oracle import tabcorr_oracle as oracle
from tabcorr_amd import synthetic
from util import assert_rel

RTOL = 1e-10                         # the project's parity bar
D = 16                               # draws per workgroup of the derivative kernels (grad.h)
LDS_LIMIT = 160 * 1024               # a workgroup has 160 KiB


def device_call(device, entry, arguments, output_shapes, synchronize='tc_table_synchronize'):
    """The C entry point `entry` of the handle `device` on freshly allocated device arrays.
    `arguments` is what follows the handle, in order, up to the outputs: every NumPy array
    among them goes up and is passed as its device pointer, everything else -- counts, flags,
    host-side pointers, None -- as it is.  The outputs, float64 arrays of `output_shapes`, are the
    entry's last arguments and come back after `synchronize`."""
    from tabcorr_amd import _lib
    lib = device.lib
    inputs = [np.ascontiguousarray(a) for a in arguments if isinstance(a, np.ndarray)]
    outputs = [np.empty(shape) for shape in output_shapes]
    pointers = []
    try:
        for array in inputs + outputs:
            ptr = ctypes.c_void_p()
            _lib.check(lib.tc_device_malloc(ctypes.byref(ptr), max(array.nbytes, 8)))
            pointers.append(ptr)
        uploaded = iter(pointers[:len(inputs)])
        passed = [next(uploaded) if isinstance(a, np.ndarray) else a for a in arguments]
        with device.lock:
            for array, ptr in zip(inputs, pointers):
                _lib.check(lib.tc_memcpy_h2d(ptr, array.ctypes.data_as(ctypes.c_void_p),
                                             array.nbytes))
            _lib.check(getattr(lib, entry)(device.handle, *passed, *pointers[len(inputs):]))
            _lib.check(getattr(lib, synchronize)(device.handle))
            for array, ptr in zip(outputs, pointers[len(inputs):]):
                _lib.check(lib.tc_memcpy_d2h(array.ctypes.data_as(ctypes.c_void_p), ptr,
                                             array.nbytes))
    finally:
        for ptr in pointers:
            lib.tc_device_free(ptr)
    return outputs


def largest(served):
    """The largest size that `served` accepts (sizes are served up to a limit)."""
    size = 1
    while served(size + 1):
        size += 1
    assert served(size) and not served(size + 1)
    return size


def chi2_data(xi, symmetric):
    """A data vector near `xi` (one draw's) and a precision matrix, symmetric positive definite or
    with a non-symmetric part on top."""
    n_r = xi.size
    rng = np.random.default_rng(11)
    a = rng.normal(size=(n_r, n_r))
    precision = a @ a.T + n_r * np.eye(n_r)
    if not symmetric:
        precision = precision + rng.normal(size=(n_r, n_r))
    return xi * (1.0 + 0.05 * rng.normal(size=xi.shape)), precision


def same_bits(got, expect, reshape=False):
    """Every array of `got` is bit-equal to its partner in `expect`, NaNs equal; reshape: `got`
    reports the correlation function bins on one axis (the C layout), `expect` on tpcf_shape."""
    return all(np.array_equal(np.reshape(a, np.shape(b)) if reshape else a, b, equal_nan=True)
               for a, b in zip(got, expect))


def check_still_serves(halotab, table, rtol=RTOL):
    """The handle serves predict_batch."""
    theta = synthetic.zheng07_draws(5, seed=2)
    expect = oracle.predict_zheng07_batch(table, theta)
    ngal, xi = halotab.predict_batch(theta)
    assert_rel(ngal, expect[0], rtol)
    assert_rel(xi, expect[1], rtol)


def check_refused(halotab, table, call, match='LDS', rtol=RTOL):
    """`call` (of five Zheng07 draws) raises NotImplementedError naming `match` and the handle
    goes on serving predict_batch."""
    with pytest.raises(NotImplementedError, match=match):
        call(synthetic.zheng07_draws(5, seed=2))
    check_still_serves(halotab, table, rtol)
