"""The slab arithmetic of the derivative entry points without a GPU (csrc/grad_call.h:
GradRequest::slab, through tc_debug_grad_slab): the offset of every array of a call against its
closed form, for every family, with and without an interpolator's extra columns, in both forms,
up to `begin` values whose products lie far beyond 2^31 elements."""

import ctypes

import numpy as np
import pytest

THETA_COLUMNS = {5: 5, 7: 7, 11: 14}         # (grad.h: grad_theta_columns)
BEGINS = [0, 1, 1 << 18, (1 << 18) + 17, (1 << 31) - 1, 1 << 31, (1 << 31) + 5, (1 << 33) + 3]


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def offsets_of(lib, n_params, n_extra, n_r, likelihood, begin):
    from tabcorr_amd import _lib
    out = (ctypes.c_int64 * 7)()
    _lib.check(lib.tc_debug_grad_slab(n_params, n_extra, n_r, int(likelihood), begin, out))
    return list(out)


@pytest.mark.parametrize('likelihood', [False, True], ids=['prediction', 'likelihood'])
@pytest.mark.parametrize('n_extra', [0, 1, 3])
@pytest.mark.parametrize('n_params', [5, 7, 11])
def test_offsets_of_a_slab(lib, n_params, n_extra, likelihood):
    for n_r in (1, 2, 19, 38, 1000):
        n_cols = n_params + n_extra
        wide = 1 if likelihood else n_r
        for begin in BEGINS:
            theta, x, ngal, dngal, value, dvalue, fisher = offsets_of(
                lib, n_params, n_extra, n_r, likelihood, begin)
            what = (n_params, n_extra, n_r, likelihood, begin)
            assert theta == begin * THETA_COLUMNS[n_params], what
            assert x == (begin * n_extra if n_extra else -1), what
            assert ngal == begin, what
            assert dngal == begin * n_cols, what
            assert value == begin * wide, what
            assert dvalue == begin * n_cols * wide, what
            assert fisher == (begin * n_cols * n_cols if likelihood else -1), what
    # (the largest product of the cases: beyond 2^31 by many orders, within 2^63)
    assert ((1 << 33) + 3) * 14 * 1000 * 8 > 1 << 46
    assert ((1 << 33) + 3) * 14 * 1000 * 8 < 1 << 62


def test_refuses_what_is_no_call(lib):
    from tabcorr_amd import _lib
    out = (ctypes.c_int64 * 7)()
    assert lib.tc_debug_grad_slab(6, 0, 19, 0, 0, out) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_grad_slab(5, -1, 19, 0, 0, out) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_grad_slab(5, 0, 0, 0, 0, out) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_grad_slab(5, 0, 19, 0, -1, out) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_grad_slab(5, 0, 19, 0, 0, None) == _lib.TC_ERR_INVALID
    assert np.all(np.array(offsets_of(lib, 5, 0, 19, False, 0))[[0, 2, 3, 4, 5]] == 0)
