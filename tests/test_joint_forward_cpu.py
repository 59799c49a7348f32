"""The forward calls of a joint of tables without a GPU: the LDS budget of joint_forward_kernel
against its closed form, what the entries refuse on the host (tc_debug_joint_forward_fit), the
exported symbols, and the argument checks of `JointLikelihood.predict_batch` / `chi2_batch`, which
fire before any device is touched."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_reference  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

LDS_LIMIT = 160 * 1024
MATH_TABLE_DOUBLES = 2306            # fastmath.h: the table the occupations read
AUTO, CROSS = 0, 1
F64, F32 = 0, 1
# the joints of tests/test_gpu_joint_forward.py: (bins, [(mode, n_r), ...])
SHAPES = [(24, [(AUTO, 5), (CROSS, 3)]), (24, [(AUTO, 19), (AUTO, 4), (CROSS, 7)]),
          (24, [(CROSS, 6), (CROSS, 2)]), (24, [(AUTO, 20)]), (24, [(CROSS, 1)]),
          (108, [(AUTO, 5), (CROSS, 3)]), (60, [(AUTO, 19), (CROSS, 19)]), (5, [(AUTO, 1)]),
          (248, [(AUTO, 3)])]
NEW_SYMBOLS = ['tc_joint_predict_batch', 'tc_joint_predict_batch_device', 'tc_joint_chi2_batch',
               'tc_joint_chi2_batch_device', 'tc_debug_joint_forward_lds_bytes',
               'tc_debug_joint_forward_fit']


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def closed_form(n_bins, n_total, waves=8):
    """joint.h: joint_forward_lds_bytes, restated in doubles: the densities (bins in whole fours,
    64) or the results tile (N, 65) in whole 16-byte words, whichever is larger; the math table or
    data | precision, N (N + 1); the waves' sums of ngal and chi2 (2, waves, 64); the passes' sums
    (waves / 2 parts, N, 64)."""
    dens = (n_bins + 3) // 4 * 4 * 64
    tile = (n_total * 65 + 1) // 2 * 2
    operands = n_total * (n_total + 1)
    return 8 * (max(dens, tile) + max(MATH_TABLE_DOUBLES, operands) + 2 * waves * 64 +
                waves // 2 * n_total * 64)


def forward_fit(lib, n_bins, members, dtypes=None):
    """(status, LDS bytes) of tc_debug_joint_forward_fit for [(mode, n_r), ...]."""
    n = len(members)
    mode = (ctypes.c_int * n)(*[m for m, _ in members])
    n_r = (ctypes.c_int * n)(*[r for _, r in members])
    dtype = (ctypes.c_int * n)(*(dtypes or [F64] * n))
    got = ctypes.c_int64(-1)
    status = lib.tc_debug_joint_forward_fit(n_bins, n, mode, n_r, dtype, ctypes.byref(got))
    return status, got.value


def test_library_exports_the_forward_symbols(lib):
    """Declared in the headers, present in the ctypes table and exported by the library; the entry
    of every (form, route) comes from FORWARD_ENTRIES."""
    from tabcorr_amd import _lib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    declared = entry.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert {_lib.FORWARD_ENTRIES['joint', form, route]
            for form in ('predict', 'chi2') for route in ('host', 'device')} == set(NEW_SYMBOLS[:4])
    assert ('joint', 'predict', 'async') not in _lib.FORWARD_ENTRIES
    # the argument order is that of the gradient entries with the derivative outputs removed
    for form in ('predict', 'chi2'):
        for suffix in ('', '_device'):
            grad = _lib.SIGNATURES['tc_joint_%s_grad_batch%s' % (form, suffix)]
            keep = len(grad) - (2 if form == 'predict' else 3)
            assert _lib.SIGNATURES['tc_joint_%s_batch%s' % (form, suffix)] == grad[:keep]


def test_lds_budget_has_its_closed_form(lib):
    from tabcorr_amd import _lib
    for n_bins, members in SHAPES:
        n_total = sum(r for _, r in members)
        for waves in (8, 16):
            got = ctypes.c_int64(-1)
            _lib.check(lib.tc_debug_joint_forward_lds_bytes(n_bins, n_total, waves,
                                                            ctypes.byref(got)))
            assert got.value == closed_form(n_bins, n_total, waves), (n_bins, members, waves)
        status, lds = forward_fit(lib, n_bins, members)
        assert status == _lib.TC_OK and lds == closed_form(n_bins, n_total) <= LDS_LIMIT
    # the real pair: 60 bins, N = 38 -- 30720 + 18448 + 8192 + 77824 bytes
    assert closed_form(60, 38) == 135184
    got = ctypes.c_int64(-1)
    for bad in ((0, 8, 8), (24, 0, 8), (24, 8, 7), (24, 8, 0), (24, 8, 18)):
        assert lib.tc_debug_joint_forward_lds_bytes(*bad, ctypes.byref(got)) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_joint_forward_lds_bytes(24, 8, 8, None) == _lib.TC_ERR_INVALID


def test_what_the_kernel_does_not_serve_is_refused_on_the_host(lib):
    """A joint beyond the LDS budget (by the formula: the largest served number of bins, then one
    block of four more), a mode-auto member of 21 r bins (a cross member of 21 is served) and a
    float32 member: TC_ERR_UNSUPPORTED with a message, which Python raises as
    NotImplementedError."""
    from tabcorr_amd import _lib
    members = [(AUTO, 19), (CROSS, 19)]
    n_bins = 4
    while closed_form(n_bins + 4, 38) <= LDS_LIMIT:
        n_bins += 4
    assert closed_form(n_bins, 38) <= LDS_LIMIT < closed_form(n_bins + 1, 38)
    assert forward_fit(lib, n_bins, members) == (_lib.TC_OK, closed_form(n_bins, 38))
    status, lds = forward_fit(lib, n_bins + 1, members)
    assert status == _lib.TC_ERR_UNSUPPORTED and lds == closed_form(n_bins + 1, 38)
    with pytest.raises(NotImplementedError, match='LDS'):
        _lib.check(status)
    # many rows: the passes' sums and the precision matrix
    status, lds = forward_fit(lib, 24, [(CROSS, 100)] * 3)
    assert status == _lib.TC_ERR_UNSUPPORTED and lds == closed_form(24, 300) > LDS_LIMIT
    assert forward_fit(lib, 24, [(AUTO, 20), (CROSS, 21)])[0] == _lib.TC_OK
    status, _ = forward_fit(lib, 24, [(CROSS, 3), (AUTO, 21)])
    assert status == _lib.TC_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match='table 1 .*21 correlation function bins'):
        _lib.check(status)
    status, _ = forward_fit(lib, 24, [(AUTO, 5), (CROSS, 3)], [F64, F32])
    assert status == _lib.TC_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match='float64 .*table 1'):
        _lib.check(status)
    # the hook's own arguments
    one = (ctypes.c_int * 1)(0)
    r = (ctypes.c_int * 1)(3)
    assert lib.tc_debug_joint_forward_fit(24, 1, None, r, one, None) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_joint_forward_fit(24, 17, one, r, one, None) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_joint_forward_fit(24, 1, (ctypes.c_int * 1)(2), r, one,
                                          None) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_joint_forward_fit(24, 1, one, r, one, None) == _lib.TC_OK


def test_c_entry_points_refuse_a_call_without_a_handle(lib):
    from tabcorr_amd import _lib
    p = _lib.as_double_p(np.zeros(0))
    assert lib.tc_joint_predict_batch(None, p, 5, 3, 10, 0, p, p) == _lib.TC_ERR_INVALID
    assert b'joint handle is NULL' in lib.tc_last_error()
    assert lib.tc_joint_chi2_batch(None, p, 5, 3, 10, 0, p, p, p, p) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_predict_batch_device(None, None, 5, 3, 10, 0, None,
                                             None) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_chi2_batch_device(None, None, 5, 3, 10, 0, p, p, None,
                                          None) == _lib.TC_ERR_INVALID
    # ... also an empty batch
    assert lib.tc_joint_predict_batch(None, p, 5, 0, 10, 0, p, p) == _lib.TC_ERR_INVALID


def test_calls_refuse_wrong_shapes_before_any_device():
    from tabcorr_amd import JointLikelihood, TabCorr
    tables = joint_reference.make_tables(6, 2, [('auto', (5, )), ('cross', (3, ))])
    halotabs = [TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                    table['tpcf_shape'], table['attrs']) for table in tables]
    joint = JointLikelihood(halotabs)
    theta = synthetic.zheng07_draws(3, seed=2)
    good_data, good_precision = np.zeros(8), np.eye(8)
    for data, precision in ((np.zeros(7), good_precision), (np.zeros((8, 2)), good_precision),
                            ([np.zeros(5), np.zeros(4)], good_precision),
                            (good_data, np.eye(5)), (good_data, np.ones((8, 9))),
                            (good_data, np.ones(64))):
        with pytest.raises(ValueError, match='data'):
            joint.chi2_batch(theta, data, precision)
    for columns in (4, 7):
        with pytest.raises(ValueError, match='theta'):
            joint.predict_batch(np.zeros((3, columns)))
        with pytest.raises(ValueError, match='theta'):
            joint.chi2_batch(np.zeros((3, columns)), good_data, good_precision)
    with pytest.raises(ValueError, match='theta'):
        joint.predict_batch(theta, assembias=True)
    with pytest.raises(ValueError, match='theta'):
        joint.chi2_batch(np.zeros((3, 5)), good_data, good_precision, assembias=True)
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.predict_batch(np.zeros((3, 14)), family='leauthaud11')
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.chi2_batch(np.zeros((3, 14)), good_data, good_precision, family='leauthaud11')
    with pytest.raises(ValueError, match='family'):
        joint.chi2_batch(theta, good_data, good_precision, family='zu_mandelbaum15')
    assert joint._device is None and all(halotab._device is None for halotab in halotabs)
