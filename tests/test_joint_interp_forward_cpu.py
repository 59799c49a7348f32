"""The forward calls of a joint of interpolators without a GPU: the LDS budgets of the two forms of
joint_interp_forward_kernel against their closed forms, what the entries refuse on the host
(tc_debug_joint_interp_forward_fit), the exported symbols, and the argument checks of
`JointInterpolator.predict_batch` / `chi2_batch`, which fire before any device is touched."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_interp_reference as reference  # noqa: E402
from tabcorr_amd import synthetic  # noqa: E402

LDS_LIMIT = 160 * 1024
MATH_TABLE_DOUBLES = 2306            # fastmath.h: the table the occupations read
SLAB = 64                            # joint_interp.h: kJointInterpForwardSlab
AUTO, CROSS = 0, 1
SLABS, ROWS = 0, 1
# (bins, [(mode, n_r), ...], grid): the joints of tests/test_gpu_joint_interp_forward.py, the
# synthetic pair of tools/joint_interp_bench.py and the shape of tests/golden/ds_efficient.hdf5
# with a second member of five rows
BENCH_PAIR = (100, [(AUTO, 19), (CROSS, 19)], (5, 5))
DS_EFFICIENT = (1104, [(CROSS, 19), (CROSS, 5)], (4, ))
SHAPES = [(18, [(AUTO, 3), (CROSS, 5)], (4, )), (36, [(AUTO, 3), (CROSS, 5)], (4, 4)),
          (32, [(CROSS, 5), (AUTO, 3)], (4, )), (36, [(AUTO, 20), (AUTO, 1), (CROSS, 7)], (4, )),
          (36, [(CROSS, 5), (CROSS, 3)], (4, )), (160, [(CROSS, 5), (CROSS, 3)], (4, 4)),
          (18, [(AUTO, 3)], (4, )), (36, [(CROSS, 5)], (4, )), (248, [(AUTO, 3)], (4, )),
          BENCH_PAIR, DS_EFFICIENT]
NEW_SYMBOLS = ['tc_joint_interp_predict_batch', 'tc_joint_interp_predict_batch_device',
               'tc_joint_interp_chi2_batch', 'tc_joint_interp_chi2_batch_device',
               'tc_debug_joint_interp_forward_lds_bytes', 'tc_debug_joint_interp_forward_fit']


@pytest.fixture(scope='module')
def lib():
    from tabcorr_amd import build, _lib
    build.build()
    return _lib.load()


def rows_form(n_bins, n_total, weight_rows, waves=8):
    """joint_interp.h: joint_interp_forward_rows_lds_bytes, restated in doubles: the regions of
    joint_forward_kernel -- the densities (bins in whole fours, 64) or the results tile (N, 65) in
    whole 16-byte words; the math table or data | precision; the waves' sums (2, waves, 64); the
    passes' slabs (waves / 2, N, 64), which are the accumulators -- then the spline weights
    (sum of the axes' nodes, 64) and the class's 1 / ngal and 1 / ngal^2 (2, 64)."""
    dens = (n_bins + 3) // 4 * 4 * 64
    tile = (n_total * 65 + 1) // 2 * 2
    operands = n_total * (n_total + 1)
    return 8 * (max(dens, tile) + max(MATH_TABLE_DOUBLES, operands) + 2 * waves * 64 +
                waves // 2 * n_total * 64 + (weight_rows + 2) * 64)


def slab_form(n_total, weight_rows, waves=8):
    """joint_interp.h: joint_interp_forward_slabs_lds_bytes: one slab of densities (64, 64) or the
    results tile; the math table or data | precision; the waves' sums; the class's products and
    the accumulators (2, N, 64); the spline weights and the class's 1 / ngal, 1 / ngal^2."""
    tile = (n_total * 65 + 1) // 2 * 2
    operands = n_total * (n_total + 1)
    return 8 * (max(SLAB * 64, tile) + max(MATH_TABLE_DOUBLES, operands) + 2 * waves * 64 +
                2 * n_total * 64 + (weight_rows + 2) * 64)


def closed_form(n_bins, members, grid, waves=8):
    n_total = sum(r for _, r in members)
    if any(mode == AUTO for mode, _ in members):
        return ROWS, rows_form(n_bins, n_total, sum(grid), waves)
    return SLABS, slab_form(n_total, sum(grid), waves)


def forward_fit(lib, n_bins, members, grid):
    """(status, form, LDS bytes) of tc_debug_joint_interp_forward_fit."""
    n = len(members)
    mode = (ctypes.c_int * n)(*[m for m, _ in members])
    n_r = (ctypes.c_int * n)(*[r for _, r in members])
    n_axis = (ctypes.c_int * len(grid))(*grid)
    form, got = ctypes.c_int(-1), ctypes.c_int64(-1)
    status = lib.tc_debug_joint_interp_forward_fit(n_bins, n, mode, n_r, len(grid), n_axis,
                                                   ctypes.byref(form), ctypes.byref(got))
    return status, form.value, got.value


def test_library_exports_the_forward_symbols(lib):
    """Declared in the headers, present in the ctypes table and exported by the library; the entry
    of every (form, route) comes from FORWARD_ENTRIES, and there is no asynchronous one."""
    from tabcorr_amd import _lib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    declared = entry.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert {_lib.FORWARD_ENTRIES['joint_interp', form, route]
            for form in ('predict', 'chi2') for route in ('host', 'device')} == set(NEW_SYMBOLS[:4])
    assert not [key for key in _lib.FORWARD_ENTRIES
                if key[0] == 'joint_interp' and key[2] == 'async']
    # the argument order is that of the gradient entries with the derivative outputs removed
    for form in ('predict', 'chi2'):
        for suffix in ('', '_device'):
            grad = _lib.SIGNATURES['tc_joint_interp_%s_grad_batch%s' % (form, suffix)]
            keep = len(grad) - (2 if form == 'predict' else 3)
            assert _lib.SIGNATURES['tc_joint_interp_%s_batch%s' % (form, suffix)] == grad[:keep]


def test_lds_budgets_have_their_closed_forms(lib):
    from tabcorr_amd import _lib
    got = ctypes.c_int64(-1)
    for n_bins, members, grid in SHAPES:
        n_total = sum(r for _, r in members)
        form, expect = closed_form(n_bins, members, grid)
        for waves in (8, 16):
            for which, value in ((ROWS, rows_form(n_bins, n_total, sum(grid), waves)),
                                 (SLABS, slab_form(n_total, sum(grid), waves))):
                _lib.check(lib.tc_debug_joint_interp_forward_lds_bytes(
                    which, n_bins, n_total, sum(grid), waves, ctypes.byref(got)))
                assert got.value == value, (n_bins, members, grid, waves, which)
        assert forward_fit(lib, n_bins, members, grid) == (_lib.TC_OK, form, expect)
        assert expect <= LDS_LIMIT
    # the synthetic pair of the benchmark, 100 bins, N = 38, a 5 x 5 grid: 51200 + 18448 + 8192 +
    # 77824 bytes of joint_forward_kernel's regions and 6144 of weights and class norms
    assert closed_form(*BENCH_PAIR) == (ROWS, 161808)
    assert closed_form(*DS_EFFICIENT) == (SLABS, 8 * (4096 + 2306 + 1024 + 3072 + 384))
    for bad in ((2, 24, 8, 4, 8), (1, 0, 8, 4, 8), (1, 24, 0, 4, 8), (1, 24, 8, 3, 8),
                (1, 24, 8, 4, 7), (0, 24, 8, 4, 0), (0, 24, 8, 4, 18)):
        assert lib.tc_debug_joint_interp_forward_lds_bytes(
            *bad, ctypes.byref(got)) == _lib.TC_ERR_INVALID
    assert lib.tc_debug_joint_interp_forward_lds_bytes(1, 24, 8, 4, 8,
                                                       None) == _lib.TC_ERR_INVALID


def test_what_the_kernel_does_not_serve_is_refused_on_the_host(lib):
    """A mode-auto member of 21 r bins (a cross member of 21 is served) or of 249 bins (an
    all-cross joint of 249 is served), and a rows-form joint beyond the LDS budget -- by the
    formula: the largest served number of bins, then one more --: TC_ERR_UNSUPPORTED with a
    message, which Python raises as NotImplementedError."""
    from tabcorr_amd import _lib
    grid = (4, )
    assert forward_fit(lib, 24, [(AUTO, 20), (CROSS, 21)], grid)[0] == _lib.TC_OK
    status, _, _ = forward_fit(lib, 24, [(CROSS, 3), (AUTO, 21)], grid)
    assert status == _lib.TC_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match='member 1 .*21 correlation function bins'):
        _lib.check(status)
    # (248 bins of densities leave room for three rows)
    assert forward_fit(lib, 248, [(AUTO, 3)], grid)[0] == _lib.TC_OK
    assert forward_fit(lib, 249, [(CROSS, 3), (CROSS, 5)], grid)[:2] == (_lib.TC_OK, SLABS)
    status, _, _ = forward_fit(lib, 249, [(AUTO, 3)], grid)
    assert status == _lib.TC_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match='member 0 .*249 bins.*248'):
        _lib.check(status)
    # the pair of the benchmark with more and more bins
    _, members, grid = BENCH_PAIR
    n_bins = 100
    while rows_form(n_bins + 4, 38, sum(grid)) <= LDS_LIMIT:
        n_bins += 4
    assert rows_form(n_bins, 38, sum(grid)) <= LDS_LIMIT < rows_form(n_bins + 1, 38, sum(grid))
    assert forward_fit(lib, n_bins, members, grid) == (_lib.TC_OK, ROWS,
                                                       rows_form(n_bins, 38, sum(grid)))
    status, form, lds = forward_fit(lib, n_bins + 1, members, grid)
    assert (status, form, lds) == (_lib.TC_ERR_UNSUPPORTED, ROWS,
                                   rows_form(n_bins + 1, 38, sum(grid)))
    with pytest.raises(NotImplementedError, match='%d bytes of LDS' % lds):
        _lib.check(status)
    # many rows in the slab form: the precision matrix and the accumulators
    status, form, lds = forward_fit(lib, 24, [(CROSS, 100)] * 3, grid)
    assert (status, form) == (_lib.TC_ERR_UNSUPPORTED, SLABS)
    assert lds == slab_form(300, sum(grid))
    assert lds > LDS_LIMIT
    # the hook's own arguments
    one, r, axis = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(3), (ctypes.c_int * 1)(4)
    fit = lib.tc_debug_joint_interp_forward_fit
    assert fit(24, 1, None, r, 1, axis, None, None) == _lib.TC_ERR_INVALID
    assert fit(24, 17, one, r, 1, axis, None, None) == _lib.TC_ERR_INVALID
    assert fit(24, 1, (ctypes.c_int * 1)(2), r, 1, axis, None, None) == _lib.TC_ERR_INVALID
    assert fit(24, 1, one, r, 1, (ctypes.c_int * 1)(3), None, None) == _lib.TC_ERR_INVALID
    assert fit(24, 1, one, r, 0, axis, None, None) == _lib.TC_ERR_INVALID
    assert fit(24, 1, one, r, 1, axis, None, None) == _lib.TC_OK


def test_c_entry_points_refuse_a_call_without_a_handle(lib):
    from tabcorr_amd import _lib
    p = _lib.as_double_p(np.zeros(0))
    assert lib.tc_joint_interp_predict_batch(None, p, 5, p, 3, 10, 0, p, p) == _lib.TC_ERR_INVALID
    assert b'joint handle is NULL' in lib.tc_last_error()
    assert lib.tc_joint_interp_chi2_batch(None, p, 5, p, 3, 10, 0, p, p, p,
                                          p) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_interp_predict_batch_device(None, None, 5, None, 3, 10, 0, None,
                                                    None) == _lib.TC_ERR_INVALID
    assert lib.tc_joint_interp_chi2_batch_device(None, None, 5, None, 3, 10, 0, p, p, None,
                                                 None) == _lib.TC_ERR_INVALID
    # ... also an empty batch
    assert lib.tc_joint_interp_predict_batch(None, p, 5, p, 0, 10, 0, p, p) == _lib.TC_ERR_INVALID


def test_calls_refuse_wrong_arguments_before_any_device():
    from tabcorr_amd import Interpolator, JointInterpolator, TabCorr
    members = reference.make_members((4, ), 9, 1, [('auto', (3, )), ('cross', (5, ))])
    interpolators = []
    for tables, keys, points in members:
        halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'],
                                        t['attrs']) for t in tables]
        interpolators.append(Interpolator(halotabs,
                                          {key: points[:, d] for d, key in enumerate(keys)}))
    joint = JointInterpolator(interpolators)
    points = members[0][2]
    theta = synthetic.zheng07_draws(3, seed=2)
    x = np.tile(points.mean(axis=0), (3, 1))
    good_data, good_precision = np.zeros(8), np.eye(8)
    for data, precision in ((np.zeros(7), good_precision), (np.zeros((8, 2)), good_precision),
                            ([np.zeros(3), np.zeros(4)], good_precision),
                            (good_data, np.eye(5)), (good_data, np.ones((8, 9))),
                            (good_data, np.ones(64))):
        with pytest.raises(ValueError, match='data'):
            joint.chi2_batch(theta, x, data, precision)
    for columns in (4, 7):
        with pytest.raises(ValueError, match='theta'):
            joint.predict_batch(np.zeros((3, columns)), x)
        with pytest.raises(ValueError, match='theta'):
            joint.chi2_batch(np.zeros((3, columns)), x, good_data, good_precision)
    with pytest.raises(ValueError, match='theta'):
        joint.predict_batch(theta, x, assembias=True)
    for bad_x in (x[:2], np.hstack([x, x]), np.zeros((3, 0))):
        with pytest.raises(ValueError, match='x must have shape'):
            joint.predict_batch(theta, bad_x)
        with pytest.raises(ValueError, match='x must have shape'):
            joint.chi2_batch(theta, bad_x, good_data, good_precision)
    for value in (points.min() - 0.01, points.max() + 0.01, np.nan):
        outside = x.copy()
        outside[1, 0] = value
        with pytest.raises(ValueError, match='extrapolation'):
            joint.predict_batch(theta, outside)
        with pytest.raises(ValueError, match='extrapolation'):
            joint.chi2_batch(theta, outside, good_data, good_precision)
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.predict_batch(np.zeros((3, 14)), x, family='leauthaud11')
    with pytest.raises(NotImplementedError, match='Zheng07'):
        joint.chi2_batch(np.zeros((3, 14)), x, good_data, good_precision, family='leauthaud11')
    with pytest.raises(ValueError, match='family'):
        joint.chi2_batch(theta, x, good_data, good_precision, family='zu_mandelbaum15')
    assert joint._device is None
    for interp in interpolators:
        assert interp._device is None
        assert all(halotab._device is None for halotab in interp.tabcorr_list)
