"""ctypes binding of libtabcorr_hip.so (C ABI: include/tabcorr_amd.h).

The library is the only compute backend.  If it is missing, or if no gfx950
device is usable, the product path raises -- there is deliberately no CPU
fallback.
"""

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBRARY = os.path.join(HERE, 'libtabcorr_hip.so')

TC_OK = 0
TC_ERR_INVALID = 1
TC_ERR_HIP = 2
TC_ERR_UNSUPPORTED = 3
TC_ERR_RCCL = 4

MODE = {'auto': 0, 'cross': 1}
DTYPE_F64 = 0
DTYPE_F32 = 1

FLAG_SEPARATE_GAL_TYPE = 1
FLAG_MODULATE_WITH_CENOCC = 2
FLAG_ASSEMBIAS = 4
FLAG_LEAUTHAUD11 = 16

UNIQUE_ID_BYTES = 128

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int_p = ctypes.POINTER(ctypes.c_int)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_int64_p = ctypes.POINTER(ctypes.c_int64)
c_uint8_p = ctypes.POINTER(ctypes.c_uint8)
c_float_p = ctypes.POINTER(ctypes.c_float)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)

# name -> (argtypes); every function returns int except tc_last_error.
SIGNATURES = {
    'tc_device_count': [c_int_p],
    'tc_set_device': [ctypes.c_int],
    'tc_get_device': [c_int_p],
    'tc_runtime_version': [c_int_p],
    'tc_device_name': [ctypes.c_char_p, ctypes.c_size_t],
    'tc_device_synchronize': [],
    'tc_device_malloc': [c_void_pp, ctypes.c_size_t],
    'tc_device_free': [ctypes.c_void_p],
    'tc_memcpy_h2d': [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t],
    'tc_memcpy_d2h': [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t],
    'tc_host_alloc': [c_void_pp, ctypes.c_size_t],
    'tc_host_free': [ctypes.c_void_p],
    'tc_host_register': [ctypes.c_void_p, ctypes.c_size_t],
    'tc_host_unregister': [ctypes.c_void_p],
    'tc_host_is_pinned': [ctypes.c_void_p, ctypes.c_size_t, c_int_p],
    'tc_gauss_legendre': [ctypes.c_int, c_double_p, c_double_p],
    'tc_debug_fastmath': [ctypes.c_int, ctypes.c_int64, c_double_p,
                          c_double_p],
    'tc_debug_fastmath_device': [ctypes.c_int, ctypes.c_int64, c_double_p,
                                 c_double_p],
    'tc_debug_grad_operand': [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p],
    'tc_debug_grad_lds': [ctypes.c_int] * 7 + [c_int64_p],
    'tc_debug_interp_grad_lds_bytes': [ctypes.c_int] * 7 + [c_int64_p],
    'tc_debug_grad_slab': [ctypes.c_int] * 4 + [ctypes.c_int64, c_int64_p],
    'tc_debug_sync_chunks': [ctypes.c_int64] * 3 + [c_int_p, ctypes.c_int, ctypes.c_uint,
                                                    c_int_p, c_int64_p, c_int_p],
    'tc_debug_leauthaud11_node_grad': [c_double_p, ctypes.c_int, ctypes.c_int64, c_double_p,
                                       c_double_p, c_double_p, c_double_p, c_double_p,
                                       c_double_p],
    'tc_pair_indices': [ctypes.c_int, c_int32_p, c_int32_p, c_int32_p],
    'tc_spline_interpolation_matrix': [ctypes.c_int, c_double_p, c_double_p],
    'tc_spline_weights': [ctypes.c_int, c_double_p, c_double_p, ctypes.c_double, c_double_p,
                          c_double_p, c_int_p],
    'tc_plan_debug': [ctypes.c_int, ctypes.c_int, c_uint8_p, ctypes.c_int,
                      c_int64_p, c_int32_p, c_int32_p, c_int32_p],
    'tc_debug_triangle_parts': [ctypes.c_int, ctypes.c_int, c_int_p, c_int_p, c_int_p],
    'tc_debug_central_series': [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                ctypes.c_int64, c_double_p, c_double_p, c_double_p, c_double_p,
                                c_int32_p],
    'tc_debug_satellite_series': [ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_double, ctypes.c_int64, c_double_p, c_double_p,
                                  c_double_p, c_double_p, c_double_p, c_int32_p],
    'tc_debug_node_groups': [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p,
                             c_int32_p, c_int32_p, c_int_p, c_int_p],
    'tc_debug_quad_schedule': [ctypes.c_int] * 10 + [c_int_p, c_int_p, c_int_p,
                                                     c_int64_p, c_int64_p],
    'tc_debug_fused_form': [ctypes.c_int] * 5 + [ctypes.c_int64, ctypes.c_int, ctypes.c_uint,
                                                 ctypes.c_uint, c_int_p, c_int_p,
                                                 c_float_p, c_int_p, c_int_p,
                                                 c_int_p],
    'tc_debug_pair_plan': [c_double_p, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
                           ctypes.c_int, ctypes.c_int, c_int32_p, c_int32_p, c_int32_p,
                           c_int32_p, c_int64_p],
    'tc_debug_quad_emulate': [ctypes.c_int, ctypes.c_int, c_double_p, c_uint8_p,
                              ctypes.c_int, ctypes.c_int, c_double_p,
                              ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                              ctypes.c_int, ctypes.c_int, c_double_p],
    'tc_table_create': [
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
        ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, c_double_p,
        c_double_p, c_double_p, c_uint8_p, ctypes.c_int, c_void_pp],
    'tc_table_destroy': [ctypes.c_void_p],
    'tc_table_autotune_result': [ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, c_int_p,
                                 c_int64_p, c_int_p, c_float_p],
    'tc_table_batch_invariant': [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, c_int_p],
    'tc_set_copy_threads': [ctypes.c_int, ctypes.c_int],
    'tc_table_resident_stats': [ctypes.c_void_p, c_int64_p, c_int64_p, c_int64_p, c_int_p],
    'tc_table_synchronize': [ctypes.c_void_p],
    'tc_table_info': [ctypes.c_void_p, c_int_p, c_int_p, c_int_p, c_int64_p,
                      c_int_p, c_int64_p],
    'tc_mean_occupation_zheng07_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, c_double_p],
    'tc_predict_zheng07_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p],
    'tc_predict_zheng07_batch_device': [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p],
    'tc_chi2_zheng07_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p, c_double_p,
        c_double_p],
    'tc_chi2_zheng07_batch_device': [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p, ctypes.c_void_p,
        ctypes.c_void_p],
    'tc_predict_zheng07_many': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p],
    'tc_predict_zheng07_joint': [
        ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, c_double_p, ctypes.c_int,
        ctypes.c_int, ctypes.c_uint, c_double_p, ctypes.POINTER(c_double_p)],
    'tc_predict_zheng07_batch_async': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p, c_int64_p],
    'tc_chi2_zheng07_batch_async': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p, c_double_p,
        c_double_p, c_int64_p],
    'tc_table_wait': [ctypes.c_void_p, ctypes.c_int64],
    'tc_table_query': [ctypes.c_void_p, ctypes.c_int64, c_int_p],
    'tc_interp_predict_zheng07_batch_async': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p,
        c_int64_p],
    'tc_interp_chi2_zheng07_batch_async': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p,
        c_double_p, c_double_p, c_int64_p],
    'tc_interp_wait': [ctypes.c_void_p, ctypes.c_int64],
    'tc_interp_query': [ctypes.c_void_p, ctypes.c_int64, c_int_p],
    'tc_predict_occupation_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int64, ctypes.c_uint,
        c_double_p, c_double_p],
    'tc_interp_create': [c_void_pp, ctypes.c_int, ctypes.c_int, c_double_p,
                         c_void_pp],
    'tc_interp_destroy': [ctypes.c_void_p],
    'tc_interp_synchronize': [ctypes.c_void_p],
    'tc_interp_axis': [ctypes.c_void_p, ctypes.c_int, c_int_p, c_double_p,
                       ctypes.c_int],
    'tc_interp_info': [ctypes.c_void_p, c_int_p, c_int_p, c_int_p, c_int_p],
    'tc_debug_interp_vjp_lds_bytes': [ctypes.c_int] * 4 + [c_int64_p],
    'tc_interp_predict_zheng07_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p],
    'tc_interp_predict_zheng07_batch_device': [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p,
        ctypes.c_void_p],
    'tc_interp_chi2_zheng07_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p,
        c_double_p, c_double_p],
    'tc_interp_chi2_zheng07_batch_device': [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p,
        ctypes.c_void_p, ctypes.c_void_p],
    # joint of tables
    'tc_joint_create': [c_void_pp, ctypes.c_int, c_void_pp],
    'tc_joint_destroy': [ctypes.c_void_p],
    'tc_joint_synchronize': [ctypes.c_void_p],
    'tc_joint_info': [ctypes.c_void_p, c_int_p, c_int_p, c_int_p],
    'tc_debug_joint_lds_bytes': [ctypes.c_int] * 5 + [c_int64_p],
    # ... its forward entries: a table's without the `_zheng07` (the family is in the flags)
    'tc_joint_predict_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p],
    'tc_joint_predict_batch_device': [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p],
    'tc_joint_chi2_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p, c_double_p,
        c_double_p],
    'tc_joint_chi2_batch_device': [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p, ctypes.c_void_p,
        ctypes.c_void_p],
    'tc_debug_joint_forward_lds_bytes': [ctypes.c_int] * 3 + [c_int64_p],
    'tc_debug_joint_vjp_lds_bytes': [ctypes.c_int] * 3 + [c_int64_p],
    'tc_debug_joint_forward_fit': [ctypes.c_int, ctypes.c_int, c_int_p, c_int_p, c_int_p,
                                   c_int64_p],
    # joint of interpolators
    'tc_joint_interp_create': [c_void_pp, ctypes.c_int, c_void_pp],
    'tc_joint_interp_destroy': [ctypes.c_void_p],
    'tc_joint_interp_synchronize': [ctypes.c_void_p],
    'tc_joint_interp_info': [ctypes.c_void_p, c_int_p, c_int_p, c_int_p, c_int_p],
    'tc_debug_joint_interp_lds_bytes': [ctypes.c_int] * 7 + [c_int64_p],
    # ... its forward entries: an interpolator's without the `_zheng07`
    'tc_joint_interp_predict_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p],
    'tc_joint_interp_predict_batch_device': [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p,
        ctypes.c_void_p],
    'tc_joint_interp_chi2_batch': [
        ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p,
        c_double_p, c_double_p],
    'tc_joint_interp_chi2_batch_device': [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int64, ctypes.c_int, ctypes.c_uint, c_double_p, c_double_p,
        ctypes.c_void_p, ctypes.c_void_p],
    'tc_debug_joint_interp_forward_lds_bytes': [ctypes.c_int] * 5 + [c_int64_p],
    'tc_debug_joint_interp_forward_fit': [ctypes.c_int, ctypes.c_int, c_int_p, c_int_p,
                                          ctypes.c_int, c_int_p, c_int_p, c_int64_p],
    'tc_table_set_option': [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int],
    'tc_table_timer_begin': [ctypes.c_void_p, ctypes.c_int],
    'tc_table_timer_end': [ctypes.c_void_p, c_float_p],
    'tc_table_kernel_time': [ctypes.c_void_p, c_int_p, c_float_p],
    'tc_debug_trace': [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                       ctypes.c_int64, c_int64_p],
    'tc_debug_wave_trace': [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                            ctypes.c_int64, c_int64_p],
    'tc_debug_resident_ticks': [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                ctypes.c_int64, c_int64_p],
    'tc_debug_ensemble_stamps': [ctypes.c_void_p,
                                 ctypes.POINTER(ctypes.c_uint64)],
    'tc_table_last_launch': [ctypes.c_void_p, c_int_p, c_int_p, c_int_p,
                             c_int_p],
    'tc_pair_count_rppi': [c_double_p, ctypes.c_int64, c_double_p,
                           ctypes.c_int64, c_double_p, c_double_p, ctypes.c_int,
                           ctypes.c_double, ctypes.c_int,
                           ctypes.POINTER(ctypes.c_uint64)],
    'tc_pair_count_smu': [c_double_p, ctypes.c_int64, c_double_p,
                          ctypes.c_int64, c_double_p, c_double_p, ctypes.c_int,
                          ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)],
    'tc_pair_count_rppi_labelled': [c_double_p, c_int32_p, ctypes.c_int64,
                                    c_double_p, c_int32_p, ctypes.c_int64,
                                    ctypes.c_int, c_double_p, c_double_p,
                                    ctypes.c_int, ctypes.c_double,
                                    ctypes.POINTER(ctypes.c_uint64)],
    'tc_pair_count_smu_labelled': [c_double_p, c_int32_p, ctypes.c_int64,
                                   c_double_p, c_int32_p, ctypes.c_int64,
                                   ctypes.c_int, c_double_p, c_double_p,
                                   ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_uint64)],
    'tc_mass_in_cylinders': [c_double_p, ctypes.c_int64, c_double_p,
                             ctypes.c_int64, c_double_p, c_double_p, c_double_p,
                             ctypes.c_int, c_double_p],
    'tc_comm_unique_id': [ctypes.c_void_p],
    'tc_comm_create': [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                       c_void_pp],
    'tc_comm_destroy': [ctypes.c_void_p],
    'tc_comm_gather': [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                       ctypes.c_int],
    'tc_comm_release': [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int],
    'tc_comm_gather_interp': [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                              ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                              ctypes.c_int],
    'tc_comm_release_interp': [ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_int],
    'tc_comm_barrier': [ctypes.c_void_p],
    'tc_comm_synchronize': [ctypes.c_void_p],
}

# The gradient entries: (handle kind, family, form) -> the host-array symbol; the device-pointer
# twin is `name + '_device'`.  Forms: 'predict' (ngal, xi, dngal, dxi), 'chi2' (ngal, chi2, dngal,
# dchi2) and 'fisher' (the same with the Fisher matrix).  Plain Zheng07 has an entry of its own
# for the Fisher matrix; the other families and the joints (whose family is in the flags) take a
# trailing `fisher` that may be None.  A joint of interpolators takes x as an interpolator does.
GRAD_ENTRIES = {}
for _kind, _prefix, _families in (('table', 'tc_', ('zheng07', 'assembias', 'leauthaud11')),
                                  ('interp', 'tc_interp_', ('zheng07', 'assembias', 'leauthaud11')),
                                  ('joint', 'tc_joint_', (None, )),
                                  ('joint_interp', 'tc_joint_interp_', (None, ))):
    for _family in _families:
        _stem = '' if _family is None else '_' + _family
        for _form, _entry in (('predict', 'predict_grad'), ('chi2', 'chi2_grad'),
                              ('fisher', 'chi2_fisher' if _family == 'zheng07' else 'chi2_grad')):
            for _key in ('zheng07', 'assembias') if _family is None else (_family, ):
                GRAD_ENTRIES[_kind, _key, _form] = '%s%s%s_batch' % (_prefix, _entry, _stem)
GRAD_OPTIONAL_FISHER = {GRAD_ENTRIES[_key] for _key in GRAD_ENTRIES if _key[2] == 'chi2' and
                        GRAD_ENTRIES[_key] == GRAD_ENTRIES[_key[:2] + ('fisher', )]}


# The forward entries: (handle kind, form, route) -> symbol.
FORWARD_ENTRIES = {
    (_kind, _form, _route): 'tc_%s%s_zheng07_batch%s' % (_prefix, _form, _suffix)
    for _kind, _prefix in (('table', ''), ('interp', 'interp_'))
    for _form in ('predict', 'chi2')
    for _route, _suffix in (('host', ''), ('device', '_device'), ('async', '_async'))}
# (the joints, of tables and of interpolators: the family is in the flags, and there are no
# asynchronous entries)
FORWARD_ENTRIES.update({
    (_kind, _form, _route): 'tc_%s_%s_batch%s' % (_kind, _form, _suffix)
    for _kind in ('joint', 'joint_interp')
    for _form in ('predict', 'chi2')
    for _route, _suffix in (('host', ''), ('device', '_device'))})


# The occupation seam: (handle kind, form) -> the host-array symbol, `name + '_device'` its
# twin.  Form 'predict': cotangents (g_ngal, g_xi) in, (ngal, xi, g_occupation) out; 'chi2':
# (data, precision) in, (ngal, chi2, dchi2_docc) out.  An interpolator takes x behind the
# occupations and has SEAM_X_OUTPUTS more outputs: g_x, or dchi2_dx and dngal_dx.  A joint and an
# interpolator take NULL for the derivative outputs (the forward-only form); a table does not.
SEAM_ENTRIES = {
    (_kind, _form): 'tc_%s%s_batch' % (_prefix, _entry)
    for _kind, _prefix in (('table', ''), ('joint', 'joint_'), ('interp', 'interp_'))
    for _form, _entry in (('predict', 'predict_occupation_vjp'),
                          ('chi2', 'chi2_occupation_grad'))}
SEAM_X_OUTPUTS = {'predict': 1, 'chi2': 2}


def _derivative_signatures():
    """The argument lists of the derivative entries, composed: the handle, the draws (and an
    interpolator's x), the counts and flags, the likelihood's operands (host pointers in both
    twins), four outputs and, where the entry has one, the Fisher matrix.  The occupation seam:
    the handle, the occupations (and an interpolator's x behind them), n_draws and flags, the
    cotangents or the operands, three outputs and, for an interpolator, those with respect to x
    last.  A `_device` twin takes device pointers for every array."""
    out = {}
    for device in (False, True):
        array = ctypes.c_void_p if device else c_double_p
        suffix = '_device' if device else ''
        for (kind, _, form), name in GRAD_ENTRIES.items():
            head = [ctypes.c_void_p, array, ctypes.c_int] + [array] * (kind in ('interp', 'joint_interp'))
            head += [ctypes.c_int64, ctypes.c_int, ctypes.c_uint]
            operands = [c_double_p, c_double_p] * (form != 'predict')
            fisher = [array] * (form == 'fisher' or name in GRAD_OPTIONAL_FISHER)
            out[name + suffix] = head + operands + [array] * 4 + fisher
        for (kind, form), name in SEAM_ENTRIES.items():
            interp = kind == 'interp'
            head = [ctypes.c_void_p, array] + [array] * interp + [ctypes.c_int64, ctypes.c_uint]
            middle = [array] * 2 if form == 'predict' else [c_double_p] * 2
            out[name + suffix] = head + middle + [array] * (3 + interp * SEAM_X_OUTPUTS[form])
    return out


SIGNATURES.update(_derivative_signatures())

_lib = None


class TabCorrHipError(RuntimeError):
    """The HIP backend failed (no device, launch error, RCCL error)."""


class Handle:
    """Owner of a handle of the library: `lib`, `handle`, and its destruction by the symbol
    `destroy` when the owner goes."""

    def __init__(self, lib, handle, destroy):
        self.lib = lib
        self.handle = handle
        self.destroy = destroy

    def __del__(self):
        handle = getattr(self, 'handle', None)
        if handle is not None and handle.value is not None:
            try:
                getattr(self.lib, self.destroy)(handle)
            except Exception:  # interpreter shutdown
                pass
            self.handle = None


def load():
    """Load the shared library (once) and declare every signature."""
    global _lib
    if _lib is not None:
        return _lib
    # developer A/B runs: TABCORR_AMD_LIBRARY points at another build of the library
    library = os.environ.get('TABCORR_AMD_LIBRARY') or LIBRARY
    if not os.path.exists(library):
        raise TabCorrHipError(
            'libtabcorr_hip.so is missing: build it with '
            '`python -m tabcorr_amd.build` (needs hipcc). There is no CPU '
            'fallback.')
    # RTLD_DEEPBIND + -z now: the library keeps the ROCm runtime it was linked
    # against even when another copy (e.g. the one bundled with PyTorch) is
    # already in the process.
    mode = os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, 'RTLD_DEEPBIND', 0)
    lib = ctypes.CDLL(library, mode=mode)
    lib.tc_last_error.restype = ctypes.c_char_p
    lib.tc_last_error.argtypes = []
    for name, argtypes in SIGNATURES.items():
        function = getattr(lib, name)
        function.restype = ctypes.c_int
        function.argtypes = argtypes
    _lib = lib
    return lib


def check(status):
    """Map a status code to the exception type the reference would raise."""
    if status == TC_OK:
        return
    message = load().tc_last_error().decode(errors='replace')
    if status == TC_ERR_INVALID:
        raise ValueError(message)
    if status == TC_ERR_UNSUPPORTED:
        raise NotImplementedError(message)
    raise TabCorrHipError(message)


def as_double_p(array):
    """Pointer to the first element of a C-contiguous float64 array for a
    ``c_double_p`` argument.  ``from_buffer`` + ``byref`` costs a third of
    ``array.ctypes.data_as`` (0.5 against 1.5 us, three of them per un-batched
    call); read-only and empty arrays take the slow way."""
    try:
        return ctypes.byref(ctypes.c_double.from_buffer(array))
    except (TypeError, ValueError, BufferError):
        return array.ctypes.data_as(c_double_p)


def device_count():
    lib = load()
    count = ctypes.c_int(0)
    status = lib.tc_device_count(ctypes.byref(count))
    if status != TC_OK:
        return 0
    return count.value


def require_device():
    """Raise unless a HIP device is usable."""
    lib = load()
    count = ctypes.c_int(0)
    check(lib.tc_device_count(ctypes.byref(count)))
    if count.value < 1:
        raise TabCorrHipError('no HIP device found; tabcorr_amd has no CPU '
                              'fallback')
    return count.value


def runtime_version():
    version = ctypes.c_int(0)
    check(load().tc_runtime_version(ctypes.byref(version)))
    return version.value


def device_name():
    buffer = ctypes.create_string_buffer(256)
    check(load().tc_device_name(buffer, 256))
    return buffer.value.decode()


def contiguous(array, dtype=np.float64):
    return np.ascontiguousarray(array, dtype=dtype)
