"""Records what the batch kernels return whose steps behind the sums -- spline weights, the
likelihood of a results tile, its write-out, the exchange of a tile's shares between workgroups,
the per-draw tail of the two mode-cross kernels, the two finalisation kernels -- are shared
through csrc/spline.h and csrc/epilogue.h or are candidates for it, on an MI355X, into
epilogue_parent.npz:
python tests/golden/make_epilogue_parent.py

Run it with the library of the commit whose bits are the reference (the parent of the change
that introduced the two headers); tests/test_gpu_epilogue.py then asks every later library for
the same bits.  `cases()` and `run_case()` are what that test evaluates too.  The cases are the
ones fused_walk_parent.npz and quad_walk_parent.npz leave out: the mode-cross one-launch forms
(register form, chunk form per instance with the deferred pairs on and off, the wide form for
few rows, interpolators), the three-kernel path of mode cross (finalize_kernel,
interp_coef_kernel), the three-kernel likelihood (finalize_quad_kernel) and the small
interpolator calls (interp_coef_small_kernel, the host's spline weights).

The file holds, per case, the (workgroups, waves, slabs, LDS bytes) of the launch and the
results as float64.  A case whose `base` runs the same table and draws in another form differs
from it in the last bits only (or, the degenerate cases, in a few draws) and is kept as the
exclusive-or with the base's words.
"""

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
FILE = os.path.join(HERE, 'epilogue_parent.npz')


def load_sibling():
    spec = importlib.util.spec_from_file_location(
        'make_fused_walk_parent', os.path.join(HERE, 'make_fused_walk_parent.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


fused = load_sibling()
N_DRAWS = fused.N_DRAWS             # 81: two tiles of 64 draws, the second partial
likelihood_of = fused.likelihood_of
# (the draws degenerate_draws replaces, in either tile)
DEGENERATE_ROWS = tuple(range(1, 13)) + tuple(range(65, 77))

FORCE = (('fused', 2), ('fused_min_draws', 1), ('single_draw', 0))     # one launch
THREE = (('fused', 0), ('single_draw', 0))                              # three kernels
DEFER_ON = (('series', 3), ('cross_defer', 1))
DEFER_OFF = (('series', 3), ('cross_defer', 0))
ONE_WORKGROUP = (('cross_target', 1), )


def cases():
    """(name, dict) of every recorded case, a case's base before it."""
    out = []

    def add(name, shape, **case):
        case['shape'] = shape           # (n_prim, n_sec, n_r)
        case['n_r'] = shape[2]
        for key, value in (('mode', 'cross'), ('grid', None), ('vary_n_h', False),
                           ('separate', False), ('chi2', False), ('degenerate', False),
                           ('dtype', 'float64'), ('assembias', False), ('modulate', False),
                           ('options', FORCE), ('per_tile', None), ('base', None)):
            case.setdefault(key, value)
        out.append((name, case))

    def both(name, shape, **case):
        base = case.pop('base', None)
        for separate in (False, True):
            tag = '_sep' if separate else '_tot'
            add(name + tag, shape, separate=separate, base=base + tag if base else None, **case)
    # the register form (up to 16 rows): several workgroups per tile, and one
    both('register', (20, 1, 13), form='register', per_tile='many')
    both('register_one', (20, 1, 13), form='register', per_tile='one',
         options=FORCE + ONE_WORKGROUP, base='register')
    both('register_assembias', (20, 2, 13), form='register', assembias=True)
    both('register_modulate', (9, 3, 5), form='register', modulate=True)
    add('register_chi2', (20, 1, 13), form='register', chi2=True)
    # the chunk form, one shape per instance, deferred pairs on and off
    for rows, shape in ((32, (9, 3, 19)), (64, (30, 2, 40))):
        both('chunk%d_on' % rows, shape, form='chunk', options=FORCE + DEFER_ON)
        both('chunk%d_off' % rows, shape, form='chunk', options=FORCE + DEFER_OFF,
             base='chunk%d_on' % rows)
    add('chunk128_tot', (10, 2, 100), form='chunk')
    both('chunk32_on_one', (9, 3, 19), form='chunk', per_tile='one',
         options=FORCE + DEFER_ON + ONE_WORKGROUP, base='chunk32_on')
    add('chunk32_off_one_tot', (9, 3, 19), form='chunk', per_tile='one',
        options=FORCE + DEFER_OFF + ONE_WORKGROUP, base='chunk32_on_tot')
    add('chunk32_on_chi2', (9, 3, 19), form='chunk', chi2=True, options=FORCE + DEFER_ON)
    add('chunk32_off_chi2', (9, 3, 19), form='chunk', chi2=True, options=FORCE + DEFER_OFF)
    # The launcher declines the deferred pairs for all of the above (run_cross_fused: groups of
    # three bins have no records; a separated call's second results area, and a tile of 40 r
    # values beside the math table, cost the second workgroup per CU): both settings record the
    # same bits there.  These shapes take them (two bins per group, total, a tile that fits the
    # math table's area) -- their LDS size shows it:
    for rows, shape in ((32, (9, 2, 19)), (64, (12, 2, 34))):
        add('chunk%d_deferred_tot' % rows, shape, form='chunk', options=FORCE + DEFER_ON)
        add('chunk%d_undeferred_tot' % rows, shape, form='chunk', options=FORCE + DEFER_OFF,
            base='chunk%d_deferred_tot' % rows)
    add('chunk32_deferred_chi2', (9, 2, 19), form='chunk', chi2=True, options=FORCE + DEFER_ON)
    add('chunk32_deferred_one_tot', (9, 2, 19), form='chunk', per_tile='one',
        options=FORCE + DEFER_ON + ONE_WORKGROUP, base='chunk32_deferred_tot')
    # few rows in the chunk form
    both('wide', (40, 2, 13), form='wide',
         options=FORCE + (('series', 3), ('cross_wide_min_draws', 1)))
    # interpolators over cross tables, one launch
    both('interp4', (20, 2, 13), form='interp', grid=(4, ))
    add('interp4_chi2', (20, 2, 13), form='interp', grid=(4, ), chi2=True)
    both('interp4x4', (10, 2, 3), form='interp', grid=(4, 4), vary_n_h=True)
    # degenerate draws: the rule for components whose norm is not finite
    add('register_degenerate_sep', (20, 1, 13), form='register', separate=True, degenerate=True,
        base='register_sep')
    add('chunk32_degenerate_sep', (9, 3, 19), form='chunk', separate=True, degenerate=True,
        options=FORCE + DEFER_ON, base='chunk32_on_sep')
    # three kernels, mode cross: finalize_kernel, interp_coef_kernel
    both('three_table', (20, 2, 13), form='three', options=THREE)
    both('three_interp4', (20, 2, 13), form='three', grid=(4, ), options=THREE, base='interp4')
    both('three_f32', (10, 2, 7), form='three', dtype='float32', options=THREE)
    # three kernels, mode auto, the likelihood: finalize_quad_kernel
    add('three_auto_chi2', (10, 1, 19), form='three', mode='auto', chi2=True, options=THREE)
    # un-batched calls and batches of three draws: the host's spline weights,
    # interp_coef_small_kernel
    add('small_cross4x4', (10, 2, 3), form='small', grid=(4, 4), vary_n_h=True, options=())
    add('small_auto4', (10, 1, 19), form='small', mode='auto', grid=(4, ), options=())
    return out


def table_of(case):
    from tabcorr_amd import synthetic
    n_prim, n_sec, n_r = case['shape']
    return synthetic.synthetic_table(n_prim, n_sec, (n_r, ), case['mode'], seed=n_prim + n_r)


def interpolator_of(case):
    """(tables, keys, points) of an interpolator case."""
    from tabcorr_amd import synthetic
    n_prim, n_sec, n_r = case['shape']
    tables, keys, points = synthetic.synthetic_interpolator(case['grid'], n_prim, n_sec, (n_r, ),
                                                            case['mode'], seed=n_prim)
    if case['vary_n_h']:        # (tables of different cosmologies: test_gpu_cross_fused.py)
        rng = np.random.default_rng(n_prim)
        for table in tables:
            table['gal_type'] = table['gal_type'].copy()
            table['gal_type']['n_h'] *= rng.uniform(0.8, 1.25, len(table['gal_type']))
    return tables, keys, points


def degenerate_draws(theta):
    """test_gpu_grouped.py: degenerate_draws, in either tile."""
    theta = theta.copy()
    for first in (0, 64):
        rows = theta[first:]
        rows[1, 0] = np.nan
        rows[2, 1] = 0.0
        rows[3, 1] = np.nan
        rows[4, 2] = np.nan
        rows[5, 3] = np.nan
        rows[6, 4] = np.nan
        rows[7, 3] = -400.0
        rows[8, 2] = 400.0
        rows[9, 0] = np.inf
        rows[10, 0] = -np.inf
        rows[11, :5] = [12.0, 0.0, 11.0, 13.0, 1.0]      # a step exactly on a bin edge
        rows[12, 2] = 15.5
    return theta


def theta_of(case):
    from tabcorr_amd import synthetic
    n_draws = 3 if case['form'] == 'small' else N_DRAWS
    theta = synthetic.zheng07_draws(n_draws, seed=N_DRAWS + case['shape'][0])
    return degenerate_draws(theta) if case['degenerate'] else theta


def strengths_of(case):
    """The assembly-bias strengths of a decorated case's draws."""
    return np.random.default_rng(case['n_r']).uniform(-1.2, 1.2, (N_DRAWS, 2))


def x_of(case, points):
    """The draws' coordinates on the interpolator's axes.  81 draws: 10 % beyond either end, draw
    3 on the right edge, draw 4 on the left (test_gpu_cross_fused.py: test_cross_interpolator).
    Three draws: inside the grid, on the right edge, outside."""
    xp = [np.unique(points[:, d]) for d in range(points.shape[1])]
    if case['form'] == 'small':
        return np.array([[0.6 * a[1] + 0.4 * a[2] for a in xp], [a[-1] for a in xp],
                         [a[-1] + 0.1 * (a[-1] - a[0]) for a in xp]])
    rng = np.random.default_rng(case['n_r'])
    x = np.stack([rng.uniform(a[0] - 0.1 * (a[-1] - a[0]), a[-1] + 0.1 * (a[-1] - a[0]), N_DRAWS)
                  for a in xp], axis=-1)
    x[3] = [a[-1] for a in xp]
    x[4] = [a[0] for a in xp]
    return x


def launch_is_the_form(case, launch):
    """Whether (workgroups, waves, slabs, LDS bytes) is a launch of the case's form, as far as one
    launch tells (the LDS sizes of the forms are compared between cases by the test)."""
    workgroups, waves, slabs, _ = (int(v) for v in launch)
    tiles = ((3 if case['form'] == 'small' else N_DRAWS) + 63) // 64
    if case['form'] in ('three', 'small'):
        # The launch is the contraction's.  Mode auto: contract_quad_kernel (kernel_args.h:
        # kQuadWavesPerBlock waves), which finalize_quad_kernel follows; mode cross: the segment
        # kernels, a workgroup per (slab, tile of 64 draws), which finalize_kernel follows.
        # (Three draws take interp_coef_small_kernel, 81 interp_coef_kernel: inst_quad.hip.)
        if case['mode'] == 'auto':
            return slabs > 0 and waves == 4 and workgroups != slabs * tiles
        return slabs > 0 and waves < 4 and workgroups == slabs * tiles
    if waves != 8 or slabs != 0 or workgroups % tiles != 0:
        return False
    per_tile = workgroups // tiles
    return {'one': per_tile == 1, 'many': 1 < per_tile <= 8, None: 1 <= per_tile <= 8}[
        case['per_tile']]


def run_case(case):
    """The case on the device: {'launch': (workgroups, waves, slabs, LDS bytes), name: float64
    array}."""
    import ctypes
    from tabcorr_amd import Interpolator, TabCorr, Zheng07Model, synthetic, _lib
    lib = _lib.load()

    def make(table):
        return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                   table['attrs'], compute_dtype=case['dtype'])
    if case['grid'] is not None:
        tables, keys, points = interpolator_of(case)
        halotabs = [make(table) for table in tables]
        interpolator = Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)})
        x = x_of(case, points)
    else:
        halotabs = [make(table_of(case))]
    for halotab in halotabs:
        for key, value in case['options']:
            _lib.check(lib.tc_table_set_option(halotab.to_device().handle, key.encode(), value))
    theta = theta_of(case)
    kwargs = {}
    if case['assembias']:
        theta = np.hstack([theta, strengths_of(case)])
        kwargs['assembias'] = True
    if case['modulate']:
        kwargs['modulate_with_cenocc'] = True
    out = {}

    def keep(ngal, xi, tag=''):
        if isinstance(ngal, dict):
            for key in ngal:
                out['ngal_' + key + tag] = ngal[key]
            for key in xi:
                out['xi_' + key + tag] = xi[key]
        else:
            out['ngal' + tag], out['xi' + tag] = ngal, xi
    with np.errstate(all='ignore'):
        if case['form'] == 'small':
            for i in range(3):          # un-batched: the host's spline weights
                model = Zheng07Model(redshift=tables[0]['attrs']['redshift'])
                for key, value in zip(synthetic.ZHENG07_KEYS, theta[i]):
                    model.param_dict[key] = value
                for key, value in zip(keys, x[i]):
                    model.param_dict[key] = value
                keep(*interpolator.predict(model, extrapolate=True, check_consistency=False),
                     tag='_one%d' % i)
            keep(*interpolator.predict_batch(theta, x, extrapolate=True))
            keep(*interpolator.predict_batch(theta, x, separate_gal_type=True, extrapolate=True))
        elif case['chi2']:
            likelihood = likelihood_of(case)
            if case['grid'] is not None:
                out['ngal'], out['chi2'] = interpolator.chi2_batch(theta, x, *likelihood,
                                                                   extrapolate=True, **kwargs)
            else:
                out['ngal'], out['chi2'] = halotabs[0].chi2_batch(theta, *likelihood, **kwargs)
        elif case['grid'] is not None:
            keep(*interpolator.predict_batch(theta, x, separate_gal_type=case['separate'],
                                             extrapolate=True, **kwargs))
        else:
            keep(*halotabs[0].predict_batch(theta, separate_gal_type=case['separate'], **kwargs))
    launch = [ctypes.c_int() for _ in range(4)]
    _lib.check(lib.tc_table_last_launch(halotabs[0].to_device().handle,
                                        *[ctypes.byref(v) for v in launch]))
    out = {key: np.ascontiguousarray(value, dtype=np.float64) for key, value in out.items()}
    out['launch'] = np.array([v.value for v in launch], dtype=np.int64)
    assert launch_is_the_form(case, out['launch']), \
        'not the form asked for (%s): %s' % (case['form'], out['launch'])
    return out


def pack(results):
    """{case: {key: array}} -> the arrays of the file."""
    bases = {name: case['base'] for name, case in cases()}
    arrays = {}
    for name, result in results.items():
        base = results[bases[name]] if bases[name] else None
        for key, value in result.items():
            if key == 'launch' or base is None:
                arrays[name + '/' + key] = value
            else:
                arrays[name + '/' + key + '^'] = value.view(np.uint64) ^ base[key].view(np.uint64)
    return arrays


def unpack(data):
    """The arrays of the file -> {case: {key: array}}."""
    results = {}
    for name, case in cases():
        result = {}
        for full in data.files:
            if not full.startswith(name + '/'):
                continue
            key = full[len(name) + 1:]
            if key.endswith('^'):
                key = key[:-1]
                result[key] = (data[full] ^ results[case['base']][key].view(np.uint64)
                               ).view(np.float64)
            else:
                result[key] = data[full]
        results[name] = result
    return results


if __name__ == '__main__':
    sys.path.insert(0, REPO)
    results = {}
    for name, case in cases():
        results[name] = run_case(case)
        print(name, results[name]['launch'], flush=True)
    target = sys.argv[1] if len(sys.argv) > 1 else FILE
    np.savez_compressed(target, **pack(results))
    again = unpack(np.load(target))
    for name, result in results.items():
        for key, value in result.items():
            assert np.array_equal(again[name][key].view(np.uint64), value.view(np.uint64)), name
    print('%s: %d cases, %d bytes' % (target, len(results), os.path.getsize(target)))
