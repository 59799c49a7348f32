"""Records what the kernels that share the schedule of csrc/fused_walk.h besides the 64-draw and
32-draw one-launch forms return -- contract_quad_kernel, contract_quad_f32_kernel and the latency
form's fused_quad_pass40 --, on an MI355X, into quad_walk_parent.npz:
python tests/golden/make_quad_walk_parent.py

Run it with the library of the commit whose bits are the reference (the parent of the change
that moved the two contract kernels onto the shared walk); tests/test_gpu_quad_walk.py then asks every later library for the same bits.  `cases()`
and `run_case()` are what that test evaluates too; tables, draws and the likelihood are those of
make_fused_walk_parent.py.

The file holds, per case, the (workgroups, waves, slabs) of the launch and the results as
float64.  Where the same table and draws are recorded for the float64 three-kernel path too, the
latency form's results (which differ from it in their last bits only) and the float32 ones (in
the lower half of the word) are kept as the exclusive-or with its words.  The separated cases
are the ones that walk rectangles (the cen-sat component) and cost three times a total case's
bytes: they cover every U of either kernel and leave out the shapes that repeat one (n_prim 4 and
5, (50, 19), (10, 40); float32: one n_prim per n_r).
"""

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
FILE = os.path.join(HERE, 'quad_walk_parent.npz')


def load_sibling():
    spec = importlib.util.spec_from_file_location(
        'make_fused_walk_parent', os.path.join(HERE, 'make_fused_walk_parent.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


fused = load_sibling()
N_DRAWS = fused.N_DRAWS             # 81: a partial last tile at 32, 40 and 64 draws per tile
DEGENERATE_ROWS = fused.DEGENERATE_ROWS
theta_of, likelihood_of = fused.theta_of, fused.likelihood_of

# three kernels (option fused = 0), float64: U = 1 ... 5 and 2 ... 25 block rows; two r tiles
SHAPES_F64 = [(4, 19), (5, 19), (10, 19), (50, 3), (50, 8), (50, 12), (50, 16), (50, 19), (10, 40)]
SEPARATED_F64 = [(10, 19), (50, 3), (50, 8), (50, 12), (50, 16)]
# ... on float32 tables: U = 1 ... 4, and 19 r values = two r tiles
SHAPES_F32 = [(n_prim, n_r) for n_prim in (10, 50) for n_r in (3, 7, 12, 16, 19)]
SEPARATED_F32 = [(50, 3), (10, 7), (50, 12), (50, 16)]
# interpolator, mode auto, a 1-D grid of four tables: (n_prim, n_r, dtype)
INTERPOLATORS = [(10, 19, 'float64'), (10, 12, 'float32')]
# the latency form (option fused_draws = 40): the five load patterns of fused_quad_pass40
SHAPES_40 = [(n_prim, n_r) for n_prim in (4, 10, 50) for n_r in (3, 8, 12, 16, 19)]


def cases():
    """(name, dict) of every recorded case, a case's base before it."""
    out = []

    def add(name, **case):
        case.setdefault('separate', False)
        case.setdefault('degenerate', False)
        case.setdefault('dtype', 'float64')
        case.setdefault('base', None)
        out.append((name, case))
    for dtype, shapes, separated in (('float64', SHAPES_F64, SEPARATED_F64),
                                     ('float32', SHAPES_F32, SEPARATED_F32)):
        tag = 'f64' if dtype == 'float64' else 'f32'
        for n_prim, n_r in shapes:
            for separate in (False, True) if (n_prim, n_r) in separated else (False, ):
                name = 'three_%%s_p%d_r%d_%s' % (n_prim, n_r, 'sep' if separate else 'tot')
                in_f64 = (n_prim, n_r) in (SEPARATED_F64 if separate else SHAPES_F64)
                add(name % tag, kind='three', n_prim=n_prim, n_r=n_r, dtype=dtype,
                    separate=separate,
                    base=name % 'f64' if dtype == 'float32' and in_f64 else None)
    for n_prim, n_r, dtype in INTERPOLATORS:
        add('interp_%s_p%d_r%d' % ('f64' if dtype == 'float64' else 'f32', n_prim, n_r),
            kind='interp', n_prim=n_prim, n_r=n_r, dtype=dtype)
    for n_prim, n_r in SHAPES_40:
        add('latency_p%d_r%d' % (n_prim, n_r), kind='latency', n_prim=n_prim, n_r=n_r,
            base='three_f64_p%d_r%d_tot' % (n_prim, n_r) if (n_prim, n_r) in SHAPES_F64 else None)
    add('latency_chi2_p50_r19', kind='latency_chi2', n_prim=50, n_r=19)
    add('latency_degenerate_p10_r19', kind='latency', n_prim=10, n_r=19, degenerate=True)
    return out


def table_of(case):
    return fused.table_of(case)


def interpolator_of(case):
    """(tables, keys, points) of an interpolator case."""
    from tabcorr_amd import synthetic
    return synthetic.synthetic_interpolator((4, ), case['n_prim'], 1, (case['n_r'], ), 'auto',
                                            seed=case['n_prim'] + case['n_r'])


def x_of(case, points):
    """The draws' coordinates on the interpolator's axis, inside the grid."""
    rng = np.random.default_rng(N_DRAWS + case['n_r'])
    return rng.uniform(points.min(), points.max(), size=(N_DRAWS, 1))


def run_case(case):
    """The case on the device: {'launch': (workgroups, waves, slabs), name: float64 array}."""
    import ctypes
    from tabcorr_amd import Interpolator, TabCorr, _lib
    lib = _lib.load()

    def make(table):
        return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                   table['attrs'], compute_dtype=case['dtype'])
    latency = case['kind'].startswith('latency')
    options = [('fused', 2), ('fused_min_draws', 1), ('single_draw', 0), ('fused_draws', 40),
               ('sync_chunks', 1)] if latency else [('fused', 0), ('single_draw', 0)]
    if case['kind'] == 'interp':
        tables, keys, points = interpolator_of(case)
        halotabs = [make(table) for table in tables]
        interpolator = Interpolator(halotabs, {key: points[:, d] for d, key in enumerate(keys)})
    else:
        halotabs = [make(table_of(case))]
    for halotab in halotabs:
        for key, value in options:
            _lib.check(lib.tc_table_set_option(halotab.to_device().handle, key.encode(), value))
    theta = theta_of(case)
    out = {}
    with np.errstate(all='ignore'):
        if case['kind'] == 'interp':
            out['ngal'], out['xi'] = interpolator.predict_batch(theta, x_of(case, points))
        elif case['kind'] == 'latency_chi2':
            out['ngal'], out['chi2'] = halotabs[0].chi2_batch(theta, *likelihood_of(case))
        elif case['separate']:
            ngal, xi = halotabs[0].predict_batch(theta, separate_gal_type=True)
            for key in ngal:
                out['ngal_' + key] = ngal[key]
            for key in xi:
                out['xi_' + key] = xi[key]
        else:
            out['ngal'], out['xi'] = halotabs[0].predict_batch(theta)
    launch = [ctypes.c_int() for _ in range(4)]
    _lib.check(lib.tc_table_last_launch(halotabs[0].to_device().handle,
                                        *[ctypes.byref(v) for v in launch]))
    out = {key: np.ascontiguousarray(value, dtype=np.float64) for key, value in out.items()}
    out['launch'] = np.array([v.value for v in launch[:3]], dtype=np.int64)
    workgroups, waves, slabs = (int(v) for v in out['launch'])
    if latency:
        assert (workgroups, waves, slabs) == ((N_DRAWS + 39) // 40, 8, 0), \
            'not the latency form: %s' % (out['launch'], )
    else:
        # (kernel_args.h: kQuadWavesPerBlock; slabs of partial sums: the contract kernels)
        assert waves == 4 and slabs > 0 and workgroups > 0, \
            'not the three-kernel path: %s' % (out['launch'], )
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
    results = {name: run_case(case) for name, case in cases()}
    target = sys.argv[1] if len(sys.argv) > 1 else FILE
    np.savez_compressed(target, **pack(results))
    again = unpack(np.load(target))
    for name, result in results.items():
        for key, value in result.items():
            assert np.array_equal(again[name][key].view(np.uint64), value.view(np.uint64)), name
    print('%s: %d cases, %d bytes' % (target, len(results), os.path.getsize(target)))
