"""Records what the one-launch kernel's 64-draw and 32-draw forms return, on an MI355X, into
fused_walk_parent.npz:  python tests/golden/make_fused_walk_parent.py

Run it with the library of the commit whose bits are the reference (the parent of the change to
the walk of the matrix units); tests/test_gpu_fused_walk.py then asks every later library for
the same bits.  `cases()` and `run_case()` are what that test evaluates too.

The file holds, per case, the (workgroups, waves) of the launch and the results as float64.  The
results of the forms 32 x 8 and 64 x 16 differ from those of 64 x 8 in their last bits only, so
they are kept as the exclusive-or with the 64 x 8 words (zeros but for a byte or two per value:
the compressed file stays a third of the plain arrays' size).
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
FILE = os.path.join(HERE, 'fused_walk_parent.npz')

N_DRAWS = 81            # one full and one partial 64-draw workgroup, two and a bit of 32
# (n_prim, n_r): 8 ... 36 bins = 2 ... 9 block rows with the most r sub-tiles (U = 5), and the
# benchmark's 100 bins = 25 block rows with U = 1, 2, 3, 5
SHAPES = [(4, 19), (5, 19), (10, 19), (18, 19), (50, 3), (50, 8), (50, 12), (50, 19)]
FORMS = {'64x8': (64, 8), '32x8': (32, 8), '64x16': (64, 16)}       # draws x waves
BASE_FORM = '64x8'
# (the draws theta_of replaces by NaN / infinite / tied parameters in a degenerate case)
DEGENERATE_ROWS = (3, 10, 11, 20, 30, 40, 50, 60, 66, 70, 72, 75, 78, 80)


def cases():
    """(name, dict) of every recorded case, the 64 x 8 form of a shape first."""
    out = []
    for n_prim, n_r in SHAPES:
        for form in FORMS:
            for separate in (False, True):
                name = 'p%d_r%d_%s_%s' % (n_prim, n_r, form, 'sep' if separate else 'tot')
                out.append((name, dict(kind='predict', n_prim=n_prim, n_r=n_r, form=form,
                                       separate=separate, degenerate=False)))
    for form in FORMS:
        out.append(('chi2_p50_r19_' + form, dict(kind='chi2', n_prim=50, n_r=19, form=form,
                                                 separate=False, degenerate=False)))
        for separate in (False, True):
            name = 'degenerate_p10_r19_%s_%s' % (form, 'sep' if separate else 'tot')
            out.append((name, dict(kind='predict', n_prim=10, n_r=19, form=form,
                                   separate=separate, degenerate=True)))
    return out


def base_name(name):
    for form in FORMS:
        name = name.replace('_' + form, '_' + BASE_FORM)
    return name


def table_of(case):
    from tabcorr_amd import synthetic
    return synthetic.synthetic_table(case['n_prim'], 1, (case['n_r'], ), 'auto',
                                     seed=case['n_prim'] + case['n_r'])


def theta_of(case):
    from tabcorr_amd import synthetic
    theta = synthetic.zheng07_draws(N_DRAWS, seed=N_DRAWS + case['n_prim'])
    if case['degenerate']:
        # the draws of test_gpu_fused.py::test_fused_degenerate_parameters, in both workgroups
        theta[3, 0] = np.nan
        theta[10, 1] = 0.0
        theta[11, 1] = np.inf
        theta[20, 2] = np.nan
        theta[30, 3] = np.nan
        theta[40, 4] = np.nan
        theta[50, 3] = -np.inf
        theta[60, 2] = np.inf
        theta[66, 0] = np.inf
        theta[70, 0] = -np.inf
        theta[72, 4] = 0.0
        theta[75, 4] = -1.0
        theta[78, 3] = -400.0
        theta[80] = [11.0, 0.0, 11.0, 13.0, 1.0]
    return theta


def likelihood_of(case):
    """Data vector and weight matrix of the likelihood case (fixed numbers, no device)."""
    rng = np.random.default_rng(case['n_r'])
    vector = np.geomspace(30.0, 0.05, case['n_r'])
    a = rng.normal(size=(case['n_r'], case['n_r']))
    return vector, a @ a.T / np.mean(vector)**2


def run_case(case):
    """The case on the device: {'launch': (workgroups, waves, slabs), name: float64 array}."""
    import ctypes
    from tabcorr_amd import TabCorr, _lib
    lib = _lib.load()
    table = table_of(case)
    halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                  table['attrs'])
    handle = halotab.to_device().handle
    draws, waves = FORMS[case['form']]
    for key, value in (('fused', 2), ('fused_min_draws', 1), ('single_draw', 0),
                       ('fused_draws', draws), ('fused_waves', waves)):
        _lib.check(lib.tc_table_set_option(handle, key.encode(), value))
    theta = theta_of(case)
    out = {}
    with np.errstate(all='ignore'):
        if case['kind'] == 'chi2':
            vector, precision = likelihood_of(case)
            ngal, chi2 = halotab.chi2_batch(theta, vector, precision)
            out['ngal'], out['chi2'] = ngal, chi2
        elif case['separate']:
            ngal, xi = halotab.predict_batch(theta, separate_gal_type=True)
            for key in ngal:
                out['ngal_' + key] = ngal[key]
            for key in xi:
                out['xi_' + key] = xi[key]
        else:
            out['ngal'], out['xi'] = halotab.predict_batch(theta)
    launch = [ctypes.c_int() for _ in range(4)]
    _lib.check(lib.tc_table_last_launch(handle, *[ctypes.byref(v) for v in launch]))
    out = {key: np.ascontiguousarray(value, dtype=np.float64) for key, value in out.items()}
    out['launch'] = np.array([v.value for v in launch[:3]], dtype=np.int64)
    assert tuple(out['launch']) == ((N_DRAWS + draws - 1) // draws, waves, 0), \
        'not the form asked for: %s' % (out['launch'], )
    return out


def pack(results):
    """{case: {key: array}} -> the arrays of the file."""
    arrays = {}
    for name, result in results.items():
        base = results[base_name(name)]
        for key, value in result.items():
            if key == 'launch' or base is result:
                arrays[name + '/' + key] = value
            else:
                arrays[name + '/' + key + '^'] = value.view(np.uint64) ^ base[key].view(np.uint64)
    return arrays


def unpack(data):
    """The arrays of the file -> {case: {key: array}}."""
    results = {}
    for name, _ in cases():
        result = {}
        for full in data.files:
            if not full.startswith(name + '/'):
                continue
            key = full[len(name) + 1:]
            if key.endswith('^'):
                key = key[:-1]
                result[key] = (data[full] ^ results[base_name(name)][key].view(np.uint64)
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
