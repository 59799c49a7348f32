"""Helpers shared by the tests: golden fixtures -> plain table dicts."""

import json
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')

XI_KEYS_AUTO = ['centrals-centrals', 'centrals-satellites',
                'satellites-satellites']
XI_KEYS_CROSS = ['centrals', 'satellites']


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def table_from_golden(data, prefix=''):
    columns = [key[len(prefix) + 3:] for key in data.files
               if key.startswith(prefix + 'gt_')]
    dtype = np.dtype([(c, data[prefix + 'gt_' + c].dtype) for c in columns])
    gal_type = np.zeros(len(data[prefix + 'gt_n_h']), dtype=dtype)
    for c in columns:
        gal_type[c] = data[prefix + 'gt_' + c]
    return {'gal_type': gal_type,
            'tpcf_matrix': data[prefix + 'tpcf_matrix'].astype(np.float64),
            'tpcf_shape': tuple(int(s) for s in data[prefix + 'tpcf_shape']),
            'attrs': json.loads(str(data[prefix + 'attrs']))}


def interpolator_tables_from_golden(data):
    """Tables of the synthetic interpolator fixtures (shared gal_type except
    for n_h, one matrix per table)."""
    base = table_from_golden(data, 'table0_')
    tables = []
    for k in range(len(data['points'])):
        table = dict(base)
        table['gal_type'] = base['gal_type'].copy()
        table['gal_type']['n_h'] = data['n_h'][k]
        table['tpcf_matrix'] = data['tpcf_matrices'][k].astype(np.float64)
        tables.append(table)
    return tables


def xi_keys(table):
    return XI_KEYS_AUTO if table['attrs']['mode'] == 'auto' else XI_KEYS_CROSS


def assert_rel(actual, desired, rtol, what='', floor=1e-14):
    """Elementwise relative agreement, with an absolute floor of ``floor`` x
    the largest |desired| (a few ulp of the scale of the array: elements more
    than ~1e4 below the largest one are sums whose rounding is set by their
    larger neighbours' scale)."""
    actual = np.asarray(actual, dtype=np.float64)
    desired = np.asarray(desired, dtype=np.float64)
    assert actual.shape == desired.shape, (what, actual.shape, desired.shape)
    scale = np.max(np.abs(desired)) if desired.size else 0.0
    np.testing.assert_allclose(actual, desired, rtol=rtol,
                               atol=floor * scale, err_msg=what)


def pair_plan(boxsize, reach_xy, reach_z, n_points, n_bin, n_labels=0):
    """tc_debug_pair_plan (no device needed): what the pair counter plans for a box, the
    reach in the plane and along the line of sight, the larger sample's point count,
    ``n_bin`` bins and ``n_labels`` labels (0: the unlabelled count) -- a dict with ``cells``
    and ``neighbours`` (per axis), ``plan`` = (labels per block of sample 1, of sample 2,
    blocks of sample 1, of sample 2) and ``lds_bytes``."""
    import ctypes
    from tabcorr_amd import _lib
    lib = _lib.load()
    box = np.ascontiguousarray(np.broadcast_to(np.asarray(boxsize, dtype=np.float64), (3, )))
    cells, neighbours = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
    per_block, n_blocks = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)()
    lds = ctypes.c_int64(-1)
    _lib.check(lib.tc_debug_pair_plan(
        box.ctypes.data_as(_lib.c_double_p), float(reach_xy), float(reach_z), int(n_points),
        int(n_bin), int(n_labels), cells, neighbours, per_block, n_blocks, ctypes.byref(lds)))
    return {'cells': tuple(cells), 'neighbours': tuple(neighbours),
            'plan': (per_block[0], per_block[1], n_blocks[0], n_blocks[1]),
            'lds_bytes': lds.value}


def cell_occupancy(pos, boxsize, cells):
    """Points per cell of the pair counter's grid, (nx, ny, nz): a point belongs to cell
    ``min(n - 1, int(x / L n))`` along every axis (hostmath.cpp: sort_into_cells)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    box = np.broadcast_to(np.asarray(boxsize, dtype=np.float64), (3, ))
    cells = np.asarray(cells)
    index = np.minimum(cells - 1, (pos / box * cells).astype(np.int64))
    flat = (index[:, 0] * cells[1] + index[:, 1]) * cells[2] + index[:, 2]
    return np.bincount(flat, minlength=int(np.prod(cells))).reshape(tuple(cells))
