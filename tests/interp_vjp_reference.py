"""Reference for the occupation seam of an interpolator, in NumPy from `vjp_reference.vjp` per
table and `interp_grad_reference.table_weights` for c_t and dc_t/dx_d.  A helper of the
interpolator-seam tests, not a test module.

Tables t on a grid, c_t(x) their tensor-product spline weights; classes v of tables with one halo
table, numbered by first appearance in the list; a draw's occupation is (C, n_bins):

  ngal = sum_t c_t ngal_t, xi = sum_t c_t xi_t
  g_n[v] = sum_{t in v} c_t g_n,t                with g_n,t the table's own VJP
  g_x[d] = sum_t (dc_t/dx_d) (g_ngal ngal_t + sum_r g_r xi_t,r)

Next to every result comes, per element, the absolute scale of the terms that cancel in it:
sum_t |c_t| scale_t for g_n, sum_t |dc_t/dx_d| (|g_ngal| ngal_t + sum_r |g_r xi_t,r|) for g_x, with
|c_t| and |dc_t| the products of the sums of absolute polynomial terms.
"""

import contextlib

import numpy as np

import interp_grad_reference
import vjp_reference
from oracle import tabcorr_oracle as oracle


def classes_of(setup):
    """table_class (K) and class_tables (C) from `oracle.interpolator_setup`, the classes
    renumbered by first appearance in the list."""
    table_class, class_tables, seen = [], [], {}
    for k, label in enumerate(setup['unique_inverse']):
        if int(label) not in seen:
            seen[int(label)] = len(class_tables)
            class_tables.append(k)
        table_class.append(seen[int(label)])
    return np.array(table_class), np.array(class_tables)


@contextlib.contextmanager
def occupations_given(tables, table_class, occupation):
    """While active, `oracle.mean_occupation` of table k returns the row of `occupation` (C,
    n_bins) of its class, whatever the model: `oracle.interpolator_predict` then evaluates the
    interpolator at these occupations."""
    rows = {id(table): occupation[table_class[k]] for k, table in enumerate(tables)}
    original = oracle.mean_occupation
    oracle.mean_occupation = lambda table, model, n_gauss_prim=10: rows[id(table)]
    try:
        yield
    finally:
        oracle.mean_occupation = original


def oracle_predict(tables, setup, table_class, occupation, x, extrapolate=True):
    """(ngal, xi) of `oracle.interpolator_predict` at the per-class occupations."""
    with occupations_given(tables, table_class, np.asarray(occupation, dtype=np.float64)):
        return oracle.interpolator_predict(tables, setup, None, np.asarray(x, dtype=np.float64),
                                           extrapolate=extrapolate)


class Walk:
    """What a batch of calls shares: the dense operands and pair caches of the tables."""

    def __init__(self, tables, setup, points):
        self.tables, self.setup = tables, setup
        self.points = np.asarray(points, dtype=np.float64).reshape(len(tables), -1)
        self.table_class, self.class_tables = classes_of(setup)
        self.ops = [vjp_reference.operands(table) for table in tables]
        self.caches = [{} for _ in tables]

    def per_table(self, occupation, g, g_ngal):
        return [vjp_reference.vjp(table, occupation[self.table_class[k]], g, g_ngal, self.ops[k],
                                  self.caches[k]) for k, table in enumerate(self.tables)]


def _combine(walk, x, results, g, g_abs, g_ngal, scales=None):
    """The interpolated results of one draw from the tables' (ngal, xi, g_n, scale)."""
    c, dc, abs_c, abs_dc = interp_grad_reference.table_weights(walk.setup, walk.points, x)
    ngal_t = np.array([r[0] for r in results])
    xi_t = np.array([np.ravel(r[1]) for r in results])
    scales = results if scales is None else scales
    n_classes = len(walk.class_tables)
    g_n = np.zeros((n_classes, ) + results[0][2].shape)
    scale = np.zeros_like(g_n)
    for k, v in enumerate(walk.table_class):
        g_n[v] += c[k] * results[k][2]
        scale[v] += abs_c[k] * scales[k][3]
    g_x = dc @ (g_ngal * ngal_t + xi_t @ g)
    g_x_scale = abs_dc @ (abs(g_ngal) * np.abs(ngal_t) + np.abs(xi_t) @ g_abs)
    # the values themselves in the oracle's own arithmetic (interpolator_predict: axis by axis
    # over the tables in grid order): sum_t c_t f_t differs from it by the rounding of the
    # power-basis terms that cancel, a few 1e-12 on a 2-D grid
    setup = walk.setup
    shape = [len(xp) for xp in setup['xp']]
    ngal = oracle.spline_interpolate(x, setup['xp'], setup['a'],
                                     ngal_t[setup['order']].reshape(shape), extrapolate=True)
    xi = oracle.spline_interpolate(x, setup['xp'], setup['a'],
                                   xi_t[setup['order']].reshape(shape + [-1]), extrapolate=True)
    return {'ngal': ngal, 'xi': xi, 'g_occupation': g_n, 'g_occupation_scale': scale,
            'g_x': g_x, 'g_x_scale': g_x_scale, 'dngal_dx': dc @ ngal_t,
            'dngal_dx_scale': abs_dc @ np.abs(ngal_t)}


def vjp(walk, occupation, x, g_xi, g_ngal=0.0):
    """One draw: a dict with ngal, xi (flat), g_occupation (C, n_bins), g_x (D), dngal_dx (D) and
    the scales of the last three."""
    g = np.asarray(g_xi, dtype=np.float64).ravel()
    results = walk.per_table(np.asarray(occupation, dtype=np.float64), g, g_ngal)
    return _combine(walk, x, results, g, np.abs(g), g_ngal)


def chi2_grad(walk, occupation, x, data, precision):
    """One draw of the likelihood form: the VJP with g = 2 P_sym (xi - data) of the INTERPOLATED
    xi and g_ngal = 0, with chi2 = e^T P e.  In the scales |g_r| is replaced by 2 sum_s |P_sym,rs|
    (|xi_s| + |data_s|), as `vjp_reference.chi2_grad` does."""
    occupation = np.asarray(occupation, dtype=np.float64)
    data = np.asarray(data, dtype=np.float64).ravel()
    precision = np.asarray(precision, dtype=np.float64)
    p_sym = 0.5 * (precision + precision.T)
    forward = _combine(walk, x, walk.per_table(occupation, np.zeros(len(data)), 0.0),
                       np.zeros(len(data)), np.zeros(len(data)), 0.0)
    e = forward['xi'] - data
    g = 2.0 * p_sym @ e
    g_abs = 2.0 * np.abs(p_sym) @ (np.abs(forward['xi']) + np.abs(data))
    out = _combine(walk, x, walk.per_table(occupation, g, 0.0), g, g_abs, 0.0,
                   walk.per_table(occupation, g_abs, 0.0))
    out['chi2'] = e @ precision @ e
    return out


def batch(function, walk, occupation, x, *per_draw, **shared):
    """`vjp` or `chi2_grad` draw by draw; per_draw arrays (or None) are indexed by the draw."""
    with np.errstate(all='ignore'):
        results = [function(walk, occupation[d], x[d],
                            *[a[d] for a in per_draw if a is not None], **shared)
                   for d in range(len(occupation))]
    return {key: np.array([r[key] for r in results]) for key in results[0]}


def usable(reference):
    return bool(all(np.all(np.isfinite(a)) for a in reference.values()))
