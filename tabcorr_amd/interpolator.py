"""``Interpolator`` with the reference's class surface, on an MI355X.

Mirrors ``tabcorr/interpolator.py`` of johannesulf/TabCorr v1.2.0: a list of
``TabCorr`` instances tabulated on a regular grid of extra parameters (e.g.
``log_eta``, ``alpha_s``, ``alpha_c``) is interpolated with a tensor-product
not-a-knot cubic spline at ``model.param_dict[key]``.

For Zheng07-family models everything runs in one pass on the device: the
occupations once per class of identical halo tables, the spline weight of
every table for every draw, and one contraction that accumulates all tables
(the interpolation is linear in the per-table ``xi``; each table's weight is
divided by that table's total pair weight beforehand because ``xi`` is a
ratio).  ``predict_batch`` exposes the batched form; ``predict`` keeps the
reference's scalar signature.
"""

import ctypes
import threading

import numpy as np

from . import _forward
from . import _grad
from . import _lib
from . import _seam
from .galtable import GalTypeTable
from .models import device_spec
from .tabcorr import (TabCorr, XI_KEYS, NGAL_KEYS, _chi2_operands, _flags,
                      _grad_theta, _unbatch)

OUT_OF_RANGE = ('The x-coordinates are outside of the interpolation ' +
                'range and extrapolation is turned off.')


def _columns(param_dict_table):
    """Column names and values of a parameter table given as an astropy
    Table, a dict of columns or a NumPy structured array."""
    if hasattr(param_dict_table, 'colnames'):
        names = list(param_dict_table.colnames)
        return names, [np.asarray(param_dict_table[n], dtype=np.float64)
                       for n in names]
    if isinstance(param_dict_table, dict):
        names = list(param_dict_table.keys())
        return names, [np.asarray(param_dict_table[n], dtype=np.float64)
                       for n in names]
    array = np.asarray(param_dict_table)
    if array.dtype.names is None:
        raise TypeError('param_dict_table must have named columns.')
    names = list(array.dtype.names)
    return names, [np.asarray(array[n], dtype=np.float64) for n in names]


class _HandleLocks:
    """The lock of an interpolator handle: its own and those of its tables.

    ``tc_interp_*`` calls use the table handles they were created from (the
    quadrature and schedule caches, the fused-likelihood state and the kernel
    timer of the first table, the lanes of every class representative), so a
    call on the interpolator must exclude calls on any of its tables
    (``include/tabcorr_amd.h``).  The table locks are taken in a fixed global
    order, so that two interpolators sharing tables cannot deadlock."""

    def __init__(self, tables):
        unique = {id(t.lock): t.lock for t in tables}
        # (a joint of interpolators takes the two parts of several handles in
        # this order: joint._DeviceJointInterp.ordered_locks)
        self.own = threading.RLock()
        self.of_tables = [unique[k] for k in sorted(unique)]
        self._locks = [self.own] + self.of_tables

    def __enter__(self):
        for lock in self._locks:
            lock.acquire()
        return self

    def __exit__(self, *exc):
        for lock in reversed(self._locks):
            lock.release()
        return False

    def acquire(self, blocking=True):
        taken = []
        for lock in self._locks:
            if not lock.acquire(blocking):
                for held in reversed(taken):
                    held.release()
                return False
            taken.append(lock)
        return True

    def release(self):
        for lock in reversed(self._locks):
            lock.release()


class _DeviceInterpolator(_lib.Handle):
    """Owner of a ``tc_interp`` handle; keeps its tables' handles alive."""

    def __init__(self, interpolator):
        lib = _lib.load()
        devices = [t.to_device() for t in interpolator.tabcorr_list]
        handles = (ctypes.c_void_p * len(devices))(
            *[d.handle for d in devices])
        points = _lib.contiguous(interpolator.points)
        handle = ctypes.c_void_p()
        _lib.check(lib.tc_interp_create(
            ctypes.cast(handles, _lib.c_void_pp), len(devices),
            points.shape[1], _lib.as_double_p(points), ctypes.byref(handle)))
        super().__init__(lib, handle, 'tc_interp_destroy')
        self.tables = devices          # keep the table handles alive
        self.n_r = devices[0].n_r
        # one host thread at a time per handle (see tabcorr._DeviceTable),
        # the handles of the tables included
        self.lock = _HandleLocks(devices)
        # scratch of the un-batched predict(model) path (see
        # tabcorr._DeviceTable.predict_one)
        self._one_theta = np.zeros(16)
        self._one_x = np.zeros(points.shape[1])
        self._one_ngal = np.zeros(1)
        self._one_xi = np.zeros(devices[0].n_r)
        self._one_pointers = tuple(_lib.as_double_p(a) for a in (
            self._one_theta, self._one_x, self._one_ngal, self._one_xi))
        self._one_call = lib.tc_interp_predict_zheng07_batch

    def predict_one(self, theta, x, n_gauss_prim, flags):
        n_theta = len(theta)
        with self.lock:
            self._one_theta[:n_theta] = theta
            self._one_x[:] = x
            p_theta, p_x, p_ngal, p_xi = self._one_pointers
            status = self._one_call(self.handle, p_theta, n_theta, p_x, 1,
                                    n_gauss_prim, flags, p_ngal, p_xi)
            if status:
                _lib.check(status)
            return self._one_ngal[0], self._one_xi.copy()


class Interpolator:
    """Interpolation of multiple `TabCorr` instances."""

    def __init__(self, tabcorr_list, param_dict_table):
        """
        Parameters
        ----------
        tabcorr_list : list of TabCorr
        param_dict_table : table
            Keys and values of the extra parameters of each instance, same
            length and order as ``tabcorr_list``.

        Raises
        ------
        ValueError
            If ``param_dict_table`` does not describe a grid
            (``tabcorr/interpolator.py:32-57``).
        """
        names, columns = _columns(param_dict_table)
        names_columns = [(n, c) for n, c in zip(names, columns)
                         if n != 'tabcorr_index']
        self.keys = [n for n, c in names_columns]
        if len(tabcorr_list) != len(names_columns[0][1]):
            raise ValueError("The number of TabCorr instances does not match" +
                             " the number of entries in 'param_dict_table'.")
        self.tabcorr_list = list(tabcorr_list)
        self.points = np.stack([c for n, c in names_columns], axis=-1)
        self.xp = [np.sort(np.unique(c)) for n, c in names_columns]
        for xp in self.xp:
            if len(xp) < 4:
                raise ValueError('Cannot perform spline interpolation with ' +
                                 'less than 4 values.')
        if (np.prod([len(xp) for xp in self.xp]) != len(self.points) or
                len(np.unique(self.points, axis=0)) != len(self.points)):
            raise ValueError(
                "The 'param_dict_table' does not describe a grid.")
        # Grid order (lexicographic in the keys), as the sorted table with its
        # tabcorr_index column in the reference (interpolator.py:59-61).
        self.order = np.lexsort(self.points.T[::-1])
        columns = {key: self.points[self.order, d]
                   for d, key in enumerate(self.keys)}
        columns['tabcorr_index'] = self.order.copy()
        # (a column table with ``colnames`` / ``[name]`` / ``len`` like the
        # astropy Table of the reference)
        self.param_dict_table = GalTypeTable(columns)
        self._device = None
        self._a = None
        self._checked = None       # signature of the last consistent model

    # -- I/O ------------------------------------------------------------------

    @classmethod
    def read(cls, fname):
        """Read an interpolator written by the reference or by `write`
        (``tabcorr/interpolator.py:72-96``)."""
        from . import io
        return io.read_interpolator(cls, fname)

    def write(self, fname, overwrite=False, max_args_size=1000000,
              matrix_dtype=np.float32):
        """Write in the reference's layout (``tabcorr/interpolator.py:98-122``:
        dataset ``param_dict_table`` plus one group ``tabcorr_{i}`` per
        instance)."""
        from . import io
        io.write_interpolator(self, fname, overwrite=overwrite,
                              max_args_size=max_args_size,
                              matrix_dtype=matrix_dtype)

    # -- device ----------------------------------------------------------------

    def to_device(self):
        if self._device is None:
            self._device = _DeviceInterpolator(self)
        return self._device

    def set_deterministic(self, level=True):
        """``TabCorr.set_deterministic`` for every table of the grid (the
        interpolator's calls read the option of the first one).  ``True``:
        batch-invariant results where a one-launch form serves the grid (mode
        cross with up to 128 rows, e.g. the reference's AbacusSummit
        interpolator); grids in mode auto run three kernels whose sums are cut
        where the batch size puts them -- there the option only refuses the
        measured dispatch.  Returns whether the first table reports a
        batch-invariant form."""
        device = self.to_device()
        invariant = [halotab.set_deterministic(level)
                     for halotab in self.tabcorr_list]
        del device
        return invariant[0]

    def _x_model(self, model):
        x = np.empty(len(self.keys))
        for i, key in enumerate(self.keys):
            try:
                x[i] = model.param_dict[key]
            except KeyError:
                raise ValueError(
                    'The key {} is not present in the parameter '.format(key) +
                    'dictionary of the model.')
        return x

    def _check_range(self, x, extrapolate):
        if extrapolate:
            return
        x = np.atleast_2d(x)
        for d, xp in enumerate(self.xp):
            # (NaN fails the test, as np.digitize puts it past the last node:
            # interpolator.py:318-326)
            if not np.all((x[:, d] >= xp[0]) & (x[:, d] <= xp[-1])):
                raise ValueError(OUT_OF_RANGE)

    # -- predict -------------------------------------------------------------------

    def predict(self, model, separate_gal_type=False, n_gauss_prim=10,
                extrapolate=False, check_consistency=True, **occ_kwargs):
        """Interpolate the predictions of the instances
        (``tabcorr/interpolator.py:124-216``).

        Raises
        ------
        ValueError
            If a key is missing from ``model.param_dict`` or a value lies
            outside the grid and ``extrapolate`` is False.
        """
        x = self._x_model(model)
        if check_consistency:
            # the checks of tabcorr.py:496-535 read a handful of model
            # attributes; they are repeated for every table only when those
            # attributes (or the tables) have changed since the last call
            components = model._input_model_dictionary
            signature = (
                id(self.tabcorr_list[0]), len(self.tabcorr_list),
                tuple(model.gal_types), model.redshift,
                tuple((components[name].prim_haloprop_key,
                       getattr(components[name], 'sec_haloprop_key', None))
                      for name in ('centrals_occupation',
                                   'satellites_occupation')))
            if signature != self._checked:
                for halotab in self.tabcorr_list:
                    halotab._check_consistency(model)
                self._checked = signature
        spec = None if occ_kwargs else device_spec(model)
        if spec is None:
            return self._predict_generic(model, x, separate_gal_type,
                                         n_gauss_prim, extrapolate,
                                         **occ_kwargs)
        if not separate_gal_type:
            self._check_range(x, extrapolate)
            ngal, xi = self.to_device().predict_one(
                spec.theta, x, n_gauss_prim,
                _flags(False, spec.modulate_with_cenocc, spec.assembias,
                       spec.family))
            return ngal, xi.reshape(self.tabcorr_list[0].tpcf_shape)
        return _unbatch(*self.predict_batch(
            spec.theta[np.newaxis], x[np.newaxis],
            separate_gal_type=separate_gal_type, n_gauss_prim=n_gauss_prim,
            extrapolate=extrapolate,
            modulate_with_cenocc=spec.modulate_with_cenocc,
            assembias=spec.assembias, family=spec.family))

    def predict_batch(self, theta, x, separate_gal_type=False,
                      n_gauss_prim=10, extrapolate=False,
                      modulate_with_cenocc=False, assembias=False,
                      family='zheng07', out=None):
        """`predict` for ``(n_draws, 5 | 7)`` Zheng07 parameters ``theta`` and
        ``(n_draws, n_dim)`` values ``x`` of the extra parameters (columns in
        the order of ``self.keys``).  ``out=(ngal, xi)``: page-locked arrays
        that receive the results (see `TabCorr.predict_batch`)."""
        if out is not None:
            return self.predict_batch_async(
                theta, x, separate_gal_type=separate_gal_type,
                n_gauss_prim=n_gauss_prim, extrapolate=extrapolate,
                modulate_with_cenocc=modulate_with_cenocc,
                assembias=assembias, family=family, out=out).wait()
        device, inputs, shapes = self._forward_inputs(
            theta, x, extrapolate, n_gauss_prim,
            _flags(separate_gal_type, modulate_with_cenocc, assembias, family))
        ngal, xi = _forward.call(device, 'interp', 'predict', inputs, shapes)
        return self.tabcorr_list[0]._package(ngal, xi, separate_gal_type)

    def _forward_inputs(self, theta, x, extrapolate, n_gauss_prim, flags,
                        likelihood=False):
        """The device, a forward entry's arguments from the handle to the
        operands, the results' shapes; ``x`` is checked before any device."""
        theta = _lib.contiguous(np.atleast_2d(theta))
        x = _lib.contiguous(np.atleast_2d(x))
        if x.shape != (len(theta), len(self.keys)):
            raise ValueError('x must have shape (n_draws, {}).'.format(
                len(self.keys)))
        self._check_range(x, extrapolate)
        device = self.to_device()
        n_draws = len(theta)
        return (device,
                (theta, theta.shape[1], x, n_draws, n_gauss_prim, flags),
                _forward.shapes(device.tables[0], n_draws, flags, likelihood))

    def predict_batch_async(self, theta, x, separate_gal_type=False,
                            n_gauss_prim=10, extrapolate=False,
                            modulate_with_cenocc=False, assembias=False,
                            family='zheng07', out=None):
        """`predict_batch` without waiting for the device (see
        `TabCorr.predict_batch_async`): returns a
        `tabcorr_amd.pinned.PendingPrediction`."""
        device, inputs, shapes = self._forward_inputs(
            theta, x, extrapolate, n_gauss_prim,
            _flags(separate_gal_type, modulate_with_cenocc, assembias, family))
        first = self.tabcorr_list[0]
        return _forward.call_async(
            device, 'interp', 'predict', inputs, shapes,
            lambda n, v: first._package(n, v, separate_gal_type), out=out)

    def chi2_batch_async(self, theta, x, data, precision, n_gauss_prim=10,
                         extrapolate=False, modulate_with_cenocc=False,
                         assembias=False, family='zheng07', out=None):
        """`chi2_batch` without waiting for the device."""
        device, inputs, shapes = self._forward_inputs(
            theta, x, extrapolate, n_gauss_prim,
            _flags(False, modulate_with_cenocc, assembias, family), True)
        return _forward.call_async(
            device, 'interp', 'chi2', inputs, shapes, lambda n, c: (n, c),
            operands=_chi2_operands(data, precision, device.tables[0].n_r),
            out=out)

    def chi2_batch(self, theta, x, data, precision, n_gauss_prim=10,
                   extrapolate=False, modulate_with_cenocc=False,
                   assembias=False, family='zheng07'):
        """Gaussian ``chi^2 = (xi - data)^T precision (xi - data)`` of every
        draw of `predict_batch`, evaluated on the device right behind the
        interpolated prediction (extension, as `TabCorr.chi2_batch`: the
        reference leaves the likelihood to the user, ``README.md:7``).

        Returns
        -------
        ngal, chi2 : numpy.ndarray ``(n_draws, )``
        """
        device, inputs, shapes = self._forward_inputs(
            theta, x, extrapolate, n_gauss_prim,
            _flags(False, modulate_with_cenocc, assembias, family), True)
        return _forward.call(
            device, 'interp', 'chi2', inputs, shapes,
            _chi2_operands(data, precision, device.tables[0].n_r))

    # -- analytic gradients ----------------------------------------------------------

    def _grad_inputs(self, theta, x, extrapolate, assembias=False,
                     family='zheng07'):
        """``theta (n, 5)`` -- ``(n, 7)`` for the model decorated with
        assembly bias, ``(n, 14)`` for the Leauthaud11 family -- and
        ``x (n, D)`` of the gradient calls, checked before any device is
        touched."""
        theta = _grad_theta(theta, assembias, family)
        x = _lib.contiguous(np.atleast_2d(x))
        if x.shape != (len(theta), len(self.keys)):
            raise ValueError('x must have shape (n_draws, {}).'.format(
                len(self.keys)))
        self._check_range(x, extrapolate)
        return theta, x

    def predict_batch_grad(self, theta, x, n_gauss_prim=10, extrapolate=False,
                           modulate_with_cenocc=False, assembias=False,
                           family='zheng07'):
        """`predict_batch` together with the exact derivatives of its results
        with respect to the five Zheng07 parameters and the ``D`` extra
        parameters (columns: `ZHENG07_KEYS`, then ``self.keys``), in one
        kernel launch: what a best-fit search, a Fisher forecast or an HMC
        sampler over ``(theta, x)`` would otherwise difference `predict_batch`
        ``2 (5 + D)`` times for.

        The interpolated result is linear in the tables' results, so the
        derivative with respect to ``theta`` is the interpolated table
        gradient (`TabCorr.predict_batch_grad`, with its kinks in ``logM0``)
        and the one with respect to ``x`` the derivative of the spline
        weights.  The not-a-knot spline is C2: there is no kink in ``x``; an
        ``x`` outside the grid (``extrapolate=True``) gets the derivative of
        the outermost polynomial.

        ``assembias=True``: the model decorated with assembly bias, as
        `TabCorr.predict_batch_grad` has it: ``theta`` and the derivatives
        carry the 7 columns of `ZHENG07_ASSEMBIAS_KEYS` (7 wherever 5 stands
        below), then ``self.keys``.

        ``family='leauthaud11'``: ``theta`` has the 14 columns
        ``predict_batch(..., family='leauthaud11')`` takes, and the
        derivatives carry the eleven columns of
        `tabcorr_amd.models.LEAUTHAUD11_GRAD_KEYS` (threshold, h and h_s are
        inputs), then ``self.keys``: 11 wherever 5 stands below.  Not
        together with ``assembias``.

        Returns
        -------
        ngal : ``(n_draws, )``
        xi : ``(n_draws, ) + tpcf_shape``
        dngal : ``(n_draws, 5 + D)``
        dxi : ``(n_draws, 5 + D) + tpcf_shape``

        Raises ``NotImplementedError`` for what the kernel does not serve
        (float32 tables, grids whose rows do not fit the LDS of a workgroup).
        """
        theta, x = self._grad_inputs(theta, x, extrapolate, assembias, family)
        return self._grad_call(theta, x, n_gauss_prim, modulate_with_cenocc,
                               assembias, family)

    def _grad_call(self, theta, x, n_gauss_prim, modulate_with_cenocc,
                   assembias, family, operands=None, want_fisher=False):
        """The derivative entry for checked ``(theta, x)``: the family's
        columns, then ``self.keys``."""
        return _grad.call(
            self.to_device(), 'interp', _grad.family_of(assembias, family),
            [theta, theta.shape[1], x, len(theta), n_gauss_prim,
             _flags(False, modulate_with_cenocc)],
            len(_grad.keys_of(assembias, family)) + len(self.keys),
            self.tabcorr_list[0].tpcf_shape, operands, want_fisher)

    def chi2_grad_batch(self, theta, x, data, precision, n_gauss_prim=10,
                        extrapolate=False, modulate_with_cenocc=False,
                        assembias=False, family='zheng07'):
        """`chi2_batch` with its gradient with respect to ``(theta, x)``:
        ``dchi2[:, k] = 2 (xi - data)^T P_sym dxi_k`` with ``P_sym =
        (precision + precision^T) / 2``, finished on the device in the launch
        that computes ``xi``.  ``assembias=True``: ``7 + D`` columns,
        ``family='leauthaud11'``: ``11 + D`` (of 14 theta columns), as in
        `predict_batch_grad`.

        Returns
        -------
        ngal, chi2 : ``(n_draws, )``
        dngal, dchi2 : ``(n_draws, 5 + D)``
        """
        theta, x = self._grad_inputs(theta, x, extrapolate, assembias, family)
        operands = _chi2_operands(
            data, precision, len(self.tabcorr_list[0].tpcf_matrix))
        return self._grad_call(theta, x, n_gauss_prim, modulate_with_cenocc,
                               assembias, family, operands)

    def predict_grad(self, model, n_gauss_prim=10, extrapolate=False,
                     check_consistency=True, assembias=False):
        """Un-batched `predict_batch_grad` for a model object: a plain
        `tabcorr_amd.Zheng07Model` (or the halotools zheng07 composite model)
        whose ``param_dict`` holds the extra parameters; with
        ``assembias=True`` a decorated one, the dicts then keyed by
        ``ZHENG07_ASSEMBIAS_KEYS + tuple(self.keys)``.  A
        `tabcorr_amd.Leauthaud11Model` is served too: the dicts are then keyed
        by the sixteen `LEAUTHAUD11_KEYS` of its ``param_dict``, then
        ``self.keys``, the eleven device columns carried to the sixteen by
        `Leauthaud11Model.device_jacobian` as in `TabCorr.predict_grad`.

        Returns
        -------
        ngal : float
        xi : numpy.ndarray of shape ``tpcf_shape``
        dngal : dict, ``ZHENG07_KEYS + tuple(self.keys)`` -> float
        dxi : dict, the same keys -> numpy.ndarray of shape ``tpcf_shape``
        """
        x = self._x_model(model)
        if check_consistency:
            for halotab in self.tabcorr_list:
                halotab._check_consistency_cached(model)
        theta, options, columns, _ = _grad.model_columns(
            model, assembias, 'predict_grad', self.keys, leauthaud11=True)
        ngal, xi, dngal, dxi = self.predict_batch_grad(
            theta, x[np.newaxis], n_gauss_prim=n_gauss_prim,
            extrapolate=extrapolate, **options)
        return (float(ngal[0]), xi[0], _grad.keyed(dngal[0], columns=columns),
                _grad.keyed(dxi[0], columns=columns))

    # -- Fisher matrix of the likelihood ------------------------------------------------

    def chi2_fisher_batch(self, theta, x, data, precision, n_gauss_prim=10,
                          extrapolate=False, modulate_with_cenocc=False,
                          assembias=False, family='zheng07'):
        """`chi2_grad_batch` with the Fisher matrix of the likelihood over
        ``(theta, x)``, from the same launch: with ``dxi_k`` the Jacobian
        column of quantity ``k`` (`ZHENG07_KEYS`, then ``self.keys``),

            ``fisher[:, k, l] = 1/2 sum_r dxi_k[r] (sum_s (P[r, s] + P[s, r])
            dxi_l[s]) = dxi_k^T P_sym dxi_l``

        with ``P_sym = (precision + precision^T) / 2`` (see
        `TabCorr.chi2_fisher_batch`).  The Gauss-Newton Hessian of chi2 is
        ``2 fisher``.  The ``ngal`` part of a likelihood stays the caller's:
        ``dngal`` is returned next to ``fisher``, and an outer product
        completes it.  The matrix is symmetric to the bit; a draw's matrix
        does not depend on its batch, and not on ``data``.
        ``assembias=True``: ``7 + D`` columns, ``family='leauthaud11'``:
        ``11 + D`` columns and an ``(11 + D, 11 + D)`` matrix, as in
        `predict_batch_grad`.

        Returns
        -------
        ngal, chi2 : ``(n_draws, )``
        dngal, dchi2 : ``(n_draws, 5 + D)`` -- those of `chi2_grad_batch`, bit
            for bit
        fisher : ``(n_draws, 5 + D, 5 + D)``
        """
        theta, x = self._grad_inputs(theta, x, extrapolate, assembias, family)
        operands = _chi2_operands(
            data, precision, len(self.tabcorr_list[0].tpcf_matrix))
        return self._grad_call(theta, x, n_gauss_prim, modulate_with_cenocc,
                               assembias, family, operands, True)

    def fisher_batch(self, theta, x, precision, n_gauss_prim=10,
                     extrapolate=False, modulate_with_cenocc=False,
                     assembias=False, family='zheng07'):
        """The forecast form of `chi2_fisher_batch`, which needs no data: the
        same launch with a zero data vector, without ``chi2`` and ``dchi2``.
        The Gauss-Newton Hessian of chi2 is ``2 fisher``; the ``ngal`` part of
        a likelihood is the caller's, from ``dngal`` by an outer product.

        Returns
        -------
        ngal : ``(n_draws, )``
        dngal : ``(n_draws, 5 + D)``
        fisher : ``(n_draws, 5 + D, 5 + D)``
        """
        ngal, _, dngal, _, fisher = self.chi2_fisher_batch(
            theta, x, np.zeros(len(self.tabcorr_list[0].tpcf_matrix)),
            precision, n_gauss_prim=n_gauss_prim, extrapolate=extrapolate,
            modulate_with_cenocc=modulate_with_cenocc, assembias=assembias,
            family=family)
        return ngal, dngal, fisher

    def fisher(self, model, precision, n_gauss_prim=10, extrapolate=False,
               check_consistency=True, assembias=False):
        """Un-batched `fisher_batch` for a model object: a plain
        `tabcorr_amd.Zheng07Model` (or the halotools zheng07 composite model)
        whose ``param_dict`` holds the extra parameters, as `predict_grad`
        takes.  The Gauss-Newton Hessian of chi2 is ``2 fisher``; the ``ngal``
        part of a likelihood is the caller's, from ``dngal`` by an outer
        product.  ``assembias=True``: a decorated model and
        ``ZHENG07_ASSEMBIAS_KEYS + tuple(self.keys)``.  A
        `tabcorr_amd.Leauthaud11Model`: `LEAUTHAUD11_KEYS`, then
        ``self.keys``, and the ``(16 + D, 16 + D)`` matrix ``J^T F J`` with
        ``F`` the ``(11 + D, 11 + D)`` matrix of the device columns and ``J``
        the block-diagonal matrix of `Leauthaud11Model.device_jacobian` and
        the identity of the extra parameters.

        Returns
        -------
        ngal : float
        dngal : dict, ``ZHENG07_KEYS + tuple(self.keys)`` -> float
        fisher : numpy.ndarray of shape ``(5 + D, 5 + D)`` in that key order
        """
        x = self._x_model(model)
        if check_consistency:
            for halotab in self.tabcorr_list:
                halotab._check_consistency_cached(model)
        theta, options, columns, jacobian = _grad.model_columns(
            model, assembias, 'fisher', self.keys, leauthaud11=True)
        ngal, dngal, fisher = self.fisher_batch(
            theta, x[np.newaxis], precision, n_gauss_prim=n_gauss_prim,
            extrapolate=extrapolate, **options)
        return (float(ngal[0]), _grad.keyed(dngal[0], columns=columns),
                _grad.carried(fisher[0], jacobian))

    # -- the occupation seam: any occupation model, one launch ---------------------------

    def _classes(self):
        """``table_class`` and ``class_tables``: the classes of identical
        halo tables (``tabcorr/interpolator.py:63-70``), numbered by first
        appearance in ``tabcorr_list``."""
        if getattr(self, '_class_cache', None) is None:
            raws, table_class, class_tables = [], [], []
            for k, halotab in enumerate(self.tabcorr_list):
                raw = halotab.gal_type.as_array()
                for v, other in enumerate(raws):
                    if other.dtype == raw.dtype and np.array_equal(other, raw):
                        table_class.append(v)
                        break
                else:
                    table_class.append(len(raws))
                    class_tables.append(k)
                    raws.append(raw)
            self._class_cache = (np.array(table_class, dtype=np.int64),
                                 np.array(class_tables, dtype=np.int64))
        return self._class_cache

    @property
    def table_class(self):
        """``(K, )``: the class of every table of ``tabcorr_list`` -- tables
        with identical halo tables share their occupations."""
        return self._classes()[0]

    @property
    def class_tables(self):
        """``(C, )``: the first table of every class, in class order (first
        appearance in ``tabcorr_list``)."""
        return self._classes()[1]

    def mean_occupation(self, model, n_gauss_prim=10, check_consistency=True,
                        **occ_kwargs):
        """The mean occupations of ``model`` for the occupation seam:
        ``(C, n_bins)``, the Gauss-Legendre average of the model's callbacks
        (``tabcorr/tabcorr.py:537-578``) for the first table of every class,
        on the host (row ``v`` in the ``gal_type`` row order of that class's
        tables).  ANY occupation model, with or without ``**occ_kwargs``."""
        if check_consistency:
            for halotab in self.tabcorr_list:
                halotab._check_consistency_cached(model)
        return np.stack([
            self.tabcorr_list[k]._host_mean_occupation(
                model, n_gauss_prim, **occ_kwargs)
            for k in self.class_tables])

    def class_weights(self, x):
        """``(n_draws, C)``: the sum of the tables' spline weights ``c_t(x)``
        over every class, on the host (``tc_spline_weights``: the text the
        kernels run; an ``x`` outside the grid takes the outermost
        polynomial).  It is the factor that the seam's calls leave to a
        likelihood with an ``ngal`` term: ``dngal/docc[:, v] =
        class_weights[:, v, None] * n_h_v`` with ``n_h_v`` the
        ``gal_type['n_h']`` of class ``v``."""
        x = _lib.contiguous(np.atleast_2d(x))
        if x.ndim != 2 or x.shape[1] != len(self.keys):
            raise ValueError('x must have shape (n_draws, {}).'.format(
                len(self.keys)))
        lib = _lib.load()
        a = self._spline_matrices()
        coef = np.ones((len(x), len(self.tabcorr_list)))
        for d, xp in enumerate(self.xp):
            xp = _lib.contiguous(xp)
            node = np.searchsorted(xp, self.points[:, d])
            weight, dweight = np.empty(len(xp)), np.empty(len(xp))
            for i in range(len(x)):
                _lib.check(lib.tc_spline_weights(
                    len(xp), _lib.as_double_p(xp), _lib.as_double_p(a[d]),
                    float(x[i, d]), _lib.as_double_p(weight),
                    _lib.as_double_p(dweight), None))
                coef[i] *= weight[node]
        out = np.zeros((len(x), len(self.class_tables)))
        for k, v in enumerate(self.table_class):
            out[:, v] += coef[:, k]
        return out

    def _seam_inputs(self, occupation, x, extrapolate):
        """The contiguous ``(n, C, n_bins)`` occupations and ``(n, D)`` grid
        parameters of the seam's calls; wrong shapes and an ``x`` outside the
        grid are refused before any device is touched."""
        n_classes = len(self.class_tables)
        n_bins = len(self.tabcorr_list[0].gal_type)
        occupation = np.asarray(occupation, dtype=np.float64)
        if occupation.ndim == 2 and n_classes == 1:
            occupation = occupation[:, np.newaxis, :]
        if occupation.ndim != 3 or occupation.shape[1:] != (n_classes, n_bins):
            raise ValueError(
                'The mean occupation array must have shape (n_draws, {}, {})'
                ', got {}.'.format(n_classes, n_bins, occupation.shape))
        x = _lib.contiguous(np.atleast_2d(x))
        if x.shape != (len(occupation), len(self.keys)):
            raise ValueError('x must have shape (n_draws, {}).'.format(
                len(self.keys)))
        self._check_range(x, extrapolate)
        return _lib.contiguous(occupation), x

    def _seam_device(self):
        device = self.to_device()
        if not getattr(self, '_classes_checked', False):
            n_tables, n_classes = ctypes.c_int(0), ctypes.c_int(0)
            table_class = np.zeros(len(self.tabcorr_list), dtype=np.int32)
            with device.lock:
                _lib.check(device.lib.tc_interp_info(
                    device.handle, ctypes.byref(n_tables),
                    ctypes.byref(n_classes),
                    table_class.ctypes.data_as(_lib.c_int_p), None))
            if not np.array_equal(table_class, self.table_class):
                raise RuntimeError(
                    'the library groups the tables into other classes ({}) '
                    'than the host ({})'.format(table_class, self.table_class))
            self._classes_checked = True
        return device

    def _predict_occupation(self, occupation, x, g_xi, g_ngal, extrapolate):
        occupation, x = self._seam_inputs(occupation, x, extrapolate)
        shape = tuple(self.tabcorr_list[0].tpcf_shape)
        cotangents = None if g_xi is None else _seam.cotangents(
            g_xi, g_ngal, len(occupation), True, shape)
        ngal, xi, g_occupation, g_x = _seam.call(
            self._seam_device(), 'interp', 'predict', occupation, x,
            cotangents=cotangents)
        return ngal, xi.reshape((len(ngal), ) + shape), g_occupation, g_x

    def predict_occupation(self, occupation, x, extrapolate=False):
        """The interpolated ``predict(occupation)`` for ANY occupation model,
        in one launch: ``occupation`` ``(n_draws, C, n_bins)`` as
        `mean_occupation` returns it per draw (``(n_draws, n_bins)`` where
        ``C = 1``), ``x`` ``(n_draws, D)`` in the order of ``self.keys``.

        Returns ``ngal (n_draws, )`` and ``xi (n_draws, ) + tpcf_shape``.
        Raises ``NotImplementedError`` for what the kernel does not serve
        (float32 tables, grids whose rows do not fit the LDS of a workgroup).
        """
        return self._predict_occupation(occupation, x, None, None,
                                        extrapolate)[:2]

    def predict_vjp(self, occupation, x, g_xi, g_ngal=None,
                    extrapolate=False):
        """`predict_occupation` with its vector-Jacobian product with respect
        to the occupation array AND the grid parameters, in the same launch:
        for cotangents ``g_ngal (n_draws, )`` (None = 0) and ``g_xi
        (n_draws, ) + tpcf_shape``, ``g_occupation[d, v, i] = g_ngal[d]
        dngal[d] / dn[d, v, i] + sum_r g_xi[d, r] dxi[d, r] / dn[d, v, i]`` and
        ``g_x[d, e]`` likewise with respect to ``x[d, e]``.  Contracted with
        the caller's own ``d<N>/dtheta`` it is the gradient of any scalar of
        ``(ngal, xi)`` for EVERY occupation model.

        Returns ``ngal, xi, g_occupation (n_draws, C, n_bins), g_x
        (n_draws, D)``.
        """
        if g_xi is None:
            raise ValueError('g_xi is None: predict_occupation is the '
                             'forward-only call.')
        return self._predict_occupation(occupation, x, g_xi, g_ngal,
                                        extrapolate)

    def _chi2_occupation(self, occupation, x, data, precision, extrapolate,
                         gradient):
        occupation, x = self._seam_inputs(occupation, x, extrapolate)
        operands = _chi2_operands(
            data, precision, len(self.tabcorr_list[0].tpcf_matrix))
        return _seam.call(self._seam_device(), 'interp', 'chi2', occupation,
                          x, operands=operands, gradient=gradient)

    def chi2_occupation(self, occupation, x, data, precision,
                        extrapolate=False):
        """``chi2 = (xi - data)^T precision (xi - data)`` of
        `predict_occupation`, finished in the launch: ``ngal, chi2``
        ``(n_draws, )``."""
        return self._chi2_occupation(occupation, x, data, precision,
                                     extrapolate, False)[:2]

    def chi2_grad_occupation(self, occupation, x, data, precision,
                             extrapolate=False):
        """`chi2_occupation` with its gradient with respect to the occupation
        array and the grid parameters -- `predict_vjp` with ``g_xi = 2 P_sym
        (xi - data)``, ``P_sym = (precision + precision^T) / 2``, and
        ``g_ngal = 0``, formed on the device from the interpolated ``xi`` in
        the same launch.  For a likelihood with an ``ngal`` term ``dngal_dx``
        comes with it, and ``dngal/docc`` needs no launch (`class_weights`).
        Contracted with the caller's own ``d<N>/dtheta`` the results are the
        gradient over ``(theta, x)`` for EVERY occupation model
        (``examples/example_interp_custom_model_grad.py``: Leauthaud11).

        Returns ``ngal, chi2 (n_draws, )``, ``dchi2_docc (n_draws, C,
        n_bins)``, ``dchi2_dx`` and ``dngal_dx (n_draws, D)``.
        """
        return self._chi2_occupation(occupation, x, data, precision,
                                     extrapolate, True)

    # -- generic models: host callbacks + device contraction per table -----------------

    def _spline_matrices(self):
        if self._a is None:
            lib = _lib.load()
            self._a = []
            for xp in self.xp:
                xp = _lib.contiguous(xp)
                a = np.zeros((len(xp) - 1, 4, len(xp)))
                _lib.check(lib.tc_spline_interpolation_matrix(
                    len(xp), _lib.as_double_p(xp), _lib.as_double_p(a)))
                self._a.append(a)
        return self._a

    def _predict_generic(self, model, x, separate_gal_type, n_gauss_prim,
                         extrapolate, **occ_kwargs):
        self._check_range(x, extrapolate)
        # occupations once per distinct halo table (interpolator.py:63-70,
        # 181-184)
        cache = []
        results = []
        for k in self.order:
            halotab = self.tabcorr_list[k]
            raw = halotab.gal_type.as_array()
            occupation = None
            for other, value in cache:
                if other.dtype == raw.dtype and np.array_equal(other, raw):
                    occupation = value
                    break
            if occupation is None:
                occupation = halotab._host_mean_occupation(
                    model, n_gauss_prim, **occ_kwargs)
                cache.append((raw, occupation))
            results.append(halotab.predict(
                occupation, separate_gal_type=separate_gal_type))
        shape = [len(xp) for xp in self.xp]
        a = self._spline_matrices()
        output = []
        for i in range(2):
            if separate_gal_type:
                output.append({})
                for key in results[0][i]:
                    data = np.array([r[i][key] for r in results])
                    data = data.reshape(shape + list(data.shape[1:]))
                    output[-1][key] = spline_interpolate(
                        x, self.xp, a, data, extrapolate=extrapolate)
            else:
                data = np.array([r[i] for r in results])
                data = data.reshape(shape + list(data.shape[1:]))
                output.append(spline_interpolate(
                    x, self.xp, a, data, extrapolate=extrapolate))
        return tuple(output)


def spline_interpolation_matrix(xp):
    """Matrix ``a`` of shape ``(n - 1, 4, n)`` such that
    ``np.einsum('ij,j,i', a[i], y, x0**np.arange(4))`` is the ``i``-th segment
    of the not-a-knot cubic spline through ``(xp, y)`` at ``x0``
    (``tabcorr/interpolator.py:219-272``; computed by the C library).

    Raises
    ------
    ValueError
        If ``xp`` has fewer than 4 entries.
    """
    xp = _lib.contiguous(xp)
    a = np.zeros((max(len(xp) - 1, 0), 4, len(xp)))
    _lib.check(_lib.load().tc_spline_interpolation_matrix(
        len(xp), _lib.as_double_p(xp), _lib.as_double_p(a)))
    return a


def spline_interpolate(x, xp, a, yp, extrapolate=False):
    """Evaluate the tensor-product spline along the first ``len(x)`` axes of
    ``yp`` (``tabcorr/interpolator.py:275-331``): segment search with
    ``np.digitize`` (right edge included), ``ValueError`` or clamping outside
    the grid, cubic polynomial per axis."""
    xp = xp if isinstance(xp, list) else [xp]
    a = a if isinstance(a, list) else [a]
    for value, matrix, nodes in zip(np.atleast_1d(x), a, xp):
        segment = int(np.searchsorted(nodes, value, side='right')) - 1
        if value == nodes[-1]:
            segment = len(nodes) - 2
        if not 0 <= segment <= len(nodes) - 2:
            if not extrapolate:
                raise ValueError(OUT_OF_RANGE)
            segment = min(max(segment, 0), len(nodes) - 2)
        weights = matrix[segment].T @ value**np.arange(4)
        yp = np.tensordot(weights, yp, axes=(0, 0))
    return yp
