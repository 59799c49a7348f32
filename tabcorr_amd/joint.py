"""``JointLikelihood``: tables that share one halo table, fitted together.

The reference's documented likelihood step evaluates two tables per model
(``docs/guides/overview.rst:86-92``: ``halotab_wp.predict(model)``, then
``halotab_ds.predict(model)``); the data vector of such an analysis is the
concatenation (w_p, DeltaSigma), and its covariance couples the probes.  A
`JointLikelihood` evaluates a batch of draws against all of its tables in ONE
kernel launch (``tc_joint_*``, ``include/tabcorr_amd.h``): the occupations and
their derivatives once per draw, every table's contraction, and chi2, its
gradient and the Fisher matrix against the full ``(N, N)`` precision matrix,
``N`` the sum of the tables' correlation function bins.  The forward calls
`predict_batch` and `chi2_batch` -- what an ensemble sampler asks per step --
take a launch of their own kind, without any derivative.  For every other
occupation model there is the occupation seam: `predict_occupation`,
`predict_vjp`, `chi2_occupation` and `chi2_grad_occupation` take the occupation
array itself, again one launch for all tables.
"""

import ctypes

import numpy as np

from . import _forward
from . import _grad
from . import _lib
from . import _seam
from .tabcorr import _flags, _grad_theta

MAX_TABLES = 16
# the gal_type columns the device reads (tabcorr.py: _DeviceTable)
BIN_COLUMNS = ('n_h', 'log_prim_haloprop_min', 'log_prim_haloprop_max',
               'sec_haloprop_percentile', 'prim_haloprop_dist_index')


def _same_bins(a, b):
    """Whether two gal_type tables describe the same bins."""
    if len(a) != len(b) or not np.array_equal(a.is_centrals(),
                                              b.is_centrals()):
        return False
    for name in BIN_COLUMNS:
        if (name in a.colnames) != (name in b.colnames):
            return False
        if name in a.colnames and not np.array_equal(a[name], b[name]):
            return False
    return True


def _zheng07_only(family):
    if family not in ('zheng07', 'leauthaud11'):
        raise ValueError("family must be 'zheng07' or 'leauthaud11'.")
    if family != 'zheng07':
        raise NotImplementedError(
            'A joint serves the Zheng07 family only (plain or decorated with '
            'assembly bias).')


class _Locks:
    """The locks of everything a joint works through, taken together in the
    order of the list: one fixed order whatever the order of the members in
    the joint (`TabCorr.predict_joint` takes its tables' the same way)."""

    def __init__(self, locks):
        self.locks = locks

    def __enter__(self):
        for lock in self.locks:
            lock.acquire()

    def __exit__(self, *exc):
        for lock in reversed(self.locks):
            lock.release()


class _DeviceJoint(_lib.Handle):
    """Owner of a ``tc_joint`` handle; keeps its tables' handles alive.  A
    joint works through its tables (``include/tabcorr_amd.h``): every call
    sits behind `lock`, all of their locks.  `n_r`: the joint axis."""

    kind = 'joint'

    def __init__(self, devices):
        lib = devices[0].lib
        handles = (ctypes.c_void_p * len(devices))(
            *[d.handle.value for d in devices])
        handle = ctypes.c_void_p()
        _lib.check(getattr(lib, 'tc_%s_create' % self.kind)(
            handles, len(devices), ctypes.byref(handle)))
        super().__init__(lib, handle, 'tc_%s_destroy' % self.kind)
        self.devices = devices
        self.n_r = sum(d.n_r for d in devices)
        self.lock = _Locks(self.ordered_locks(devices))

    @staticmethod
    def ordered_locks(devices):
        return [d.lock for d in sorted(devices, key=id)]


class _DeviceJointInterp(_DeviceJoint):
    """Owner of a ``tc_joint_interp`` handle; keeps its members' handles
    alive.  The joint works through its members and their tables: every call
    sits behind `lock`, all of their locks."""

    kind = 'joint_interp'

    @staticmethod
    def ordered_locks(devices):
        """The interpolator handles' own locks first, then every table's, each
        group by identity as `interpolator._HandleLocks` orders a handle's."""
        own = {id(d.lock.own): d.lock.own for d in devices}
        tables = {id(lock): lock for d in devices for lock in d.lock.of_tables}
        return ([own[k] for k in sorted(own)] +
                [tables[k] for k in sorted(tables)])


class _JointBase:
    """What a joint of tables and a joint of interpolators share: the parts
    of the joint axis, the operands of the likelihood, and every call on the
    draws -- ``(theta, )`` for tables, ``(theta, x)`` for interpolators, in
    the entries' arguments as the handle kind of `_lib.FORWARD_ENTRIES` and
    `_lib.GRAD_ENTRIES` has them.  A subclass says the `kind`, the owner of
    its handle, how draws are checked (`_draws`) and what an un-batched call
    reads from a model (`_model_draws`)."""

    kind = None
    _Device = None

    def _set_parts(self, members, part_tables=None, tables=None,
                   extra_keys=()):
        """`members`: what the handle is created from; `part_tables`: per
        member the table whose correlation function bins are its part of the
        joint axis; `tables`: every table a model must be consistent with
        (both: the members themselves); `extra_keys`: the parameters
        differentiated behind the model's."""
        self._members = members
        self._part_tables = part_tables or members
        self._tables = tables or members
        self._extra_keys = tuple(extra_keys)
        sizes = [len(halotab.tpcf_matrix) for halotab in self._part_tables]
        offsets = np.concatenate([[0], np.cumsum(sizes)])
        self.slices = [slice(int(offsets[k]), int(offsets[k + 1]))
                       for k in range(len(members))]
        self.n_r_total = int(offsets[-1])
        self._device = None

    def to_device(self):
        """Upload the members and create the joint handle (done lazily by the
        first call)."""
        devices = [member.to_device() for member in self._members]
        if self._device is None or any(
                a is not b for a, b in zip(self._device.devices, devices)):
            self._device = self._Device(devices)
        return self._device

    # -- arguments ------------------------------------------------------------

    def _operands(self, data, precision):
        """``data`` -- a flat ``(N, )`` vector or a list of per-table arrays
        -- and ``precision`` ``(N, N)``, contiguous, or a ValueError."""
        n = self.n_r_total
        if isinstance(data, (list, tuple)) and len(data) == len(self.slices) \
                and not np.isscalar(data[0]):
            parts = [np.ravel(np.asarray(part, dtype=np.float64))
                     for part in data]
            for k, part in enumerate(parts):
                size = self.slices[k].stop - self.slices[k].start
                if part.size != size:
                    raise ValueError('data of table {} must have {} entries, '
                                     'got {}.'.format(k, size, part.size))
            data = np.concatenate(parts)
        data = _lib.contiguous(data)
        precision = _lib.contiguous(precision)
        if data.shape != (n, ) or precision.shape != (n, n):
            raise ValueError('data must have {0} entries and precision shape '
                             '({0}, {0}).'.format(n))
        return data, precision

    def _split(self, array, leading):
        """The per-member parts of an array whose last axis is the joint one,
        each reshaped to ``leading + tpcf_shape``."""
        return [np.ascontiguousarray(array[..., part]).reshape(
            leading + tuple(halotab.tpcf_shape))
            for part, halotab in zip(self.slices, self._part_tables)]

    def _inputs(self, theta, n_gauss_prim, modulate_with_cenocc, assembias,
                family, x=None, extrapolate=False):
        """What follows the handle in an entry's arguments up to the operands
        -- the draws, checked here before any device is touched, theta's
        columns behind theta --; the family is in the flags."""
        _zheng07_only(family)
        draws = self._draws(theta, assembias, x, extrapolate)
        theta = draws[0]
        return (theta, theta.shape[1]) + tuple(draws[1:]) + (
            len(theta), n_gauss_prim,
            _flags(False, modulate_with_cenocc, assembias))

    # -- batched calls --------------------------------------------------------

    def _forward_call(self, form, inputs, operands=()):
        """The forward entry (``_lib.FORWARD_ENTRIES[kind, form, 'host']``)
        for checked `inputs`; the operands are checked here, before any device
        is touched: the results on the joint axis of ``n_r_total`` entries."""
        if operands:
            operands = self._operands(*operands)
        n_draws = len(inputs[0])
        shapes = ((n_draws, ), (n_draws, ) if operands else
                  (n_draws, self.n_r_total))
        return _forward.call(self.to_device(), self.kind, form, inputs, shapes,
                             operands)

    def _predict_batch(self, inputs):
        ngal, xi = self._forward_call('predict', inputs)
        return ngal, self._split(xi, (len(ngal), ))

    def _grad_call(self, inputs, operands=None, want_fisher=False):
        """The derivative entry for checked `inputs` (and operands checked
        here): the results on the joint axis of ``n_r_total`` entries."""
        if operands is not None:
            operands = self._operands(*operands)
        return _grad.call(
            self.to_device(), self.kind,
            _grad.family_of(bool(inputs[-1] & _lib.FLAG_ASSEMBIAS)), inputs,
            inputs[1] + len(self._extra_keys), (self.n_r_total, ), operands,
            want_fisher)

    def _predict_batch_grad(self, inputs):
        ngal, xi, dngal, dxi = self._grad_call(inputs)
        return (ngal, self._split(xi, dngal.shape[:1]), dngal,
                self._split(dxi, dngal.shape))

    def _fisher_batch(self, inputs, precision):
        ngal, _, dngal, _, fisher = self._grad_call(
            inputs, (np.zeros(self.n_r_total), precision), True)
        return ngal, dngal, fisher

    # -- un-batched forms -----------------------------------------------------

    def _model_call(self, batched, model, what, n_gauss_prim, extrapolate,
                    check_consistency, assembias, operands=()):
        """The public `batched` call for one model object: its results and
        the ``columns`` of `_grad.model_columns` that name the derivatives."""
        draws, options = self._model_draws(model, extrapolate)
        if check_consistency:
            for halotab in self._tables:
                halotab._check_consistency_cached(model)
        theta, model_options, columns, _ = _grad.model_columns(
            model, assembias, what, self._extra_keys)
        return batched(theta, *draws, *operands, n_gauss_prim=n_gauss_prim,
                       **options, **model_options), columns

    def _predict_grad(self, model, *arguments):
        (ngal, xis, dngal, dxis), columns = self._model_call(
            self.predict_batch_grad, model, 'predict_grad', *arguments)
        return (float(ngal[0]), [xi[0] for xi in xis],
                _grad.keyed(dngal[0], columns),
                {key: [dxi[0, k] for dxi in dxis]
                 for key, (k, _) in columns.items()})

    def _chi2_fisher(self, model, data, precision, *arguments):
        (ngal, chi2, dngal, dchi2, fisher), columns = self._model_call(
            self.chi2_fisher_batch, model, 'chi2_fisher', *arguments,
            operands=(data, precision))
        return (float(ngal[0]), float(chi2[0]), _grad.keyed(dngal[0], columns),
                _grad.keyed(dchi2[0], columns), fisher[0])


class JointLikelihood(_JointBase):
    """``JointLikelihood([halotab_wp, halotab_ds])``: 1 to 16 `TabCorr`
    tables with identical ``gal_type`` tables (mode ``'auto'`` and mode
    ``'cross'`` may be mixed).  The tables' results are concatenated in list
    order: table ``k`` owns ``joint.slices[k]`` of the ``joint.n_r_total``
    entries of ``data`` and of the rows and columns of ``precision``.

    Total correlation functions, float64 tables.  Which calls serve which
    model:

    - the calls that take ``theta`` -- `predict_batch`, `chi2_batch`,
      `predict_batch_grad`, `chi2_grad_batch`, `chi2_fisher_batch`,
      `fisher_batch` and the un-batched `predict_grad`, `chi2_fisher` --
      serve plain Zheng07 and, with ``assembias=True``, the model decorated
      with assembly bias (7 columns wherever 5 stand);
      ``family='leauthaud11'`` raises ``NotImplementedError``;
    - the calls that take the occupation array -- `predict_occupation`,
      `predict_vjp`, `chi2_occupation`, `chi2_grad_occupation` -- serve ANY
      occupation model, Leauthaud11 and custom ones among them: the caller
      contracts their results with the model's own ``d<N>/dtheta``.
    """

    kind = 'joint'
    _Device = _DeviceJoint

    def __init__(self, tabcorr_list):
        self.tabcorr_list = list(tabcorr_list)
        n_tables = len(self.tabcorr_list)
        if n_tables < 1 or n_tables > MAX_TABLES:
            raise ValueError('A joint takes 1 to {} tables, got {}.'.format(
                MAX_TABLES, n_tables))
        first = self.tabcorr_list[0]
        for k, halotab in enumerate(self.tabcorr_list):
            if any(halotab is other for other in self.tabcorr_list[:k]):
                raise ValueError(
                    'Table {} appears twice in the joint.'.format(k))
            if halotab.compute_dtype != 'float64':
                raise ValueError('Table {} does not have a float64 compute '
                                 'dtype.'.format(k))
            if not _same_bins(halotab.gal_type, first.gal_type):
                raise ValueError('Table {} does not have the gal_type table '
                                 'of table 0.'.format(k))
        self._set_parts(self.tabcorr_list)

    def _draws(self, theta, assembias, x, extrapolate):
        return (_grad_theta(theta, assembias), )

    def _model_draws(self, model, extrapolate):
        return (), {}

    # -- batched calls --------------------------------------------------------

    def predict_batch(self, theta, n_gauss_prim=10, modulate_with_cenocc=False,
                      assembias=False, family='zheng07'):
        """`TabCorr.predict_batch` of every table in one launch, without any
        derivative: the occupations once per draw, then every table's
        contraction.

        Returns
        -------
        ngal : ``(n_draws, )`` -- the tables share their bins: one per draw
        xis : list, per table ``(n_draws, ) + tpcf_shape``

        ``theta`` is ``(n_draws, 5)``, ``(n_draws, 7)`` with
        ``assembias=True``.  Raises ``NotImplementedError`` for
        ``family='leauthaud11'`` and for a joint the one-launch kernel does
        not serve: a mode ``'auto'`` table of more than 20 correlation
        function bins, or rows beyond the kernel's LDS."""
        return self._predict_batch(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family))

    def chi2_batch(self, theta, data, precision, n_gauss_prim=10,
                   modulate_with_cenocc=False, assembias=False,
                   family='zheng07'):
        """``chi2 = (xi - data)^T precision (xi - data)`` of the concatenated
        data vector for every draw, finished in the launch of `predict_batch`
        (``xi`` is never stored): ``ngal, chi2``, each ``(n_draws, )`` -- what
        an ensemble sampler asks per step.  ``data`` and ``precision`` as
        `chi2_grad_batch` takes them; the signature is the one
        `parallel.chi2_batch_sharded` calls a predictor with."""
        return self._forward_call('chi2', self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family),
            (data, precision))

    def predict_batch_grad(self, theta, n_gauss_prim=10,
                           modulate_with_cenocc=False, assembias=False,
                           family='zheng07'):
        """`TabCorr.predict_batch_grad` of every table in one launch.

        Returns
        -------
        ngal : ``(n_draws, )`` -- the tables share their bins: one per draw
        xis : list, per table ``(n_draws, ) + tpcf_shape``
        dngal : ``(n_draws, 5)``
        dxis : list, per table ``(n_draws, 5) + tpcf_shape``

        Raises ``NotImplementedError`` for ``family='leauthaud11'`` and for a
        joint whose rows do not fit the kernel's LDS.
        """
        return self._predict_batch_grad(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family))

    def chi2_grad_batch(self, theta, data, precision, n_gauss_prim=10,
                        modulate_with_cenocc=False, assembias=False,
                        family='zheng07'):
        """chi2 of the concatenated data vector and its gradient
        (`TabCorr.chi2_grad_batch` with ``N`` for ``n_r``): ``ngal, chi2``
        ``(n_draws, )``, ``dngal, dchi2`` ``(n_draws, 5)``."""
        return self._grad_call(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family),
            (data, precision))

    def chi2_fisher_batch(self, theta, data, precision, n_gauss_prim=10,
                          modulate_with_cenocc=False, assembias=False,
                          family='zheng07'):
        """`chi2_grad_batch` with the Fisher matrix ``fisher[:, k, l] =
        dxi_k^T P_sym dxi_l`` of the joint data vector, ``(n_draws, 5, 5)``,
        from the same launch (`TabCorr.chi2_fisher_batch`): the off-diagonal
        blocks of ``precision`` couple the tables."""
        return self._grad_call(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family),
            (data, precision), True)

    def fisher_batch(self, theta, precision, n_gauss_prim=10,
                     modulate_with_cenocc=False, assembias=False,
                     family='zheng07'):
        """The forecast form, which needs no data: ``ngal, dngal, fisher``."""
        return self._fisher_batch(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family),
            precision)

    # -- the occupation seam: any occupation model -----------------------------

    def _cotangents(self, g_xis, g_ngal, n_draws, batched):
        """``g_xis`` -- a list with one array per table of shape ``(n_draws, )
        + tpcf_shape``, or one ``(n_draws, N)`` array (without the leading
        axis when un-batched) -- on the joint axis, and ``g_ngal``: the
        cotangents as `_seam.cotangents` returns them, or a ValueError."""
        leading = (n_draws, ) if batched else ()
        if isinstance(g_xis, (list, tuple)):
            if len(g_xis) != len(self.tabcorr_list):
                raise ValueError('g_xis must hold one array per table ({}), '
                                 'got {}.'.format(len(self.tabcorr_list),
                                                  len(g_xis)))
            parts = []
            for k, (part, halotab) in enumerate(zip(g_xis,
                                                    self.tabcorr_list)):
                part = np.asarray(part, dtype=np.float64)
                shape = leading + tuple(halotab.tpcf_shape)
                if part.shape != shape:
                    raise ValueError('g_xis of table {} must have shape {}, '
                                     'got {}.'.format(k, shape, part.shape))
                parts.append(part.reshape(leading + (-1, )))
            g_xis = np.concatenate(parts, axis=-1)
        elif np.shape(g_xis) != leading + (self.n_r_total, ):
            raise ValueError('g_xis must be a list of per-table arrays or '
                             'have shape {}, got {}.'.format(
                                 leading + (self.n_r_total, ),
                                 np.shape(g_xis)))
        return _seam.cotangents(g_xis, g_ngal, n_draws, batched,
                                (self.n_r_total, ))

    def _predict_occupation(self, occupation, g_xis, g_ngal):
        """`predict_occupation` (``g_xis`` None) and `predict_vjp`: the
        arguments are checked before any device is touched."""
        occupation, batched = self.tabcorr_list[0]._vjp_occupation(occupation)
        n_draws = len(occupation)
        cotangents = None if g_xis is None else self._cotangents(
            g_xis, g_ngal, n_draws, batched)
        ngal, xi, g_occupation = _seam.call(
            self.to_device(), 'joint', 'predict', occupation,
            cotangents=cotangents)
        xis = self._split(xi, (n_draws, ))
        if not batched:
            ngal, xis = ngal[0], [part[0] for part in xis]
            g_occupation = None if g_xis is None else g_occupation[0]
        return ngal, xis, g_occupation

    def predict_occupation(self, occupation):
        """``predict(occupation)`` of every table in one launch, for ANY
        occupation model: ``ngal`` ``(n_draws, )`` and ``xis``, per table
        ``(n_draws, ) + tpcf_shape``.  ``occupation`` is ``(n_draws, n_bins)``
        in the row order of ``gal_type``, or ``(n_bins, )`` (un-batched: a
        float and arrays of ``tpcf_shape``).  Raises ``NotImplementedError``
        for a joint whose rows do not fit the kernel's LDS."""
        return self._predict_occupation(occupation, None, None)[:2]

    def predict_vjp(self, occupation, g_xis, g_ngal=None):
        """`predict_occupation` with its vector-Jacobian product with respect
        to the occupation array (`TabCorr.predict_vjp` for all the tables at
        once): ``g_occupation[d, i] = g_ngal[d] dngal[d] / dn[d, i] + sum_r
        g_xi[d, r] dxi[d, r] / dn[d, i]`` with ``r`` over the joint axis, in
        one kernel launch.  ``g_xis`` is a list with one array per table of
        shape ``(n_draws, ) + tpcf_shape``, or one ``(n_draws, N)`` array;
        ``g_ngal`` ``(n_draws, )`` or None = 0.  Returns ``ngal, xis,
        g_occupation``, the last ``(n_draws, n_bins)`` in the row order of
        ``gal_type``."""
        if g_xis is None:
            raise ValueError('g_xis is None: predict_occupation is the '
                             'forward-only call.')
        return self._predict_occupation(occupation, g_xis, g_ngal)

    def _chi2_occupation(self, occupation, data, precision, gradient):
        occupation, batched = self.tabcorr_list[0]._vjp_occupation(occupation)
        operands = self._operands(data, precision)
        ngal, chi2, dchi2 = _seam.call(
            self.to_device(), 'joint', 'chi2', occupation, operands=operands,
            gradient=gradient)
        if not batched:
            return ngal[0], chi2[0], dchi2[0] if gradient else None
        return ngal, chi2, dchi2

    def chi2_occupation(self, occupation, data, precision):
        """``chi2 = (xi - data)^T precision (xi - data)`` of the concatenated
        `predict_occupation`, finished in the launch: ``ngal, chi2``
        ``(n_draws, )`` (scalars for a 1-D occupation).  ``data`` and
        ``precision`` as `chi2_grad_batch` takes them."""
        return self._chi2_occupation(occupation, data, precision, False)[:2]

    def chi2_grad_occupation(self, occupation, data, precision):
        """`chi2_occupation` with its gradient with respect to the occupation
        array -- `predict_vjp` with ``g = 2 P_sym (xi - data)`` over the joint
        axis and ``g_ngal = 0``, formed on the device in the same launch, so
        that the off-diagonal blocks of ``precision`` couple the tables:
        ``ngal, chi2, dchi2_docc``, the last ``(n_draws, n_bins)`` in the row
        order of ``gal_type``.  Contracted with the caller's own
        ``d<N>/dtheta`` it is the gradient of the joint likelihood for EVERY
        occupation model (``examples/example_joint_custom_model_grad.py``:
        Leauthaud11)."""
        return self._chi2_occupation(occupation, data, precision, True)

    # -- un-batched forms -----------------------------------------------------

    def predict_grad(self, model, n_gauss_prim=10, check_consistency=True,
                     assembias=False):
        """Un-batched `predict_batch_grad` for a model object, as
        `TabCorr.predict_grad`: ``ngal`` (float), ``xis`` (list of arrays of
        each table's ``tpcf_shape``), ``dngal`` (dict by parameter name) and
        ``dxis`` (dict by parameter name of lists)."""
        return self._predict_grad(model, n_gauss_prim, False,
                                  check_consistency, assembias)

    def chi2_fisher(self, model, data, precision, n_gauss_prim=10,
                    check_consistency=True, assembias=False):
        """Un-batched `chi2_fisher_batch` for a model object: ``ngal``,
        ``chi2`` (floats), ``dngal``, ``dchi2`` (dicts by parameter name) and
        ``fisher`` ``(5, 5)`` in the order of the keys."""
        return self._chi2_fisher(model, data, precision, n_gauss_prim, False,
                                 check_consistency, assembias)


# ---- joint of interpolators ---------------------------------------------------

MAX_MEMBERS = 16


def _grid_nodes(interpolator):
    """The grid node (one index per axis) of every table of the list."""
    return [tuple(int(np.searchsorted(xp, value))
                  for xp, value in zip(interpolator.xp, point))
            for point in interpolator.points]


class JointInterpolator(_JointBase):
    """``JointInterpolator([interp_wp, interp_ds])``: 1 to 16 `Interpolator`
    members built over the same grid -- the same ``keys`` in the same order,
    bit-identical abscissae per axis -- whose tables share their ``gal_type``
    table grid node by grid node (the reference's AbacusSummit database reads
    a ``wp`` and a ``ds`` interpolator for one model).  A member is mode
    ``'auto'`` or mode ``'cross'`` throughout; the members may differ, and so
    may the orders of their lists: tables are matched by grid node, and the
    walk over the grid is member 0's.

    The members' results are concatenated in list order: member ``m`` owns
    ``joint.slices[m]`` of the ``joint.n_r_total`` entries of ``data`` and of
    the rows and columns of ``precision``.  Derivatives have ``5 + D`` columns
    -- `ZHENG07_KEYS`, then ``joint.keys`` -- and ``7 + D`` with
    ``assembias=True``.  One kernel launch per call (``tc_joint_interp_*``,
    ``include/tabcorr_amd.h``): the occupations of every class of halo tables
    once for all members, and chi2, its gradient and the Fisher matrix over
    ``(theta, x)`` against the full ``(N, N)`` precision matrix.  The forward
    calls `predict_batch` and `chi2_batch` -- what an ensemble sampler over
    ``(theta, x)`` asks per step -- take a launch of their own kind, without
    any derivative: a draw's results there depend on the draw alone, and
    permuting the members or the list of a member other than member 0 returns
    the same bits.
    """

    kind = 'joint_interp'
    _Device = _DeviceJointInterp

    def __init__(self, interpolators):
        from .interpolator import Interpolator
        self.interpolators = list(interpolators)
        n_members = len(self.interpolators)
        if n_members < 1 or n_members > MAX_MEMBERS:
            raise ValueError('A joint takes 1 to {} interpolators, got '
                             '{}.'.format(MAX_MEMBERS, n_members))
        for m, member in enumerate(self.interpolators):
            if not isinstance(member, Interpolator):
                raise ValueError(
                    'Member {} is not an Interpolator.'.format(m))
            if any(member is other for other in self.interpolators[:m]):
                raise ValueError(
                    'Member {} appears twice in the joint.'.format(m))
        first = self.interpolators[0]
        nodes = {node: k for k, node in enumerate(_grid_nodes(first))}
        for m, member in enumerate(self.interpolators):
            if list(member.keys) != list(first.keys):
                raise ValueError('Member {} does not have the keys of member '
                                 '0, in their order.'.format(m))
            if any(a.tobytes() != b.tobytes()
                   for a, b in zip(member.xp, first.xp)):
                raise ValueError('Member {} does not have the abscissae of '
                                 'member 0.'.format(m))
            mine = _grid_nodes(member)
            if sorted(mine) != sorted(nodes):
                raise ValueError('Member {} does not have the grid points of '
                                 'member 0.'.format(m))
            modes = {halotab.attrs['mode'] for halotab in member.tabcorr_list}
            if len(modes) != 1:
                raise ValueError('Member {} mixes the modes of its '
                                 'tables.'.format(m))
            for k, halotab in enumerate(member.tabcorr_list):
                if halotab.compute_dtype != 'float64':
                    raise ValueError('Member {}: table {} does not have a '
                                     'float64 compute dtype.'.format(m, k))
                partner = first.tabcorr_list[nodes[mine[k]]]
                if not _same_bins(halotab.gal_type, partner.gal_type):
                    raise ValueError(
                        'Member {}: table {} does not have the gal_type table '
                        "of member 0's table at its grid node.".format(m, k))
        self.keys = list(first.keys)
        self._set_parts(
            self.interpolators,
            [member.tabcorr_list[0] for member in self.interpolators],
            [halotab for member in self.interpolators
             for halotab in member.tabcorr_list], self.keys)

    def _draws(self, theta, assembias, x, extrapolate):
        """``theta (n, 5)`` -- ``(n, 7)`` decorated -- and ``x (n, D)``,
        checked as `Interpolator._grad_inputs` does."""
        return self.interpolators[0]._grad_inputs(theta, x, extrapolate,
                                                  assembias)

    def _model_draws(self, model, extrapolate):
        x = self.interpolators[0]._x_model(model)
        return (x[np.newaxis], ), {'extrapolate': extrapolate}

    # -- batched calls --------------------------------------------------------

    def predict_batch(self, theta, x, n_gauss_prim=10, extrapolate=False,
                      modulate_with_cenocc=False, assembias=False,
                      family='zheng07'):
        """`Interpolator.predict_batch` of every member in one launch, without
        any derivative: the occupations of every class of halo tables once for
        all members, then every member's contraction at every grid node.

        Returns
        -------
        ngal : ``(n_draws, )`` -- the members share their halo tables
        xis : list, per member ``(n_draws, ) + tpcf_shape``

        ``theta`` is ``(n_draws, 5)``, ``(n_draws, 7)`` with
        ``assembias=True``; ``x`` is ``(n_draws, D)``.  Raises ``ValueError``
        for ``x`` outside the grid unless ``extrapolate``,
        ``NotImplementedError`` for ``family='leauthaud11'`` and for a joint
        the one-launch kernel does not serve: a mode ``'auto'`` member of more
        than 20 correlation function bins or more than 248 bins, or rows
        beyond the kernel's LDS."""
        return self._predict_batch(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family, x,
            extrapolate))

    def chi2_batch(self, theta, x, data, precision, n_gauss_prim=10,
                   extrapolate=False, modulate_with_cenocc=False,
                   assembias=False, family='zheng07'):
        """``chi2 = (xi - data)^T precision (xi - data)`` of the concatenated
        data vector for every draw ``(theta, x)``, finished in the launch of
        `predict_batch` (``xi`` is never stored): ``ngal, chi2``, each
        ``(n_draws, )`` -- what an ensemble sampler over the model's and the
        grid's parameters asks per step.  ``data`` and ``precision`` as
        `chi2_grad_batch` takes them."""
        return self._forward_call('chi2', self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family, x,
            extrapolate), (data, precision))

    def predict_batch_grad(self, theta, x, n_gauss_prim=10, extrapolate=False,
                           modulate_with_cenocc=False, assembias=False,
                           family='zheng07'):
        """`Interpolator.predict_batch_grad` of every member in one launch.

        Returns
        -------
        ngal : ``(n_draws, )`` -- the members share their halo tables
        xis : list, per member ``(n_draws, ) + tpcf_shape``
        dngal : ``(n_draws, 5 + D)``
        dxis : list, per member ``(n_draws, 5 + D) + tpcf_shape``

        Raises ``ValueError`` for ``x`` outside the grid unless
        ``extrapolate``, ``NotImplementedError`` for
        ``family='leauthaud11'`` and for a joint whose rows do not fit the
        kernel's LDS.
        """
        return self._predict_batch_grad(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family, x,
            extrapolate))

    def chi2_grad_batch(self, theta, x, data, precision, n_gauss_prim=10,
                        extrapolate=False, modulate_with_cenocc=False,
                        assembias=False, family='zheng07'):
        """chi2 of the concatenated data vector and its gradient with respect
        to ``(theta, x)`` (`Interpolator.chi2_grad_batch` with ``N`` for
        ``n_r``): ``ngal, chi2`` ``(n_draws, )``, ``dngal, dchi2``
        ``(n_draws, 5 + D)``.  ``data`` is flat ``(N, )`` or a list of
        per-member arrays, ``precision`` ``(N, N)``."""
        return self._grad_call(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family, x,
            extrapolate), (data, precision))

    def chi2_fisher_batch(self, theta, x, data, precision, n_gauss_prim=10,
                          extrapolate=False, modulate_with_cenocc=False,
                          assembias=False, family='zheng07'):
        """`chi2_grad_batch` with the Fisher matrix ``fisher[:, k, l] =
        dxi_k^T P_sym dxi_l`` of the joint data vector over ``(theta, x)``,
        ``(n_draws, 5 + D, 5 + D)``, from the same launch: the off-diagonal
        blocks of ``precision`` couple the members."""
        return self._grad_call(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family, x,
            extrapolate), (data, precision), True)

    def fisher_batch(self, theta, x, precision, n_gauss_prim=10,
                     extrapolate=False, modulate_with_cenocc=False,
                     assembias=False, family='zheng07'):
        """The forecast form, which needs no data: ``ngal, dngal, fisher``."""
        return self._fisher_batch(self._inputs(
            theta, n_gauss_prim, modulate_with_cenocc, assembias, family, x,
            extrapolate), precision)

    # -- un-batched forms -----------------------------------------------------

    def predict_grad(self, model, n_gauss_prim=10, extrapolate=False,
                     check_consistency=True, assembias=False):
        """Un-batched `predict_batch_grad` for a model object whose
        ``param_dict`` holds the extra parameters, as
        `Interpolator.predict_grad`: ``ngal`` (float), ``xis`` (list of arrays
        of each member's ``tpcf_shape``), ``dngal`` (dict by the model keys,
        then ``self.keys``) and ``dxis`` (dict by the same keys of lists)."""
        return self._predict_grad(model, n_gauss_prim, extrapolate,
                                  check_consistency, assembias)

    def chi2_fisher(self, model, data, precision, n_gauss_prim=10,
                    extrapolate=False, check_consistency=True,
                    assembias=False):
        """Un-batched `chi2_fisher_batch` for a model object: ``ngal``,
        ``chi2`` (floats), ``dngal``, ``dchi2`` (dicts by the model keys, then
        ``self.keys``) and ``fisher`` ``(5 + D, 5 + D)`` in that order."""
        return self._chi2_fisher(model, data, precision, n_gauss_prim,
                                 extrapolate, check_consistency, assembias)
