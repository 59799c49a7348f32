"""The occupation seam of `TabCorr`, `JointLikelihood` and `Interpolator` --
`predict_occupation`, `predict_vjp`, `chi2_occupation`, `chi2_grad_occupation`:
one helper checks the cotangents, one allocates the outputs, calls the entry
`_lib.SEAM_ENTRIES` names under the handle's lock, checks the status and
returns the flat results."""

import math

import numpy as np

from . import _lib


def cotangents(g_xi, g_ngal, n_draws, batched, shape):
    """The cotangents of `predict_vjp`, contiguous: ``g_xi (n_draws, n_r)``
    from ``(n_draws, ) + shape`` and ``g_ngal (n_draws, )`` or None -- without
    the leading axis when not `batched` --, or a ValueError."""
    leading = (n_draws, ) if batched else ()
    g_xi = np.asarray(g_xi, dtype=np.float64)
    if g_xi.shape != leading + tuple(shape):
        raise ValueError('g_xi must have shape {}, got {}.'.format(
            leading + tuple(shape), g_xi.shape))
    g_xi = _lib.contiguous(g_xi.reshape(n_draws, math.prod(shape)))
    if g_ngal is not None:
        g_ngal = np.asarray(g_ngal, dtype=np.float64)
        if g_ngal.shape != leading:
            raise ValueError('g_ngal must have shape {}, got {}.'.format(
                leading, g_ngal.shape))
        g_ngal = _lib.contiguous(g_ngal.reshape(n_draws))
    return g_xi, g_ngal


def call(device, kind, form, occupation, x=None, cotangents=None,
         operands=None, gradient=True):
    """The seam entry of a handle `kind` (``'table'``, ``'joint'``,
    ``'interp'``) and `form` on `device`, the handle's wrapper, whose lock the
    call holds and whose ``n_r`` is the length of one draw's ``xi``.

    `occupation` and, for an interpolator, `x` are the checked contiguous
    arrays of the draws.  Form ``'predict'`` takes `cotangents` ``(g_xi,
    g_ngal)`` as `cotangents` above returns them (``g_ngal`` may be None), or
    None for the forward-only form; form ``'chi2'`` takes `operands` ``(data,
    precision)`` and is forward-only without `gradient`.  A forward-only call
    passes NULL for every derivative output (a table has no such form).

    Returns the flat arrays in the order of the C arguments: ``ngal (n, )``,
    ``xi (n, n_r)`` or ``chi2 (n, )``, the derivative with respect to the
    occupations in their shape and, for an interpolator, those with respect to
    x -- ``g_x``, or ``dchi2_dx`` and ``dngal_dx``; None for what a
    forward-only call leaves out.
    """
    predict = form == 'predict'
    n_draws = len(occupation)
    if predict:
        gradient = cotangents is not None
        g_xi, g_ngal = cotangents if gradient else (None, None)
        if gradient and g_xi.shape != (n_draws, device.n_r):
            raise ValueError('g_xi has {} entries per draw, the handle {}.'
                             .format(g_xi.shape[1:], device.n_r))
        middle = [g_ngal, g_xi]
    else:
        middle = list(operands)
    n_x = 0 if x is None else _lib.SEAM_X_OUTPUTS[form]
    # (in the order of the C arguments, as `_grad.call` says why)
    outputs = [np.empty(n_draws),
               np.empty((n_draws, device.n_r) if predict else n_draws)]
    if gradient:
        outputs.append(np.empty_like(occupation))
        outputs += [np.empty_like(x) for _ in range(n_x)]
    else:
        outputs += [None] * (1 + n_x)
    arrays = [occupation] if x is None else [occupation, x]
    arguments = [_lib.as_double_p(a) for a in arrays] + [n_draws, 0]
    arguments += [None if a is None else _lib.as_double_p(a)
                  for a in middle + outputs]
    with device.lock:
        _lib.check(getattr(device.lib, _lib.SEAM_ENTRIES[kind, form])(
            device.handle, *arguments))
    return tuple(outputs)
