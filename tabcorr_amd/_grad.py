"""The derivative calls of `TabCorr`, `Interpolator`, `JointLikelihood` and
`JointInterpolator`: one
helper allocates the outputs, calls the entry under the handle's lock, checks
the status and returns the results reshaped.  Which entry serves a (handle
kind, family, form) is `_lib.GRAD_ENTRIES`' to say."""

import math

import numpy as np

from . import _lib


def family_of(assembias=False, family='zheng07'):
    """The key of the model family in `_lib.GRAD_ENTRIES`."""
    return 'leauthaud11' if family == 'leauthaud11' else \
        'assembias' if assembias else 'zheng07'


def call(device, kind, family, inputs, n_cols, shape, operands=None,
         want_fisher=False):
    """The derivative entry of a handle `kind` (``'table'``, ``'interp'``,
    ``'joint'``, ``'joint_interp'``) and model `family` on `device` (the
    handle's wrapper, whose lock the call holds).

    `inputs` is what follows the handle up to the operands, the draws first:
    arrays are passed as pointers, everything else as it is.  `n_cols`
    columns are differentiated; `shape` is that of one draw's correlation
    function.  `operands` ``(data, precision)``: the likelihood form, with the
    Fisher matrix where `want_fisher`.

    Returns ``ngal (n, )``, ``xi (n, ) + shape``, ``dngal (n, n_cols)`` and
    ``dxi (n, n_cols) + shape``, or ``ngal, chi2 (n, )``, ``dngal, dchi2
    (n, n_cols)`` and, where wanted, ``fisher (n, n_cols, n_cols)``.
    """
    likelihood = operands is not None
    form = 'predict' if not likelihood else 'fisher' if want_fisher else 'chi2'
    name = _lib.GRAD_ENTRIES[kind, family, form]
    n_draws = len(inputs[0])
    wide = () if likelihood else (math.prod(shape), )
    # (in the order of the C arguments: a call's arrays are freed and taken
    # again by the next call, and the allocator reuses warm pages for this
    # order -- ngal, dngal, xi, dxi costs 13-16 us more per 10^4 draws)
    outputs = [np.empty(n_draws), np.empty((n_draws, ) + wide),
               np.empty((n_draws, n_cols)),
               np.empty((n_draws, n_cols) + wide)]
    if want_fisher:
        outputs.append(np.empty((n_draws, n_cols, n_cols)))
    arguments = [_lib.as_double_p(a) if isinstance(a, np.ndarray) else a
                 for a in inputs]
    arguments += [_lib.as_double_p(a) for a in operands or ()]
    arguments += [_lib.as_double_p(a) for a in outputs]
    if not want_fisher and name in _lib.GRAD_OPTIONAL_FISHER:
        arguments.append(None)
    with device.lock:
        _lib.check(getattr(device.lib, name)(device.handle, *arguments))
    if not likelihood:
        outputs[1] = outputs[1].reshape((n_draws, ) + tuple(shape))
        outputs[3] = outputs[3].reshape((n_draws, n_cols) + tuple(shape))
    return tuple(outputs)


def keyed(values, keys=None, columns=None):
    """One draw's derivatives by parameter name: ``{key: values[k]}`` for the
    ``k``-th of `keys`, or ``{key: factor * values[k]}`` for `columns` ``{key:
    (k, factor)}``; floats where `values` is a vector."""
    pick = float if np.ndim(values) == 1 else (lambda value: value)
    if columns is None:
        return {key: pick(values[k]) for k, key in enumerate(keys)}
    return {key: pick(factor * values[k])
            for key, (k, factor) in columns.items()}
