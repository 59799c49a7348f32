"""The derivative calls of `TabCorr`, `Interpolator`, `JointLikelihood` and
`JointInterpolator`: one
helper allocates the outputs, calls the entry under the handle's lock, checks
the status and returns the results reshaped.  Which entry serves a (handle
kind, family, form) is `_lib.GRAD_ENTRIES`' to say.  Their un-batched forms
take a model object: `model_columns` says what the batched call is given for
it and how its columns are named, `keyed` and `carried` name the results."""

import math

import numpy as np

from . import _lib
from .models import (LEAUTHAUD11_GRAD_KEYS, LEAUTHAUD11_KEYS,
                     ZHENG07_ASSEMBIAS_KEYS, ZHENG07_KEYS, device_spec)


def family_of(assembias=False, family='zheng07'):
    """The key of the model family in `_lib.GRAD_ENTRIES`."""
    return 'leauthaud11' if family == 'leauthaud11' else \
        'assembias' if assembias else 'zheng07'


def keys_of(assembias=False, family='zheng07'):
    """The differentiated model parameters, in column order."""
    if family == 'leauthaud11':
        return LEAUTHAUD11_GRAD_KEYS
    return ZHENG07_ASSEMBIAS_KEYS if assembias else ZHENG07_KEYS


def model_columns(model, assembias, what, extra_keys=(), leauthaud11=False):
    """The model of the un-batched call `what` as its batched call takes it:
    plain Zheng07 -- with `assembias` Zheng07 decorated with assembly bias;
    `leauthaud11`: the caller serves a `Leauthaud11Model` too.  Any other
    model is refused.  `extra_keys`: the parameters differentiated behind the
    model's (an interpolator's axes).

    Returns the ``(1, n)`` row of draws; the keyword arguments of the batched
    call that say the model; ``columns`` ``{key: (k, factor)}`` for `keyed`,
    in key order -- a Zheng07 key its own column with factor 1.0, each of the
    sixteen `LEAUTHAUD11_KEYS` one of the eleven device columns (``smhm_X_0``
    and ``smhm_X_a`` the relation's X, the other six their own) by its entry
    of `Leauthaud11Model.device_jacobian` (zero for ``smhm_X_a`` at redshift
    0), `extra_keys` theirs behind the model's with 1.0; and ``jacobian``,
    which carries a Fisher matrix of the device columns to the keys as ``J^T
    F J``: None for Zheng07, whose matrix stays as it is (it may hold inf),
    else the block-diagonal matrix of `device_jacobian` and the identity of
    the extra parameters."""
    spec = device_spec(model)
    if (leauthaud11 and not assembias and spec is not None and
            spec.family == 'leauthaud11'):
        options = {'family': 'leauthaud11'}
        own = model.device_jacobian()
        n_model, n_extra = own.shape[0], len(extra_keys)
        columns = {}
        for j, key in enumerate(LEAUTHAUD11_KEYS):
            k = j // 2 if j < 10 else j - 5
            columns[key] = (k, float(own[k, j]))
        jacobian = np.zeros((n_model + n_extra, own.shape[1] + n_extra))
        jacobian[:n_model, :own.shape[1]] = own
        jacobian[n_model:, own.shape[1]:] = np.eye(n_extra)
        theta = spec.theta[np.newaxis]
    else:
        if not assembias:
            if spec is None or spec.family != 'zheng07' or spec.assembias:
                raise NotImplementedError(
                    '{} needs a plain Zheng07 model (no assembly bias, no '
                    'other family).'.format(what))
        elif spec is None or spec.family != 'zheng07' or not spec.assembias:
            raise ValueError(
                '{} with assembias=True needs a Zheng07 model decorated with '
                'assembly bias.'.format(what))
        options = {'assembias': assembias}
        keys = keys_of(assembias)
        n_model, jacobian = len(keys), None
        columns = {key: (k, 1.0) for k, key in enumerate(keys)}
        theta = spec.theta[np.newaxis, :n_model]
    options['modulate_with_cenocc'] = spec.modulate_with_cenocc
    for d, key in enumerate(extra_keys):
        columns[key] = (n_model + d, 1.0)
    return theta, options, columns, jacobian


def carried(fisher, jacobian):
    """One draw's Fisher matrix in the keys of `model_columns`: ``J^T F J``,
    or ``F`` itself for no `jacobian` -- never a product then: ``inf * 0``
    would make NaN of an entry that is legitimately inf."""
    return fisher if jacobian is None else jacobian.T @ fisher @ jacobian


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


def keyed(values, columns):
    """One draw's derivatives by parameter name: ``{key: factor * values[k]}``
    for the `columns` ``{key: (k, factor)}`` of `model_columns` (a factor of
    1.0 keeps every bit); floats where `values` is a vector."""
    pick = float if np.ndim(values) == 1 else (lambda value: value)
    return {key: pick(factor * values[k])
            for key, (k, factor) in columns.items()}
