"""The forward calls of `TabCorr` and `Interpolator` -- predictions and
likelihoods, synchronous and asynchronous: allocate or stage the outputs, call
the entry `_lib.FORWARD_ENTRIES` names under the handle's lock, check the
status, return the results.  `inputs` is what follows the handle up to the
operands: ``(theta, n_theta, ...)`` of a table, ``(theta, n_theta, x, ...)``
of an interpolator or a joint of interpolators; `shapes` those of the two results; `operands` ``(data,
precision)`` of a likelihood.  A microsecond is 2 % of a small call: the
arguments are spelt out, not looped over."""

import ctypes

from numpy import empty

from . import pinned
from ._lib import (FLAG_SEPARATE_GAL_TYPE, FORWARD_ENTRIES, as_double_p as p,
                   check)


def shapes(table, n_draws, flags, likelihood):
    """Of the two results of `n_draws` draws on `table` (a table's wrapper)."""
    if likelihood:
        return (n_draws, ), (n_draws, )
    if flags & FLAG_SEPARATE_GAL_TYPE:
        return (n_draws, 2), (n_draws, table.n_components, table.n_r)
    return (n_draws, 1), (n_draws, 1, table.n_r)


def _run(device, kind, form, route, inputs, operands, outputs, *ticket):
    if kind in ('interp', 'joint_interp'):
        inputs = (p(inputs[0]), inputs[1], p(inputs[2])) + inputs[3:]
    else:
        inputs = (p(inputs[0]), ) + inputs[1:]
    if operands:
        inputs += (p(operands[0]), p(operands[1]))
    entry = getattr(device.lib, FORWARD_ENTRIES[kind, form, route])
    with device.lock:
        check(entry(device.handle, *inputs, p(outputs[0]), p(outputs[1]),
                    *ticket))


def call(device, kind, form, inputs, shapes, operands=(), out=None):
    """The synchronous host-array entry of a handle `kind` (``'table'``,
    ``'interp'``, ``'joint'``: a joint of tables, called as a table,
    ``'joint_interp'``: a joint of interpolators, called as an interpolator)
    and `form` (``'predict'``, ``'chi2'``) on `device`, the
    handle's wrapper.  `out`: the caller's arrays for the results, else new
    ones (allocated in the order of the C arguments, as `_grad.call`)."""
    outputs = (empty(shapes[0]), empty(shapes[1])) if out is None else \
        pinned.caller_outputs(shapes, out)
    _run(device, kind, form, 'host', inputs, operands, outputs)
    return outputs


def call_async(device, kind, form, inputs, shapes, package, operands=(),
               out=None):
    """`call` without waiting: theta (and x) are staged in page-locked memory
    unless they are there already, the results go to `out` (page-locked) or to
    pooled page-locked blocks, and the `tabcorr_amd.pinned.PendingPrediction`
    that is returned gives ``package(*results)`` at ``wait()``."""
    outputs, pooled_out = pinned.stage_outputs(shapes, out)
    where = (0, 2) if kind == 'interp' else (0, )
    staged, pooled_in = pinned.stage_inputs([inputs[k] for k in where])
    inputs = list(inputs)
    for k, array in zip(where, staged):
        inputs[k] = array
    ticket = ctypes.c_int64(-1)
    _run(device, kind, form, 'async', tuple(inputs), operands, outputs,
         ctypes.byref(ticket))
    stem = 'tc_%s_' % kind
    return pinned.PendingPrediction(
        device, getattr(device.lib, stem + 'wait'),
        getattr(device.lib, stem + 'query'), ticket.value, staged, outputs,
        pooled_in, pooled_out, package)
