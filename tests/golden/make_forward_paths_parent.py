"""Records the forward paths that call_paths_parent.npz does not reach -- the staggered chunks of a
large synchronous call, the direct loads and stores of asynchronous calls and of chunks, a
synchronous interpolator call separated by galaxy type in chunks, and the single asynchronous
call that a reused ticket ring must reproduce -- on an MI355X, into forward_paths_parent.npz:
python tests/golden/make_forward_paths_parent.py

Run it with the library of the commit whose bits are the reference (the parent of the change
that gives the forward calls one request, one chunk plan and one ticket ring);
tests/test_gpu_forward_paths.py then asks every later library for the same bits.  It is a second
recorder in the style of make_call_paths_parent.py, whose tables, draws and handles it uses.

Per case the file holds the (workgroups, waves, slabs, LDS bytes) of the last launch and the
results as float64 words; a case of 4096 draws or more is kept as the SHA-256 of its result bytes
and the words of its first and last 64 draws.  A case with a `base` is kept as the exclusive-or
with the base's words.  Every case is run twice on fresh handles; one whose words do not repeat is
listed under `unrepeatable`, and the test compares it with the oracle only.
"""

import ctypes
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
FILE = os.path.join(HERE, 'forward_paths_parent.npz')


def load_call_paths():
    spec = importlib.util.spec_from_file_location(
        'make_call_paths_parent', os.path.join(HERE, 'make_call_paths_parent.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


base = load_call_paths()

# The smallest table whose synchronous call takes the staggered path: float32, 6 mass bins x 1,
# n_r = 256, so that 8192 draws give 16.8 MB of results (past 16 MB) of 2056 bytes per draw.
STAGGER = dict(n_prim=6, n_sec=1, tpcf_shape=(16, 16), mode='auto', dtype='float32', seed=6 + 256)
N_STAGGER = 8192
MAX_TICKETS = 64        # (csrc/predict_call.h: Tickets::kMaxTickets)
N_RING = MAX_TICKETS + 3


def cases():
    """(name, dict) of every recorded case, a case's base before it."""
    out = []

    def add(name, target, entry, **case):
        case.update(target=target, entry=entry)
        for key, value in (('chi2', False), ('separate', False), ('degenerate', False),
                           ('n_draws', base.N_DRAWS), ('options', ()), ('base', None)):
            case.setdefault(key, value)
        out.append((name, case))
    # staggered chunks: the automatic six, four at 50 %, and six at 1 % (whose last is empty in
    # the parent's arithmetic)
    for tag, options in (('default', ()),
                         ('4_50', (('sync_chunks', 4), ('sync_stagger', 50))),
                         ('6_1', (('sync_chunks', 6), ('sync_stagger', 1)))):
        add('stagger_' + tag, 'stagger', 'host', n_draws=N_STAGGER, options=options,
            base=None if tag == 'default' else 'stagger_default')
    # which arrays an asynchronous call's kernels address in the caller's memory themselves
    for direct_in in (0, 1):
        for direct_out in (0, 1, 2):
            name = 'auto19_async_in%d_out%d' % (direct_in, direct_out)
            add(name, 'auto19', 'async',
                options=(('async_direct_in', direct_in), ('async_direct_out', direct_out)),
                base=None if (direct_in, direct_out) == (0, 0) else 'auto19_async_in0_out0')
    # ... and a chunk's
    for direct_out in (0, 1, 2):
        add('auto19_chunks2_out%d' % direct_out, 'auto19', 'host', n_draws=base.N_LARGE,
            options=(('sync_chunks', 2), ('sync_direct_out', direct_out)),
            base=None if direct_out == 0 else 'auto19_chunks2_out0')
    # the single asynchronous call every call of the ticket-ring test repeats
    add('auto19_ring', 'auto19', 'async', base='auto19_async_in0_out0')
    add('interp_cross_ring', 'interp_cross', 'async')
    # a synchronous interpolator call in three chunks, separated by galaxy type
    for target in ('interp_auto', 'interp_cross'):
        add(target + '_separate_chunks3', target, 'host', separate=True, n_draws=base.N_LARGE,
            options=(('sync_chunks', 3), ))
    return out


def tables_of(target):
    if target != 'stagger':
        return base.tables_of(target)
    from tabcorr_amd import synthetic
    s = STAGGER
    return [synthetic.synthetic_table(s['n_prim'], s['n_sec'], s['tpcf_shape'], s['mode'],
                                      seed=s['seed'])], None, None


def dtype_of(target):
    return STAGGER['dtype'] if target == 'stagger' else base.dtype_of(target)


class Target(base.Target):
    """make_call_paths_parent.Target, and the staggered table."""

    def __init__(self, target, options=()):
        if target != 'stagger':
            super().__init__(target, options)
            return
        from tabcorr_amd import TabCorr, _lib
        self.lib = _lib.load()
        (table, ), _, self.points = tables_of(target)
        self.halotab = TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'],
                                           table['tpcf_shape'], table['attrs'],
                                           compute_dtype=dtype_of(target))
        self.halotabs, self.interpolator = [self.halotab], None
        self.n_r = self.halotab.to_device().n_r
        self.set_options(options)


def run_case(case):
    """The case on fresh handles: {'launch': ..., name: float64 array (n_draws, values)}."""
    target = Target(case['target'], case['options'])
    out = target.call(case)
    out['launch'] = target.last_launch()
    return out


def ring(target_name):
    """N_RING asynchronous predictions of the 81 draws in flight on one fresh handle, each into
    page-locked outputs of its own, nothing waited for; then ticket 0 (its slot reused) and the
    last ticket are queried and waited for.  Returns the results of every call as run_case
    gives them and {'tickets', 'done_after_wait': {ticket: flag}, 'never_issued': status}."""
    from tabcorr_amd import _lib, pinned_empty
    target = Target(target_name)
    interp = target.interpolator is not None
    owner = target.interpolator if interp else target.halotab
    device = owner.to_device()
    lib = target.lib
    case = dict(cases())[target_name + '_ring']
    theta = base.theta_of(case)
    args = [theta] + ([base.x_of(case, target.points)] if interp else [])
    kwargs = {'extrapolate': True} if interp else {}
    outs = [(pinned_empty((len(theta), 1)), pinned_empty((len(theta), 1, target.n_r)))
            for _ in range(N_RING)]
    pending = [owner.predict_batch_async(*args, out=out, **kwargs) for out in outs]
    query, wait = ((lib.tc_interp_query, lib.tc_interp_wait) if interp
                   else (lib.tc_table_query, lib.tc_table_wait))
    report = {'tickets': [p.ticket for p in pending], 'done_after_wait': {}}
    flag = ctypes.c_int(-1)
    with device.lock:
        for ticket in (pending[0].ticket, pending[-1].ticket):
            _lib.check(query(device.handle, ticket, ctypes.byref(flag)))
            assert flag.value in (0, 1)
            _lib.check(wait(device.handle, ticket))
            _lib.check(query(device.handle, ticket, ctypes.byref(flag)))
            report['done_after_wait'][ticket] = flag.value
        report['never_issued'] = (query(device.handle, pending[-1].ticket + 1, ctypes.byref(flag)),
                                  wait(device.handle, pending[-1].ticket + 1))
    results = []
    for p in pending:
        ngal, xi = p.wait()
        results.append({'ngal': np.array(ngal).reshape(len(theta), -1),
                        'xi': np.array(xi).reshape(len(theta), -1)})
    return results, report


def pack(results, unrepeatable):
    """{case: {key: array}} -> the arrays of the file."""
    arrays, index = {}, {'unrepeatable': sorted(unrepeatable), 'cases': {}}
    stored = {name: base.stored_form(case, results[name]) for name, case in cases()}
    for name, case in cases():
        entries = []
        for key in sorted(stored[name]):
            value = stored[name][key]
            words = value.view(np.uint64) if key != 'launch' else value
            other = stored[case['base']].get(key) if case['base'] else None
            against = (other is not None and key != 'launch' and not key.endswith('#') and
                       other.shape == value.shape)
            if against:
                words = words ^ other.view(np.uint64)
            arrays['%s/%s' % (name, key)] = words
            entries.append([key, against])
        index['cases'][name] = entries
    arrays['index'] = np.array(json.dumps(index))
    return arrays


def unpack(data):
    """The arrays of the file -> ({case: {key: array, key + '#': digest, 'launch': array}},
    unrepeatable names).  Of a large case the arrays are its first and last 64 draws."""
    index = json.loads(str(data['index']))
    results = {}
    for name, case in cases():
        result = {}
        for key, against in index['cases'][name]:
            words = data['%s/%s' % (name, key)]
            if against:
                words = words ^ results[case['base']][key].view(np.uint64)
            result[key] = (words if key == 'launch' else words.view(np.uint8) if key.endswith('#')
                           else words.view(np.float64))
        results[name] = result
    return results, set(index['unrepeatable'])


if __name__ == '__main__':
    sys.path.insert(0, REPO)
    results, unrepeatable = {}, set()
    for name, case in cases():
        results[name] = run_case(case)
        again = run_case(case)
        if not all(base.same_words(results[name][key], again[key]) for key in results[name]):
            unrepeatable.add(name)
        print(name, results[name]['launch'], 'UNREPEATABLE' if name in unrepeatable else '',
              flush=True)
    for target in ('auto19', 'interp_cross'):
        calls, report = ring(target)
        single = results[target + '_ring']
        same = all(base.same_words(call[key], single[key]) for call in calls for key in call)
        print(target, 'ring:', report, 'every call the single call\'s bits:', same, flush=True)
    target = sys.argv[1] if len(sys.argv) > 1 else FILE
    np.savez_compressed(target, **pack(results, unrepeatable))
    recorded, listed = unpack(np.load(target))
    assert listed == unrepeatable
    for name, case in cases():
        for key, value in base.stored_form(case, results[name]).items():
            assert recorded[name][key].tobytes() == value.tobytes(), (name, key)
    print('%s: %d cases, %d unrepeatable %s, %d bytes' % (
        target, len(results), len(unrepeatable), sorted(unrepeatable), os.path.getsize(target)))
