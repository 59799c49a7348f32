"""Records what every entry point of the prediction path returns -- host arrays, device pointers,
asynchronous calls, un-batched walkers, the chunks of a large synchronous call, the interpolator's
twins of them -- on an MI355X, into call_paths_parent.npz:
python tests/golden/make_call_paths_parent.py

Run it with the library of the commit whose bits are the reference (the parent of the change
that passes a call's lane, likelihood target and chunk hints down the launch path as an argument
instead of writing them on the handle); tests/test_gpu_call_paths.py then asks every later library
for the same bits.  `cases()` and `run_case()` are what that test evaluates too.

The file holds, per case, the (workgroups, waves, slabs, LDS bytes) of the last launch and the
results as float64 words, one vector per case (`index` names the arrays in it).  A case whose
`base` runs the same table and draws through another entry point is kept as the exclusive-or with
the base's words; the later calls of a case of consecutive calls share their first 64 draws with
the first and are kept as the exclusive-or with its words.  A case of 4096 draws or more is kept
as the SHA-256 of its result bytes and the words of its first and last 64 draws (which are the
first 64 of the 81-draw cases, so that they too are kept against a base).  Every case is run twice
on fresh handles; one whose words do not repeat is listed under `unrepeatable`, and the test
compares it with the oracle only.
"""

import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
FILE = os.path.join(HERE, 'call_paths_parent.npz')

N_DRAWS = 81            # two tiles of 64 draws, the second partial
N_LARGE = 4096          # 19 r values: 884 KB of draws and results, beyond the zero-copy limit
N_EDGE = 64             # draws kept of either end of a large case
MAX_SLAB = 1 << 18      # (csrc/internal.h: kMaxSlab; what max_slab() gives tables of few bins)
GRID = (4, )            # the smallest interpolator grid of the parent fixtures
# (the draws degenerate_draws replaces, in either tile)
DEGENERATE_ROWS = tuple(range(1, 13)) + tuple(range(65, 77))

# (n_prim, n_sec, n_r), mode, dtype.  The (9, 2, 19) tables are the first tables of the two
# interpolators: tables that are also called directly.
TABLES = {
    'auto19': ((9, 2, 19), 'auto', 'float64'),      # one-launch forms
    'cross19': ((9, 2, 19), 'cross', 'float64'),
    'auto34': ((12, 2, 34), 'auto', 'float64'),     # more than 32 rows: launch_chi2 by itself
    'auto40': ((30, 2, 40), 'auto', 'float64'),     # three kernels, several r tiles
    'f32': ((10, 2, 7), 'cross', 'float32'),
}
INTERPOLATORS = {'interp_auto': 'auto19', 'interp_cross': 'cross19'}


def cases():
    """(name, dict) of every recorded case, a case's base before it."""
    out = []

    def add(name, target, entry, **case):
        case.update(target=target, entry=entry)
        for key, value in (('chi2', False), ('separate', False), ('degenerate', False),
                           ('n_draws', N_DRAWS), ('options', ()), ('base', None)):
            case.setdefault(key, value)
        out.append((name, case))
    for target in list(TABLES) + list(INTERPOLATORS):
        # prediction and likelihood through the host-array, _device and _async symbols
        for chi2 in (False, True):
            tag = '_chi2' if chi2 else '_predict'
            add(target + '_host' + tag, target, 'host', chi2=chi2)
            for entry in ('device', 'async'):
                add('%s_%s%s' % (target, entry, tag), target, entry, chi2=chi2,
                    base=target + '_host' + tag)
    for target in ('auto19', 'cross19', 'interp_auto', 'interp_cross'):
        # degenerate draws, every entry point
        for chi2 in (False, True):
            tag = '_chi2' if chi2 else '_predict'
            for entry in ('host', 'device', 'async'):
                add('%s_%s%s_degenerate' % (target, entry, tag), target, entry, chi2=chi2,
                    degenerate=True, base=target + '_host' + tag + (
                        '' if entry == 'host' else '_degenerate'))
        # the chunks of a large synchronous call
        for chi2 in (False, True):
            tag = '_chi2' if chi2 else '_predict'
            for chunks in (-1, 2, 3):
                add('%s_large%s_chunks%d' % (target, tag, chunks), target, 'host', chi2=chi2,
                    n_draws=N_LARGE, options=(('sync_chunks', chunks), ),
                    base=target + '_host' + tag if chunks == -1
                    else '%s_large%s_chunks-1' % (target, tag))
        # n_lanes + 1 consecutive _device calls on default lanes
        add(target + '_ordered_off', target, 'pipelined', options=(('ordered', 0), ),
            base=target + '_host_predict')
        add(target + '_ordered_on', target, 'pipelined', options=(('ordered', 1), ),
            base=target + '_ordered_off')
    for target in ('auto19', 'cross19'):
        # separated by galaxy type
        add(target + '_host_separate', target, 'host', separate=True)
        add(target + '_device_separate', target, 'device', separate=True,
            base=target + '_host_separate')
    for target in TABLES:
        for walkers in (1, 5):
            add('%s_many%d' % (target, walkers), target, 'many', n_draws=walkers)
    add('auto19_many5_degenerate', 'auto19', 'many', n_draws=5, degenerate=True)
    # batch-invariant forms
    for entry in ('host', 'device', 'async'):
        add('auto19_%s_deterministic2' % entry, 'auto19', entry, options=(('deterministic', 2), ),
            base='auto19_host_predict' if entry == 'host' else 'auto19_host_deterministic2')
    add('auto19_many1_deterministic2', 'auto19', 'many', n_draws=1,
        options=(('deterministic', 2), ))
    # more than one slab: the only place where the "one slab" rule switches the fused likelihood off
    add('auto19_slabs_chi2', 'auto19', 'host', chi2=True, n_draws=MAX_SLAB + 17)
    return out


def is_digest(case):
    return case['n_draws'] >= N_LARGE


def tables_of(target):
    """The table dicts behind a target: one, or the interpolator's with (keys, points)."""
    from tabcorr_amd import synthetic
    name = INTERPOLATORS.get(target, target)
    (n_prim, n_sec, n_r), mode, dtype = TABLES[name]
    if name in INTERPOLATORS.values():
        tables, keys, points = synthetic.synthetic_interpolator(GRID, n_prim, n_sec, (n_r, ), mode,
                                                                seed=n_prim)
        return (tables, keys, points) if target in INTERPOLATORS else ([tables[0]], None, None)
    return [synthetic.synthetic_table(n_prim, n_sec, (n_r, ), mode, seed=n_prim + n_r)], None, None


def dtype_of(target):
    return TABLES[INTERPOLATORS.get(target, target)][2]


def degenerate_draws(theta):
    """test_gpu_grouped.py: degenerate_draws, in either tile (as far as the batch has them)."""
    theta = theta.copy()
    for first in (0, 64):
        rows = theta[first:]
        for row, column, value in ((1, 0, np.nan), (2, 1, 0.0), (3, 1, np.nan), (4, 2, np.nan),
                                   (5, 3, np.nan), (6, 4, np.nan), (7, 3, -400.0), (8, 2, 400.0),
                                   (9, 0, np.inf), (10, 0, -np.inf), (12, 2, 15.5)):
            if row < len(rows):
                rows[row, column] = value
        if len(rows) > 11:
            rows[11, :5] = [12.0, 0.0, 11.0, 13.0, 1.0]      # a step exactly on a bin edge
    return theta


def theta_of(case, call=0):
    """The draws of a case; `call`: of the call-th of its consecutive calls (the first tile of
    64 draws is the first call's).  A large case begins and ends with the first 64 draws of the
    81-draw cases."""
    from tabcorr_amd import synthetic
    n = case['n_draws']
    theta = synthetic.zheng07_draws(n, seed=n)
    if call > 0:
        theta[64:] = synthetic.zheng07_draws(n, seed=n + 7 * call)[64:]
    if is_digest(case):
        theta[:N_EDGE] = theta[-N_EDGE:] = synthetic.zheng07_draws(N_DRAWS, seed=N_DRAWS)[:N_EDGE]
    return degenerate_draws(theta) if case['degenerate'] else theta


def x_of(case, points, call=0):
    """The draws' coordinates on the interpolator's axis, as theta_of: 10 % beyond either end,
    draw 3 on the right edge, draw 4 on the left."""
    a = np.unique(points[:, 0])

    def uniform(n, seed):
        x = np.random.default_rng(seed).uniform(a[0] - 0.1 * (a[-1] - a[0]),
                                                a[-1] + 0.1 * (a[-1] - a[0]), (n, 1))
        x[3], x[4] = a[-1], a[0]
        return x
    n = case['n_draws']
    x = uniform(n, n)
    if call > 0:
        x[64:] = uniform(n, n + call)[64:]
    if is_digest(case):
        x[:N_EDGE] = x[-N_EDGE:] = uniform(N_DRAWS, N_DRAWS)[:N_EDGE]
    return x


def likelihood_of(n_r):
    """Data vector and weight matrix of the likelihood cases (fixed numbers, no device)."""
    rng = np.random.default_rng(n_r)
    vector = np.geomspace(30.0, 0.05, n_r)
    a = rng.normal(size=(n_r, n_r))
    return vector, a @ a.T / np.mean(vector)**2


class Target:
    """Fresh handles of a case's target: `halotab`, or `interpolator` over `halotabs`."""

    def __init__(self, target, options=()):
        from tabcorr_amd import Interpolator, TabCorr, _lib
        self.lib = _lib.load()
        tables, keys, self.points = tables_of(target)
        self.halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'],
                                             t['attrs'], compute_dtype=dtype_of(target))
                         for t in tables]
        self.halotab = self.halotabs[0]
        self.interpolator = None
        if keys is not None:
            self.interpolator = Interpolator(self.halotabs, {keys[0]: self.points[:, 0]})
            self.interpolator.to_device()
        self.n_r = self.halotab.to_device().n_r
        self.set_options(options)

    def set_options(self, options):
        from tabcorr_amd import _lib
        for halotab in self.halotabs:
            for key, value in options:
                _lib.check(self.lib.tc_table_set_option(halotab.to_device().handle, key.encode(),
                                                        value))

    def n_lanes(self):
        return 4            # (csrc/internal.h: Tuning::lanes)

    def last_launch(self):
        from tabcorr_amd import _lib
        launch = [ctypes.c_int() for _ in range(4)]
        _lib.check(self.lib.tc_table_last_launch(self.halotab.to_device().handle,
                                                 *[ctypes.byref(v) for v in launch]))
        return np.array([v.value for v in launch], dtype=np.int64)

    def device_calls(self, calls, chi2, separate):
        """Consecutive calls of the _device symbol, one per (theta, x) of `calls`, then one
        synchronisation: [(ngal, second)] per call."""
        from tabcorr_amd import _lib
        lib = self.lib
        interp = self.interpolator is not None
        device = (self.interpolator if interp else self.halotab).to_device()
        table = self.halotab.to_device()
        n_comp = table.n_components if separate else 1
        flags = _lib.FLAG_SEPARATE_GAL_TYPE if separate else 0
        vector, precision = (np.ascontiguousarray(a) for a in likelihood_of(self.n_r))
        pointers, results = [], []

        def on_device(array):
            ptr = ctypes.c_void_p()
            _lib.check(lib.tc_device_malloc(ctypes.byref(ptr), max(array.nbytes, 8)))
            pointers.append(ptr)
            return ptr
        try:
            with device.lock:
                for theta, x in calls:
                    n = len(theta)
                    ngal = np.empty((n, 2 if separate else 1))
                    second = np.empty(n) if chi2 else np.empty((n, n_comp, self.n_r))
                    inputs = [np.ascontiguousarray(theta)] + ([np.ascontiguousarray(x)]
                                                              if interp else [])
                    d_in = [on_device(a) for a in inputs]
                    for array, ptr in zip(inputs, d_in):
                        _lib.check(lib.tc_memcpy_h2d(ptr, array.ctypes.data_as(ctypes.c_void_p),
                                                     array.nbytes))
                    d_out = [on_device(ngal), on_device(second)]
                    head = [device.handle, d_in[0], theta.shape[1]] + d_in[1:] + [n, 10, flags]
                    if chi2:
                        head += [_lib.as_double_p(vector), _lib.as_double_p(precision)]
                    name = 'tc_%s%s_zheng07_batch_device' % ('interp_' if interp else '',
                                                             'chi2' if chi2 else 'predict')
                    _lib.check(getattr(lib, name)(*head, *d_out))
                    results.append((ngal, second, d_out))
                _lib.check((lib.tc_interp_synchronize if interp else lib.tc_table_synchronize)(
                    device.handle))
                for ngal, second, d_out in results:
                    for array, ptr in zip((ngal, second), d_out):
                        _lib.check(lib.tc_memcpy_d2h(array.ctypes.data_as(ctypes.c_void_p), ptr,
                                                     array.nbytes))
        finally:
            for ptr in pointers:
                lib.tc_device_free(ptr)
        return [(ngal, second) for ngal, second, _ in results]

    def many(self, theta):
        """tc_predict_zheng07_many: (ngal, xi) of len(theta) walkers."""
        from tabcorr_amd import _lib
        device = self.halotab.to_device()
        theta = np.ascontiguousarray(theta)
        ngal, xi = np.empty(len(theta)), np.empty((len(theta), self.n_r))
        with device.lock:
            _lib.check(self.lib.tc_predict_zheng07_many(
                device.handle, _lib.as_double_p(theta), theta.shape[1], len(theta), 10, 0,
                _lib.as_double_p(ngal), _lib.as_double_p(xi)))
        return ngal, xi

    def call(self, case):
        """The case's call(s) on these handles: {name: float64 array}."""
        out = {}

        def keep(ngal, second, tag=''):
            if isinstance(ngal, dict):
                for key in ngal:
                    out['ngal_' + key + tag] = ngal[key]
                for key in second:
                    out['xi_' + key + tag] = second[key]
            else:
                out['ngal' + tag] = ngal
                out[('chi2' if case['chi2'] else 'xi') + tag] = second
        entry, chi2, separate = case['entry'], case['chi2'], case['separate']
        interp = self.interpolator is not None
        owner = self.interpolator if interp else self.halotab
        theta = theta_of(case)
        args = [theta] + ([x_of(case, self.points)] if interp else [])
        kwargs = {'extrapolate': True} if interp else {}
        with np.errstate(all='ignore'):
            if entry == 'many':
                keep(*self.many(theta))
            elif entry == 'pipelined':
                calls = [(theta_of(case, k), x_of(case, self.points, k) if interp else None)
                         for k in range(self.n_lanes() + 1)]
                for k, (ngal, xi) in enumerate(self.device_calls(calls, False, False)):
                    keep(ngal, xi, tag='_call%d' % k)
            elif entry == 'device':
                ngal, second = self.device_calls([(theta, args[-1])], chi2, separate)[0]
                if separate:
                    ngal, second = self.halotab._package(ngal, second, True)
                keep(ngal, second)
            elif chi2:
                method = owner.chi2_batch if entry == 'host' else owner.chi2_batch_async
                result = method(*args, *likelihood_of(self.n_r), **kwargs)
                keep(*(result if entry == 'host' else result.wait()))
            else:
                method = owner.predict_batch if entry == 'host' else owner.predict_batch_async
                result = method(*args, separate_gal_type=separate, **kwargs)
                keep(*(result if entry == 'host' else result.wait()))
        return {key: np.ascontiguousarray(value, dtype=np.float64).reshape(len(value), -1)
                for key, value in out.items()}


def run_case(case):
    """The case on fresh handles: {'launch': (workgroups, waves, slabs, LDS bytes), name: float64
    array (n_draws, values per draw)}."""
    target = Target(case['target'], case['options'])
    out = target.call(case)
    out['launch'] = target.last_launch()
    return out


def digest_of(array):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(array).tobytes()).digest(),
                         dtype=np.uint8)


def edges_of(array):
    """The first and last N_EDGE draws."""
    return np.concatenate([array[:N_EDGE], array[-N_EDGE:]])


def same_words(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def reference_of(case, key, base, own):
    """The words an array of a case is kept against (its stored form), or None: the base's array
    of that name; the base's only call for the first of consecutive calls; the first call's for
    the later ones.  `base`, `own`: the base's and the case's own arrays in stored form."""
    other = None
    if base is not None:
        other = base.get(key, base.get(key.replace('_call0', '')))
        if other is not None and is_digest(case) and len(other) != 2 * N_EDGE:
            other = np.concatenate([other[:N_EDGE], other[:N_EDGE]])
    if other is None and re.search('_call[1-9]', key):
        other = own[re.sub('_call[1-9]', '_call0', key)]
    return other


def stored_keys(result):
    """The arrays of a stored result in the order they are kept: a first call's before the
    later calls'."""
    return sorted((key for key in result if key != 'launch'),
                  key=lambda key: (bool(re.search('_call[1-9]', key)), key))


def pack(results, unrepeatable):
    """{case: {key: array}} -> the arrays of the file."""
    all_cases = dict(cases())
    arrays = {'launch': np.array([results[name]['launch'] for name in all_cases])}
    index = {'unrepeatable': sorted(unrepeatable), 'cases': {}}
    stored = {}
    for name, case in all_cases.items():
        stored[name] = stored_form(case, results[name])
        words, entries = [], []
        for key in stored_keys(stored[name]):
            value = stored[name][key]
            other = None if key.endswith('#') else reference_of(
                case, key, stored[case['base']] if case['base'] else None, stored[name])
            if other is not None and other.shape != value.shape:
                other = None
            kept = value.view(np.uint64)
            words.append((kept ^ other.view(np.uint64) if other is not None else kept).ravel())
            entries.append([key, list(value.shape), other is not None])
        arrays[name] = np.concatenate(words)
        index['cases'][name] = entries
    arrays['index'] = np.array(json.dumps(index))
    return arrays


def unpack(data):
    """The arrays of the file -> ({case: {key: array, key + '#': digest, 'launch': array}},
    unrepeatable names).  Of a large case the arrays are its first and last N_EDGE draws."""
    index = json.loads(str(data['index']))
    results = {}
    for number, (name, case) in enumerate(cases()):
        result, words, at = {}, data[name], 0
        for key, shape, against in index['cases'][name]:
            digest = key.endswith('#')
            count = 4 if digest else int(np.prod(shape))
            kept = words[at:at + count]
            at += count
            if against:
                other = reference_of(case, key, results[case['base']] if case['base'] else None,
                                     result)
                kept = kept ^ other.view(np.uint64).ravel()
            result[key] = kept.view(np.uint8) if digest else kept.view(np.float64).reshape(shape)
        result['launch'] = data['launch'][number]
        results[name] = result
    return results, set(index['unrepeatable'])


def stored_form(case, result):
    """A run's result as unpack() returns a recorded one."""
    out = {}
    for key, value in result.items():
        if key != 'launch' and is_digest(case):
            out[key + '#'] = digest_of(value)
            value = edges_of(value)
        out[key] = value
    return out


if __name__ == '__main__':
    sys.path.insert(0, REPO)
    results, unrepeatable = {}, set()
    for name, case in cases():
        results[name] = run_case(case)
        again = run_case(case)
        if not all(same_words(results[name][key], again[key]) for key in results[name]):
            unrepeatable.add(name)
        print(name, results[name]['launch'], 'UNREPEATABLE' if name in unrepeatable else '',
              flush=True)
    target = sys.argv[1] if len(sys.argv) > 1 else FILE
    np.savez_compressed(target, **pack(results, unrepeatable))
    recorded, listed = unpack(np.load(target))
    assert listed == unrepeatable
    for name, case in cases():
        for key, value in stored_form(case, results[name]).items():
            assert recorded[name][key].tobytes() == value.tobytes(), (name, key)
    print('%s: %d cases, %d unrepeatable %s, %d bytes' % (
        target, len(results), len(unrepeatable), sorted(unrepeatable), os.path.getsize(target)))
