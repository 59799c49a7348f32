"""Records what every derivative entry point returns -- tables, interpolators and joints of tables;
the host-array and the _device symbols; Zheng07, its assembly-bias decoration and Leauthaud11;
prediction, likelihood and likelihood with Fisher matrix; the occupation VJP -- on an MI355X, into
grad_paths_parent.npz:
python tests/golden/make_grad_paths_parent.py

Run it with the library of the commit whose bits are the reference (the parent of the change that
gives the derivative calls one request struct, one staging path and one entry);
tests/test_gpu_grad_paths.py then asks every later library for the same bits.  `cases()` and
`run_case()` are what that test evaluates too.

The file holds, per case, the (workgroups, waves, slabs, LDS bytes) of the last launch and the
results as float64 words, one vector per case (`index` names the arrays in it).  A case whose
`base` runs the same handle kind and draws through another entry point or form is kept as the
exclusive-or with the base's words of the arrays they share; a joint's prediction is kept against
its `parts`, the tables' own predictions side by side.  A case of 4096 draws or more is kept
as the SHA-256 of its result bytes (`key#`), the words of its first 64 draws (`key`) and those of
its last 64 (`key$`): they are the same draws, so the last are kept against the first.  Every
case is run twice on fresh handles; one whose words do not repeat is listed under `unrepeatable`,
and the test compares it with the reference only.
"""

import ctypes
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
FILE = os.path.join(HERE, 'grad_paths_parent.npz')
for _path in (HERE, TESTS, REPO):
    if _path not in sys.path:
        sys.path.insert(0, _path)

from make_call_paths_parent import (  # noqa: E402
    GRID, TABLES, digest_of, likelihood_of, same_words, tables_of)

N_DRAWS = 35                    # two workgroups of 16 draws and a partial one of 3
MAX_SLAB = 1 << 18              # (csrc/internal.h: kMaxSlab; what max_slab() gives tables of few bins)
N_SLABS = MAX_SLAB + 17         # a second slab of 17 draws: a whole workgroup and one draw
N_LARGE = 4096                  # from here on a case is kept as a digest and its edges
N_EDGE = 64                     # draws kept of either end of such a case
N_GAUSS = 10

# the slab cases: (n_prim, n_sec, n_r) = (3, 2, 2) keeps 2^18 + 17 draws' results at a few tens of MB
NARROW = {'narrow_auto': ((3, 2, 2), 'auto'), 'narrow_cross': ((3, 2, 2), 'cross')}
N_PARAMS = {'zheng07': 5, 'assembias': 7, 'leauthaud11': 11}
FAMILIES = {'table': ('zheng07', 'assembias', 'leauthaud11'), 'interp': ('zheng07', 'assembias'),
            'joint': ('zheng07', 'assembias')}
FORMS = ('predict', 'chi2', 'fisher')       # prediction, likelihood, likelihood with Fisher matrix
TARGETS = {'table': ('auto19', 'cross19'), 'interp': ('interp_auto', 'interp_cross'),
           'joint': ('joint', )}


def kind_of(target):
    return 'interp' if target.startswith('interp') else \
        'joint' if target.startswith('joint') else 'table'


def cases():
    """(name, dict) of every recorded case, a case's base before it."""
    out = []

    def add(name, target, **case):
        case.update(target=target)
        for key, value in (('family', 'zheng07'), ('form', 'predict'), ('entry', 'host'),
                           ('modulate', False), ('symmetric', True), ('n_draws', N_DRAWS),
                           ('vjp', False), ('base', None), ('parts', None)):
            case.setdefault(key, value)
        out.append((name, case))
    # every derivative entry of the three handle kinds, host arrays and device pointers
    for kind in ('table', 'interp', 'joint'):
        for target in TARGETS[kind]:
            for family in FAMILIES[kind]:
                for form in FORMS:
                    host = '%s_%s_%s_host' % (target, family, form)
                    add(host, target, family=family, form=form,
                        base='%s_%s_chi2_host' % (target, family) if form == 'fisher' else None,
                        parts=['%s_%s_predict_host' % (table, family)
                               for table in TARGETS['table']]
                        if kind == 'joint' and form == 'predict' else None)
                    add(host[:-4] + 'device', target, family=family, form=form, entry='device',
                        base=host)
    # TC_FLAG_MODULATE_WITH_CENOCC and a non-symmetric precision matrix, once per handle kind
    add('auto19_zheng07_fisher_host_modulate', 'auto19', form='fisher', modulate=True)
    add('interp_cross_zheng07_fisher_host_modulate', 'interp_cross', form='fisher', modulate=True)
    add('joint_assembias_fisher_host_modulate', 'joint', family='assembias', form='fisher',
        modulate=True)
    for target in ('auto19', 'interp_auto', 'joint'):
        add(target + '_zheng07_fisher_host_nonsymmetric', target, form='fisher', symmetric=False)
    # the four occupation-VJP entries
    for target in TARGETS['table']:
        for form in ('predict', 'chi2'):
            host = '%s_vjp_%s_host' % (target, form)
            add(host, target, form=form, vjp=True)
            add(host[:-4] + 'device', target, form=form, vjp=True, entry='device', base=host)
    # more than one slab
    for target in NARROW:
        for form in ('predict', 'chi2'):
            host = '%s_slabs_%s_host' % (target, form)
            add(host, target, form=form, n_draws=N_SLABS)
            add(host[:-4] + 'device', target, form=form, entry='device', n_draws=N_SLABS,
                base=host)
    add('narrow_auto_slabs_leauthaud11_fisher_host', 'narrow_auto', family='leauthaud11',
        form='fisher', n_draws=N_SLABS)
    add('interp_narrow_slabs_predict_host', 'interp_narrow', n_draws=N_SLABS)
    add('joint_narrow_slabs_fisher_host', 'joint_narrow', form='fisher', n_draws=N_SLABS)
    add('narrow_cross_slabs_vjp_predict_host', 'narrow_cross', vjp=True, n_draws=N_SLABS)
    return out


def is_digest(case):
    return case['n_draws'] >= N_LARGE


def tables_for(target):
    """The table dicts behind a target, with (keys, points) for an interpolator."""
    from tabcorr_amd import synthetic

    def narrow(name):
        (n_prim, n_sec, n_r), mode = NARROW[name]
        return synthetic.synthetic_table(n_prim, n_sec, (n_r, ), mode, seed=n_prim + n_r)
    if target in NARROW:
        return [narrow(target)], None, None
    if target == 'interp_narrow':
        return synthetic.synthetic_interpolator(GRID, 3, 2, (2, ), 'auto', seed=3)
    if target == 'joint':
        return [tables_of('auto19')[0][0], tables_of('cross19')[0][0]], None, None
    if target == 'joint_narrow':
        return [narrow('narrow_auto'), narrow('narrow_cross')], None, None
    return tables_of(target)


def n_r_of(target):
    """The rows of a draw's result: the sum of the tables' of a joint."""
    tables, _, _ = tables_for(target)
    if kind_of(target) == 'joint':
        return sum(len(table['tpcf_matrix']) for table in tables)
    return len(tables[0]['tpcf_matrix'])


def rows_of(case):
    """Which of the N_DRAWS base draws each draw of the case is: a large case repeats them in
    turn, and its last N_EDGE draws are its first."""
    rows = np.arange(case['n_draws']) % N_DRAWS
    if is_digest(case):
        rows[-N_EDGE:] = rows[:N_EDGE]
    return rows


@functools.lru_cache(maxsize=None)
def base_draws(target, family):
    """The N_DRAWS draws of a target and family: the stress draws of the family's own suite
    (seed 5), logM0 clear of every table's nodes."""
    import assembias_grad_reference
    import grad_reference
    import leauthaud11_grad_reference
    tables, _, _ = tables_for(target)
    if family == 'leauthaud11':
        return leauthaud11_grad_reference.stress_draws(N_DRAWS, seed=5)
    module = assembias_grad_reference if family == 'assembias' else grad_reference
    theta = module.stress_draws(tables[0], N_DRAWS, seed=5, n_gauss_prim=N_GAUSS)
    nodes = np.unique(np.concatenate([grad_reference.nodes_of(t, N_GAUSS) for t in tables]))
    grad_reference.centre_log_m0(theta, nodes)
    return np.ascontiguousarray(theta)


@functools.lru_cache(maxsize=None)
def base_x(target):
    """The N_DRAWS coordinates on an interpolator's axis: uniform over the grid, draws 0 and 1
    beyond either end by 10 %, draw 3 on the right edge, draw 4 on the left."""
    points = tables_for(target)[2]
    a = np.unique(points[:, 0])
    x = np.random.default_rng(N_DRAWS).uniform(a[0], a[-1], (N_DRAWS, 1))
    x[0], x[1] = a[0] - 0.1 * (a[-1] - a[0]), a[-1] + 0.1 * (a[-1] - a[0])
    x[3], x[4] = a[-1], a[0]
    return x


@functools.lru_cache(maxsize=None)
def base_occupations(target):
    """The N_DRAWS occupation arrays of the VJP cases: the oracle's of the Zheng07 draws."""
    from oracle import tabcorr_oracle as oracle
    table = tables_for(target)[0][0]
    return np.array([oracle.mean_occupation(table, oracle.Zheng07(t), N_GAUSS)
                     for t in base_draws(target, 'zheng07')])


@functools.lru_cache(maxsize=None)
def base_cotangents(target):
    """g_xi (N_DRAWS, n_r) and g_ngal (N_DRAWS) of the VJP cases."""
    rng = np.random.default_rng(17)
    return rng.normal(size=(N_DRAWS, n_r_of(target))), rng.normal(size=N_DRAWS)


def operands_of(n_r, symmetric=True):
    """Data vector and precision matrix of the likelihood cases (fixed numbers, no device):
    symmetric positive semi-definite, or other data and a non-symmetric part on top."""
    vector, precision = likelihood_of(n_r)
    if symmetric:
        return np.ascontiguousarray(vector), np.ascontiguousarray(precision)
    rng = np.random.default_rng(100 + n_r)
    return (np.ascontiguousarray(vector * (1.0 + 0.1 * rng.normal(size=n_r))),
            np.ascontiguousarray(precision + rng.normal(size=(n_r, n_r)) / np.mean(vector)**2))


class TrailingNull:
    """derivative_kit.device_call's view of a handle whose entry `name` is given NULL for the
    trailing `fisher` behind the outputs that device_call allocates."""

    def __init__(self, device, name):
        self.lock, self.handle, self.lib = device.lock, device.handle, self
        self.library, self.name = device.lib, name

    def __getattr__(self, name):
        if name == 'with_trailing_null':
            entry = getattr(self.library, self.name)
            return lambda handle, *passed: entry(handle, *passed, None)
        return getattr(self.library, name)


class Target:
    """Fresh handles of a target: a table, an interpolator over `halotabs` or their joint."""

    def __init__(self, target):
        from tabcorr_amd import Interpolator, JointLikelihood, TabCorr, _lib
        self.lib = _lib.load()
        self.target, self.kind = target, kind_of(target)
        tables, keys, self.points = tables_for(target)
        self.halotabs = [TabCorr.from_arrays(t['gal_type'], t['tpcf_matrix'], t['tpcf_shape'],
                                             t['attrs']) for t in tables]
        self.owner = self.halotabs[0]
        if self.kind == 'interp':
            self.owner = Interpolator(self.halotabs, {keys[0]: self.points[:, 0]})
        elif self.kind == 'joint':
            self.owner = JointLikelihood(self.halotabs)
        self.owner.to_device()
        self.n_r = n_r_of(target)

    def last_launch(self):
        from tabcorr_amd import _lib
        launch = [ctypes.c_int() for _ in range(4)]
        _lib.check(self.lib.tc_table_last_launch(self.halotabs[0].to_device().handle,
                                                 *[ctypes.byref(v) for v in launch]))
        return np.array([v.value for v in launch], dtype=np.int64)

    def flat(self, value, leading):
        """A result of the Python layer in the C layout: a joint's per-table list on one axis."""
        if isinstance(value, list):
            value = np.concatenate([np.reshape(part, leading + (-1, )) for part in value], axis=-1)
        return value

    def host(self, case, theta, x, data, precision):
        """The case through the Python methods: the host-array symbols."""
        family, form = case['family'], case['form']
        kwargs = {'modulate_with_cenocc': case['modulate']}
        if self.kind == 'table':
            kwargs.update(assembias=family == 'assembias',
                          family='leauthaud11' if family == 'leauthaud11' else 'zheng07')
        else:
            kwargs.update(assembias=family == 'assembias')
        args = [theta]
        if self.kind == 'interp':
            args.append(x)
            kwargs.update(extrapolate=True)
        if form == 'predict':
            got = self.owner.predict_batch_grad(*args, **kwargs)
            n, q = len(theta), got[2].shape[1]
            return got[0], self.flat(got[1], (n, )), got[2], self.flat(got[3], (n, q))
        method = self.owner.chi2_grad_batch if form == 'chi2' else self.owner.chi2_fisher_batch
        return method(*args, data, precision, **kwargs)

    def device(self, case, theta, x, data, precision):
        """The case through the _device symbol on freshly allocated device arrays."""
        from derivative_kit import device_call
        from tabcorr_amd import _lib
        family, form = case['family'], case['form']
        device = self.owner.to_device()
        n, n_r = len(theta), self.n_r
        q = theta.shape[1] if family != 'leauthaud11' else N_PARAMS[family]
        flags = _lib.FLAG_MODULATE_WITH_CENOCC if case['modulate'] else 0
        prefix = {'table': 'tc_', 'interp': 'tc_interp_', 'joint': 'tc_joint_'}[self.kind]
        arguments = [theta, theta.shape[1]]
        if self.kind == 'interp':
            arguments.append(x)
            q += x.shape[1]
        if self.kind == 'joint':
            flags |= _lib.FLAG_ASSEMBIAS if family == 'assembias' else 0
            stem, optional_fisher = '', True
        else:
            stem, optional_fisher = '_' + family, family != 'zheng07'
        arguments += [n, N_GAUSS, flags]
        sync = {'table': 'tc_table_synchronize', 'interp': 'tc_interp_synchronize',
                'joint': 'tc_joint_synchronize'}[self.kind]
        if form == 'predict':
            return device_call(device, prefix + 'predict_grad%s_batch_device' % stem, arguments,
                               [n, (n, n_r), (n, q), (n, q, n_r)], sync)
        arguments += [_lib.as_double_p(data), _lib.as_double_p(precision)]
        shapes = [n, n, (n, q), (n, q)]
        if form == 'fisher':
            name = 'chi2_grad' if optional_fisher else 'chi2_fisher'
            return device_call(device, prefix + '%s%s_batch_device' % (name, stem), arguments,
                               shapes + [(n, q, q)], sync)
        name = prefix + 'chi2_grad%s_batch_device' % stem
        if optional_fisher:
            return device_call(TrailingNull(device, name), 'with_trailing_null', arguments,
                               shapes, sync)
        return device_call(device, name, arguments, shapes, sync)

    def vjp(self, case, rows, data, precision):
        from derivative_kit import device_call
        from tabcorr_amd import _lib
        occupation = np.ascontiguousarray(base_occupations(self.target)[rows])
        g_xi, g_ngal = (np.ascontiguousarray(a[rows]) for a in base_cotangents(self.target))
        n = len(occupation)
        if case['entry'] == 'host':
            if case['form'] == 'chi2':
                return self.owner.chi2_grad_occupation(occupation, data, precision)
            return self.owner.predict_vjp(occupation, g_xi, g_ngal)
        device = self.owner.to_device()
        if case['form'] == 'chi2':
            return device_call(device, 'tc_chi2_occupation_grad_batch_device',
                               [occupation, n, 0, _lib.as_double_p(data),
                                _lib.as_double_p(precision)], [n, n, occupation.shape])
        return device_call(device, 'tc_predict_occupation_vjp_batch_device',
                           [occupation, n, 0, g_ngal, g_xi], [n, (n, self.n_r), occupation.shape])

    def call(self, case):
        """The case's call on these handles: {name: float64 array (n_draws, values per draw)}."""
        rows = rows_of(case)
        data, precision = operands_of(self.n_r, case['symmetric'])
        with np.errstate(all='ignore'):
            if case['vjp']:
                got = self.vjp(case, rows, data, precision)
                names = ('ngal', 'chi2', 'dchi2_docc') if case['form'] == 'chi2' else \
                    ('ngal', 'xi', 'g_occupation')
            else:
                theta = np.ascontiguousarray(base_draws(self.target, case['family'])[rows])
                x = np.ascontiguousarray(base_x(self.target)[rows]) \
                    if self.kind == 'interp' else None
                got = (self.host if case['entry'] == 'host' else self.device)(
                    case, theta, x, data, precision)
                names = ('ngal', 'xi', 'dngal', 'dxi') if case['form'] == 'predict' else \
                    ('ngal', 'chi2', 'dngal', 'dchi2', 'fisher')
        return {key: np.ascontiguousarray(value, dtype=np.float64).reshape(len(value), -1)
                for key, value in zip(names, got)}


def run_case(case, target=None):
    """The case on fresh handles (or on `target`): {'launch': (workgroups, waves, slabs, LDS
    bytes), name: float64 array}."""
    target = Target(case['target']) if target is None else target
    out = target.call(case)
    out['launch'] = target.last_launch()
    return out


def stored_form(case, result):
    """A run's result as unpack() returns a recorded one."""
    out = {}
    for key, value in result.items():
        if key != 'launch' and is_digest(case):
            out[key + '#'] = digest_of(value)
            out[key + '$'] = value[-N_EDGE:]
            value = value[:N_EDGE]
        out[key] = value
    return out


def stored_keys(result):
    """The arrays of a stored result in the order they are kept: `key` before `key$`."""
    return sorted((key for key in result if key != 'launch'),
                  key=lambda key: (key.endswith('$'), key))


def reference_of(key, shape, base, own):
    """The words an array is kept against, or None: the base's array of that name and shape,
    else the first draws for the last ones of a large case.  `base`, `own`: the base's and the
    case's own arrays in stored form."""
    if key.endswith('#'):
        return None
    if base is not None and key in base and base[key].shape == tuple(shape):
        return base[key]
    if key.endswith('$'):
        return own[key[:-1]]
    return None


def base_of(case, stored):
    """The stored arrays a case is kept against, or None: its base's, or those of its `parts`
    side by side as a joint of them returns them."""
    if case['parts']:
        parts = [stored[name] for name in case['parts']]
        n, q = parts[0]['dngal'].shape
        return {'ngal': parts[0]['ngal'], 'dngal': parts[0]['dngal'],
                'xi': np.concatenate([part['xi'] for part in parts], axis=1),
                'dxi': np.concatenate([part['dxi'].reshape(n, q, -1) for part in parts],
                                      axis=2).reshape(n, -1)}
    return stored[case['base']] if case['base'] else None


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
            other = reference_of(key, value.shape, base_of(case, stored), stored[name])
            kept = value.view(np.uint64)
            words.append((kept ^ other.view(np.uint64) if other is not None else kept).ravel())
            entries.append([key, list(value.shape), other is not None])
        arrays[name] = np.concatenate(words)
        index['cases'][name] = entries
    arrays['index'] = np.array(json.dumps(index))
    return arrays


def unpack(data):
    """The arrays of the file -> ({case: {key: array, key + '#': digest, 'launch': array}},
    unrepeatable names).  Of a large case `key` and `key$` are its first and last N_EDGE draws."""
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
                other = reference_of(key, shape, base_of(case, results), result)
                kept = kept ^ other.view(np.uint64).ravel()
            result[key] = kept.view(np.uint8) if digest else kept.view(np.float64).reshape(shape)
        result['launch'] = data['launch'][number]
        results[name] = result
    return results, set(index['unrepeatable'])


if __name__ == '__main__':
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
