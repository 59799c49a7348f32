"""What the entry sequences of the occupation seam (a table, a joint of tables, an interpolator)
and of the forward calls of the two joints refuse, in which order, and what they serve, at the C
level: every case is a refusal on the host or one launch of a single draw.  Needs an MI355X.

Every seam entry is the VJP or the chi2 gradient, on host arrays and on device pointers; every
forward entry predict or chi2 of a joint of tables and of a joint of interpolators, on both routes.
The tables are the smallest the synthetic fixtures build: 6 bins, a mode-auto table of 3 and a
mode-cross table of 2 correlation function bins, interpolators over 4 nodes of one axis (the fewest
an axis may have), joints of two.  The order pinned: the NULL handle, then flags, then a negative
count, then n_draws == 0 (served: nothing is read), then the NULL arrays.
"""

import ctypes

import numpy as np
import pytest

from tabcorr_amd import synthetic

pytestmark = pytest.mark.gpu

N_PRIM, N_SEC, GRID = 3, 1, (4, )
PARTS = [('auto', (3, )), ('cross', (2, ))]
SCALARS = {'n_draws': 1, 'flags': 0, 'n_theta': 5, 'n_gauss': 10}
HOST_ONLY = ('data', 'precision')            # host pointers in both twins of an entry
ROUTES = ['host', 'device']

# (kind, form) -> (symbol of the host-array entry, what follows the handle)
SEAM = {
    ('table', 'vjp'): ('tc_predict_occupation_vjp_batch',
                       'occupation n_draws flags g_ngal g_xi ngal xi g_occupation'),
    ('table', 'chi2_grad'): ('tc_chi2_occupation_grad_batch',
                        'occupation n_draws flags data precision ngal chi2 dchi2_docc'),
    ('joint', 'vjp'): ('tc_joint_predict_occupation_vjp_batch',
                       'occupation n_draws flags g_ngal g_xi ngal xi g_occupation'),
    ('joint', 'chi2_grad'): ('tc_joint_chi2_occupation_grad_batch',
                        'occupation n_draws flags data precision ngal chi2 dchi2_docc'),
    ('interp', 'vjp'): ('tc_interp_predict_occupation_vjp_batch',
                        'occupation x n_draws flags g_ngal g_xi ngal xi g_occupation g_x'),
    ('interp', 'chi2_grad'): ('tc_interp_chi2_occupation_grad_batch',
                         'occupation x n_draws flags data precision ngal chi2 dchi2_docc dchi2_dx '
                         'dngal_dx'),
}
FORWARD = {
    ('joint', 'predict'): ('tc_joint_predict_batch', 'theta n_theta n_draws n_gauss flags ngal xi'),
    ('joint', 'chi2'): ('tc_joint_chi2_batch',
                        'theta n_theta n_draws n_gauss flags data precision ngal chi2'),
    ('joint_interp', 'predict'): ('tc_joint_interp_predict_batch',
                                  'theta n_theta x n_draws n_gauss flags ngal xi'),
    ('joint_interp', 'chi2'): ('tc_joint_interp_chi2_batch',
                               'theta n_theta x n_draws n_gauss flags data precision ngal chi2'),
}
assert not set(SEAM) & set(FORWARD)
ENTRIES = {**SEAM, **FORWARD}
# The adjoint arrays of a seam entry: a table needs every one; those of a joint and of an
# interpolator go together, all NULL being the forward-only form.  (g_ngal may always be NULL.)
ADJOINT = {
    ('table', 'vjp'): ['g_xi', 'g_occupation'],
    ('table', 'chi2_grad'): ['dchi2_docc'],
    ('joint', 'vjp'): ['g_xi', 'g_occupation'],
    ('joint', 'chi2_grad'): ['dchi2_docc'],
    ('interp', 'vjp'): ['g_xi', 'g_occupation', 'g_x'],
    ('interp', 'chi2_grad'): ['dchi2_docc', 'dchi2_dx', 'dngal_dx'],
}
OUTPUTS = ('ngal', 'xi', 'chi2', 'g_occupation', 'dchi2_docc', 'g_x', 'dchi2_dx', 'dngal_dx')
SYNCHRONIZE = {'table': 'tc_table_synchronize', 'joint': 'tc_joint_synchronize',
               'interp': 'tc_interp_synchronize', 'joint_interp': 'tc_joint_interp_synchronize'}
# The flags a seam entry refuses, and how: (status name, word of the message).
SEAM_FLAG_STATUS = {'table': 'TC_ERR_UNSUPPORTED', 'interp': 'TC_ERR_UNSUPPORTED',
                    'joint': 'TC_ERR_INVALID'}
FORWARD_NOUN = {'joint': 'joint forward calls', 'joint_interp': 'joint interpolator forward calls'}


def tokens(key):
    return ENTRIES[key][1].split()


def required(key):
    """The arrays of an entry that must be there: all but g_ngal and the adjoint ones."""
    return [name for name in tokens(key)
            if name not in SCALARS and name != 'g_ngal' and name not in ADJOINT.get(key, ())]


class Kind:
    """A handle of one kind with valid arrays of one draw for all of its entries, on the host
    and (but for data and precision) on the device."""

    def __init__(self, kind, owner, n_bins, n_r, x):
        from tabcorr_amd import _lib
        self.kind, self.owner, self.device = kind, owner, owner.to_device()
        self.lib = self.device.lib
        occupation = np.full((1, n_bins), 0.5)
        self.host = {
            'theta': synthetic.zheng07_draws(1, seed=1), 'x': x, 'occupation': occupation,
            'g_ngal': np.ones(1), 'g_xi': np.ones((1, n_r)), 'data': np.ones(n_r),
            'precision': np.eye(n_r), 'ngal': np.zeros(1), 'xi': np.zeros((1, n_r)),
            'chi2': np.zeros(1), 'g_occupation': np.zeros_like(occupation),
            'dchi2_docc': np.zeros_like(occupation), 'g_x': np.zeros_like(x),
            'dchi2_dx': np.zeros_like(x), 'dngal_dx': np.zeros_like(x)}
        self.host = {name: np.ascontiguousarray(a, dtype=np.float64)
                     for name, a in self.host.items()}
        self.on_device = {}
        for name, array in self.host.items():
            if name in HOST_ONLY:
                continue
            ptr = ctypes.c_void_p()
            _lib.check(self.lib.tc_device_malloc(ctypes.byref(ptr), array.nbytes))
            _lib.check(self.lib.tc_memcpy_h2d(ptr, array.ctypes.data_as(ctypes.c_void_p),
                                              array.nbytes))
            self.on_device[name] = ptr

    def release(self):
        for ptr in self.on_device.values():
            self.lib.tc_device_free(ptr)

    def call(self, form, route, null=(), handle=True, **scalars):
        """The status of the entry; null: the arrays passed as NULL ('all': every one)."""
        from tabcorr_amd import _lib
        key = (self.kind, form)
        values = dict(SCALARS, **scalars)
        passed = []
        for name in tokens(key):
            if name in values:
                passed.append(values[name])
            elif null == 'all' or name in null:
                passed.append(None)
            elif route == 'host' or name in HOST_ONLY:
                passed.append(_lib.as_double_p(self.host[name]))
            else:
                passed.append(self.on_device[name])
        entry = getattr(self.lib, ENTRIES[key][0] + ('_device' if route == 'device' else ''))
        with self.device.lock:
            return entry(self.device.handle if handle else None, *passed)

    def results(self, form, route, null=()):
        """The outputs of a served call, by name."""
        from tabcorr_amd import _lib
        assert self.call(form, route, null) == _lib.TC_OK
        names = [name for name in tokens((self.kind, form)) if name in OUTPUTS and name not in null]
        if route == 'host':
            return {name: self.host[name].copy() for name in names}
        out = {}
        with self.device.lock:
            _lib.check(getattr(self.lib, SYNCHRONIZE[self.kind])(self.device.handle))
            for name in names:
                out[name] = np.empty_like(self.host[name])
                _lib.check(self.lib.tc_memcpy_d2h(out[name].ctypes.data_as(ctypes.c_void_p),
                                                  self.on_device[name], out[name].nbytes))
        return out


@pytest.fixture(scope='module')
def kinds():
    from tabcorr_amd import Interpolator, JointInterpolator, JointLikelihood, TabCorr, _lib
    _lib.require_device()

    def halotab(table):
        return TabCorr.from_arrays(table['gal_type'], table['tpcf_matrix'], table['tpcf_shape'],
                                   table['attrs'])

    tables = [synthetic.synthetic_table(N_PRIM, N_SEC, shape, mode, seed=3)
              for mode, shape in PARTS]
    halotabs = [halotab(table) for table in tables]
    interpolators = []
    for mode, shape in PARTS:
        nodes, keys, points = synthetic.synthetic_interpolator(GRID, N_PRIM, N_SEC, shape, mode,
                                                               seed=40)
        interpolators.append(Interpolator([halotab(table) for table in nodes],
                                          {key: points[:, d] for d, key in enumerate(keys)}))
    n_bins = len(tables[0]['gal_type'])
    x = np.mean(points, axis=0, keepdims=True)
    none = np.zeros((1, 1))
    out = {'table': Kind('table', halotabs[0], n_bins, 3, none),
           'joint': Kind('joint', JointLikelihood(halotabs), n_bins, 5, none),
           'interp': Kind('interp', interpolators[0], n_bins, 3, x),
           'joint_interp': Kind('joint_interp', JointInterpolator(interpolators), n_bins, 5, x)}
    # (an interpolator's occupations have one row per class: its tables share their gal_type)
    n_classes = ctypes.c_int()
    _lib.check(out['interp'].lib.tc_interp_info(out['interp'].device.handle, None,
                                                ctypes.byref(n_classes), None, None))
    assert n_classes.value == 1
    yield out
    for kind in out.values():
        kind.release()


def refused(kind, status, expect, *words):
    """`status` is the code named `expect` and the message has every one of `words`."""
    from tabcorr_amd import _lib
    assert status == getattr(_lib, expect), (status, expect)
    message = kind.lib.tc_last_error().decode(errors='replace')
    for word in words:
        assert word in message, (word, message)


SEAM_CASES = [key + (route, ) for key in SEAM for route in ROUTES]
FORWARD_CASES = [key + (route, ) for key in FORWARD for route in ROUTES]


@pytest.mark.parametrize('kind,form,route', SEAM_CASES + FORWARD_CASES)
def test_a_required_array_that_is_null_is_invalid(kinds, kind, form, route):
    for name in required((kind, form)):
        refused(kinds[kind], kinds[kind].call(form, route, null=(name, )), 'TC_ERR_INVALID',
                'NULL')


@pytest.mark.parametrize('kind,form,route', SEAM_CASES)
def test_the_adjoint_arrays_go_together(kinds, kind, form, route):
    """A table has no forward-only form; a joint's and an interpolator's adjoint arrays are all
    there or all NULL, and the refusal of a mixed set names them."""
    from tabcorr_amd import _lib
    group = ADJOINT[kind, form]
    subsets = [tuple(name for k, name in enumerate(group) if mask >> k & 1)
               for mask in range(1, 2 ** len(group) - 1)]
    if kind == 'table':
        for null in subsets + [tuple(group)]:
            refused(kinds[kind], kinds[kind].call(form, route, null=null), 'TC_ERR_INVALID',
                    'NULL pointer')
        return
    for null in subsets:
        refused(kinds[kind], kinds[kind].call(form, route, null=null), 'TC_ERR_INVALID',
                'go together', *group)
    assert kinds[kind].call(form, route, null=tuple(group)) == _lib.TC_OK
    assert kinds[kind].call(form, route, null=tuple(group) + ('g_ngal', )) == _lib.TC_OK


@pytest.mark.parametrize('kind,form,route', SEAM_CASES + FORWARD_CASES)
def test_no_draws_and_a_negative_count(kinds, kind, form, route):
    """n_draws == 0 is served with every array NULL -- nothing is read --, but not on a NULL handle;
    a negative count is invalid."""
    from tabcorr_amd import _lib
    one = kinds[kind]
    assert one.call(form, route, null='all', n_draws=0) == _lib.TC_OK
    assert one.call(form, route, n_draws=0) == _lib.TC_OK
    refused(one, one.call(form, route, null='all', n_draws=0, handle=False), 'TC_ERR_INVALID',
            'joint handle is NULL' if kind.startswith('joint') else 'handle is NULL')
    refused(one, one.call(form, route, n_draws=-1), 'TC_ERR_INVALID', 'n_draws')


@pytest.mark.parametrize('kind,form,route', SEAM_CASES)
def test_a_seam_entry_refuses_flags_first(kinds, kind, form, route):
    """A flag is refused with its own status and words whatever else is wrong with the call: a
    NULL array, every array NULL, no draws, a negative count."""
    from tabcorr_amd import _lib
    one = kinds[kind]
    for flags in (_lib.FLAG_ASSEMBIAS, _lib.FLAG_LEAUTHAUD11, 32):
        for wrong in ({}, {'null': ('occupation', )}, {'null': 'all'},
                      {'null': 'all', 'n_draws': 0}, {'n_draws': -1}):
            refused(one, one.call(form, route, flags=flags, **wrong), SEAM_FLAG_STATUS[kind],
                    'flags')
    # (and the NULL handle before the flags)
    refused(one, one.call(form, route, flags=_lib.FLAG_ASSEMBIAS, handle=False), 'TC_ERR_INVALID',
            'handle is NULL')


@pytest.mark.parametrize('kind,form,route', FORWARD_CASES)
def test_a_joint_forward_entry_refuses_flags_first(kinds, kind, form, route):
    from tabcorr_amd import _lib
    one = kinds[kind]
    for flags, words in ((_lib.FLAG_SEPARATE_GAL_TYPE, 'separate_gal_type'),
                         (_lib.FLAG_LEAUTHAUD11, 'Zheng07 family'),
                         (32, 'unknown flags 0x20')):
        for wrong in ({}, {'null': ('theta', )}, {'null': 'all'}, {'null': 'all', 'n_draws': 0},
                      {'n_draws': -1}, {'n_theta': 4}):
            refused(one, one.call(form, route, flags=flags, **wrong), 'TC_ERR_UNSUPPORTED',
                    FORWARD_NOUN[kind], words)
    refused(one, one.call(form, route, flags=32, handle=False), 'TC_ERR_INVALID',
            'joint handle is NULL')
    # (the family's flag is served, with its seven columns)
    refused(one, one.call(form, route, flags=_lib.FLAG_ASSEMBIAS), 'TC_ERR_INVALID', '7 columns')


@pytest.mark.parametrize('kind,form', list(SEAM) + list(FORWARD))
def test_a_served_draw_has_the_same_bits_on_both_routes(kinds, kind, form):
    """After all the refusals above, or before them: one draw, complete and (a joint, an
    interpolator) forward-only."""
    one = kinds[kind]
    forms = [()] if kind == 'table' or (kind, form) in FORWARD else [(), tuple(ADJOINT[kind, form])]
    for null in forms:
        host, device = one.results(form, 'host', null), one.results(form, 'device', null)
        assert list(host) == list(device) and len(host) == (2 if null else len(host))
        for name in host:
            assert np.all(np.isfinite(host[name])), (name, host[name])
            assert np.array_equal(host[name], device[name]), (name, host[name], device[name])
        assert host['ngal'][0] > 0.0
