"""The table-driven math of the occupation kernels as the DEVICE compiles it
(tc_debug_fastmath_device: the table staged in LDS, kinds 0 - 7 of tc_debug_fastmath, 8 the
reciprocal of the satellites' expansion, 9 exp2 with keep == false) within the bounds the host
tests state for the same functions (test_fastmath_accuracy_on_host,
test_central_moment_expansion_reproduces_the_node_loop, test_natural_log_accuracy_on_host,
test_half_erfc_from_the_gaussian_on_host), on their inputs cut to a few thousand plus the edges
where the device text differs from the host's: log2 takes mantissa, exponent and table row from
frexp_mant / frexp_exp / ubfe, the reciprocal is the hardware estimate with two Newton steps, and
a * b + c contracts.  Needs an MI355X.

Every test prints how many inputs give bits that differ from the host hook's; not asserted."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Inputs whose device bits differ from the host hook's, as measured on an MI355X with these
# inputs (kind: differing / all; largest difference):
#   0 erf, 4 erf of erf_gauss_fast, 5 its Gaussian   0 / 9159
#   1 log2   16 / 8364 (5.6e-17)         6 ln   13 / 8364 (5.6e-17)
#   2 exp2    0 / 10153                  3 exp10   0 / 3026
#   7 erfc(|x|) / 2   125 / 4510 (3.1e-33: the libm Gaussian beyond |x| = 6)
#   8 reciprocal against the host's 1.0 / x   287 / 8582 (one ulp)


def run(kind, x, device=True):
    from tabcorr_amd import _lib
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.full_like(x, np.nan)
    call = lib.tc_debug_fastmath_device if device else lib.tc_debug_fastmath
    _lib.check(call(kind, x.size, _lib.as_double_p(x), _lib.as_double_p(y)))
    return y


def both(kind, x):
    """Device values; prints how many differ in bits from the host hook's."""
    device = run(kind, x)
    host = run(kind, x, device=False)
    differ = int(np.sum(device.view(np.uint64) != host.view(np.uint64)))
    print('kind %d: %d of %d inputs differ in bits from the host hook, largest difference %.2e'
          % (kind, differ, len(device), float(np.max(np.abs(device - host)))))
    return device


def neighbours(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)])


def test_erf_on_the_device():
    from scipy import special
    rng = np.random.default_rng(5)
    centres = np.arange(0, 769) / 128.0
    ties = (np.arange(0, 768) + 0.5) / 128.0
    x = np.concatenate([rng.uniform(-7, 7, 3000), centres, -centres, neighbours(ties),
                        -neighbours(ties), neighbours([6.0, -6.0]),
                        [0.0, -0.0, 1e-300, 50.0, -50.0, 5.999, 30.0]])
    exact = special.erf(x)
    for kind, bound in ((0, 4e-16), (4, 4.5e-16)):
        got = both(kind, x)
        assert np.max(np.abs(got - exact)) < bound, kind
        assert np.array_equal(np.signbit(got), np.signbit(exact)), kind       # (+-0.0 too)
    # the derivative 2 / sqrt(pi) exp(-x^2), zero from the clamp of erf on
    got = both(5, x)
    gauss = (2 / np.sqrt(np.pi, dtype=np.longdouble) *
             np.exp(-x.astype(np.longdouble)**2)).astype(float)
    gauss[np.abs(x) >= 6.0] = 0.0
    np.testing.assert_allclose(got, gauss, rtol=1e-15)


def test_log2_on_the_device():
    rng = np.random.default_rng(5)
    rows = 1.0 + np.arange(257) / 256.0
    y = np.concatenate([10**rng.uniform(-290, 290, 2000), rng.uniform(0.5, 2.0, 2000),
                        2.0**np.arange(-1022, 1024), neighbours(rows)[neighbours(rows) >= 1.0],
                        neighbours(rows) * 2.0**-700, neighbours(rows) * 2.0**900,
                        [np.finfo(float).max, np.finfo(float).tiny, 1e-300, 1.0, 2.0, 0.5]])
    expect = np.log2(y.astype(np.longdouble))
    got = both(1, y)
    assert np.max(np.abs(got - expect) / np.maximum(1.0, np.abs(expect))) < 4e-16
    # the natural logarithm of the gradient kernels
    expect = np.log(y.astype(np.longdouble))
    got = both(6, y)
    assert np.max(np.abs(got - expect) / np.maximum(1.0, np.abs(expect))) < 4e-16


def test_exp2_and_exp10_on_the_device():
    rng = np.random.default_rng(5)
    steps = np.arange(-512, 513) / 256.0
    ties = (np.arange(-512, 512) + 0.5) / 256.0
    z = np.concatenate([rng.uniform(-900, 900, 3000), rng.uniform(-1, 1, 1000), steps,
                        neighbours(ties), steps + 700.0, steps - 700.0,
                        [1000.0, -1000.0, np.nextafter(1000.0, 0.0), np.nextafter(-1000.0, 0.0),
                         999.5, -999.5]])
    got = both(2, z)
    expect = np.exp2(z.astype(np.longdouble))
    assert np.max(np.abs(got / expect - 1.0)) < 4e-16
    # beyond +-1000 the argument is clamped
    beyond = np.array([np.nextafter(1000.0, np.inf), 1000.5, 1e300,
                       np.nextafter(-1000.0, -np.inf), -5000.0, -1e300])
    got = run(2, beyond)
    assert np.array_equal(got, run(2, np.where(beyond > 0, 1000.0, -1000.0)))
    assert np.all(got[3:] < 1e-300) and np.all(got[:3] > 1e300)
    # keep == false: exactly zero whatever the argument (the lanes with M <= M0)
    assert np.array_equal(run(9, z), np.zeros(len(z)))
    assert not np.any(np.signbit(run(9, z)))
    w = np.concatenate([rng.uniform(9.0, 16.0, 3000), np.arange(9, 17).astype(float),
                        neighbours(np.arange(10, 16).astype(float))])
    got = both(3, w)
    expect = np.power(np.longdouble(10), w.astype(np.longdouble))
    assert np.max(np.abs(got / expect - 1.0)) < 6e-16


def test_half_erfc_on_the_device():
    from scipy.special import erfc
    x = np.concatenate([np.linspace(2.5, 6.0, 2001), np.linspace(6.0, 26.0, 2001),
                        -np.linspace(2.5, 26.0, 501), neighbours([6.0]), [2.5, 6.0, 1e3, np.inf]])
    got = both(7, x)
    expect = 0.5 * erfc(np.abs(x))
    normal = expect > 1e-300
    assert np.max(np.abs(got[normal] / expect[normal] - 1.0)) < 1e-12
    assert np.all(got[~normal] <= 1e-300) and np.all(got >= 0.0)


def test_reciprocal_on_the_device():
    """The hardware estimate and two Newton steps r <- r + r (1 - x r), each an FMA pair: the
    last step adds a correction below an ulp to an r that is already within an ulp, so the
    result carries the error of one rounding of r + r (1 - x r) -- within an ulp of the exact
    quotient (a faithful rounding).  It is NOT always the correctly rounded 1.0 / x: 3 per cent
    of these inputs come out an ulp away (the residual 1 - x r is formed from the rounded r;
    Markstein's final correction step would be needed for that); quotients that are exact
    (powers of two) are exact."""
    rng = np.random.default_rng(7)
    powers = 2.0**np.arange(-1000, 1001, 8)
    near = powers
    for _ in range(4):
        near = np.unique(neighbours(near))
    x = np.concatenate([near, -near[::7], rng.uniform(0.5, 2.0, 3000),
                        10**rng.uniform(-280, 280, 2000), 10**rng.uniform(9, 16, 1000)])
    got = run(8, x)
    rounded = 1.0 / x
    exact = 1 / x.astype(np.longdouble)
    differ = int(np.sum(got != rounded))
    print('kind 8: %d of %d inputs differ in bits from 1.0 / x' % (differ, len(x)))
    spacing = np.spacing(np.abs(rounded)).astype(np.longdouble)
    assert np.all(np.abs(got.astype(np.longdouble) - exact) < spacing)
    assert np.array_equal(run(8, powers), 1.0 / powers)          # (exact quotients)
