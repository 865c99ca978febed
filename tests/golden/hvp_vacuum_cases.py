"""The vacuum-to-bulk case of the Hessian-vector goldens (make_golden_hvp_vacuum.py writes them, tests/test_hvp_vacuum_cpu.py and
tests/test_hvp_vacuum_gpu.py read them).  Every other density fed to a Hessian test lies in 0.02 .. 0.4 with small reduced gradients;
`v16s` is a slab: along z the density falls from 3.7e-2 to 1.6e-6 (about 1 500 points per decade), the reduced gradient s runs from
1e-2 to about 1e3 and r_s from 1.9 to 53 -- the range in which the second-order jets of PBE (n^(-8/3), n^(-7/3), r_s) and
n^(beta - 2) of WGC99 are largest.

The density floor of the second-order tests is 1e-6 (asserted below).  Under it the reference's `n^(7/3) + 1e-30` and the device's
`min(., 1e30)` guard differ by 1e-30 / n^(7/3): 1e-16 at n = 1e-6 but 5e-12 at n = 1e-8 -- a difference of guards, not of kernels.
Lower densities are out of scope.

The direction is weighted by sqrt(n / max n): that is what the chi-space product feeds the n-space one (dn ~ phi d), and an
unweighted direction makes the product 4 000 times larger in the vacuum decade than in the bulk, so that the transforms' rounding
of the vacuum sets the bulk's figures."""
import numpy as np

import hvp_cases
import hvp_wgc_cases

SHAPE = (16, 16, 32)
CASES = ['v16s']
DENSITY_FLOOR = 1e-6
HALF_INTEGER_MARGIN = hvp_wgc_cases.HALF_INTEGER_MARGIN
CFG3W = hvp_wgc_cases.CFG3W
# golden key -> engine term names.  The pair ('pbe_x', 'pbe_c') has no key: exchange and correlation cancel, and the numpy double was
# already 2.8e-12 from long double there, which leaves no room under the 1e-11 that counts as a finding.
KEYS = {'wgc99_nl': ('wgc99_nl',), 'pbe_x': ('pbe_x',), 'pbe_c': ('pbe_c',), 'cfg3w': CFG3W}
# The keys whose fields the GPU test compares.  pbe_x and pbe_c on their own are dropped: without a device the numpy double, its long
# double twin and the reference's golden already disagree by 0.9e-12 .. 5.1e-12 (pbe_x) and 1.4e-12 .. 1.7e-12 (pbe_c) of a decade's
# max|hv| (tests/test_hvp_vacuum_cpu.py), so ten times the yardstick would pass the 1e-11 that counts as a finding.  The cause is
# not the pointwise jets (1e-13 against long double on the sweep of that file) but their input: a transform rounds grad n to 1e-15 of
# its largest value, the bulk's, which is 1e-11 of the vacuum's own gradient, and sigma = |grad n|^2 enters f_ns dsigma and the flux at
# full weight there (f_ns dsigma alone is 1.4e-12 off).  Any transform-based product has this conditioning, the device's included.
# Their sums q_t stay compared (1.1e-14 and 1.8e-14 of sum|w hv_t| dV), and their fields inside cfg3w (6e-14 of its decade maxima).
GPU_KEYS = ('wgc99_nl', 'cfg3w')


def make_inputs(name='v16s'):
    """-> box, den, vext (numpy fp64)"""
    assert name == 'v16s'
    box = np.diag([8.0, 8.0, 16.0])
    rng = np.random.default_rng(5)
    z, x = np.arange(32) / 32, np.arange(16) / 16
    a, b = (np.log(0.03) + np.log(2e-6)) / 2, (np.log(0.03) - np.log(2e-6)) / 2
    den = (np.exp(a + b * np.cos(2 * np.pi * z))[None, None, :]
           * (1 + 0.2 * np.cos(2 * np.pi * x)[:, None, None] * np.sin(2 * np.pi * x)[None, :, None])
           * (1 + 0.05 * rng.random(SHAPE)))
    assert den.min() >= DENSITY_FLOOR, den.min()
    vext = -0.3 * np.cos(2 * np.pi * z)[None, None, :] * np.ones(SHAPE)          # (linear in n: no second derivative)
    return box, den, vext


def direction(den, seed=78):
    """the n-space direction: hvp_cases.direction weighted by sqrt(n / max n)"""
    return hvp_cases.direction(den.shape, seed=seed) * np.sqrt(den / den.max())


ZERO_AT = (3, 5, 7)          # (an odd flat index: the second lane of a pair)


def chi_inputs(box, den, zero=False):
    """-> phi = 1.7 sqrt(den) (with `zero`: exactly 0 at ZERO_AT, so n = 0 there), the unweighted direction d, a made-up gradient
    made perpendicular to phi, and N = sum den dV"""
    phi = 1.7 * np.sqrt(den)
    if zero:
        phi[ZERO_AT] = 0.0
    d = hvp_cases.direction(den.shape, seed=83)
    gr = hvp_cases.direction(den.shape, seed=84)
    gr -= phi * (phi * gr).sum() / (phi * phi).sum()
    return phi, d, gr, float(den.sum() * abs(np.linalg.det(box)) / den.size)


def decades(den):
    """floor(log10 den) per point, and the sorted list of the values that occur (a point where den = 0 counts with the lowest)"""
    dec = np.floor(np.log10(np.where(den > 0, den, den[den > 0].min()))).astype(int)
    return dec, sorted(set(dec.ravel().tolist()))
