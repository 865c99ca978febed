"""Comparison helper of the extent-matrix tests (tests/test_extent_matrix_gpu.py): an engine output against its oracle value.

Two criteria, both must hold:
  * real space -- the max-norm of the difference relative to the max magnitude of the oracle value (energies: relative to
    max(1, |E|));
  * per k-point -- max_k |V^_k - Vo^_k| / (|Vo^_k| + tau rms|Vo^|), the rms taken over k != 0.  A mix error confined to a few
    k-points of a grid of N points moves the real-space field by ~1/sqrt(N) of its size and passes the first criterion at
    any realistic N; this one sees it wherever the oracle's spectrum is not negligible.

Also the input recipe of the matrix (full-spectrum fields: every k-point carries a share of the rms spectral amplitude) and
the k-points where x-pass kernels go wrong (Nyquist planes, the folded half of the x axis, k off the 32-point tiling)."""
import numpy as np

from professad_amd import synth

# Tolerances of the matrix, per precision: about ten times the largest error measured on an MI355X over the whole matrix and
# the two full-size grids (both calls, every kernel family and GGA form), and never looser than the other GPU test files
# (fp64: E 1e-10, v 5e-10 of the max magnitude; fp32: 5e-6 / 5e-4).  Measured maxima:
#   fp64  E 1.5e-14, v 1.5e-13 (chi.grad 1.1e-13), mu 4.4e-15, per k-point 1.7e-10 (tau 1e-3; 256^3 closure)
#   fp32  E 4.3e-7,  v 1.5e-5  (chi.grad 6.5e-6),  mu 1.2e-7,  per k-point 4.2e-3 (tau 1; 512 x 256 x 128 closure)
# (the fp32 per-k bound is 2x its measured maximum: 10x would pass the single-k-point errors of 1e-2 that
# tests/test_spectral_check_cpu.py requires it to reject)
E_TOL = {'f64': 1e-13, 'f32': 4e-6}
V_TOL = {'f64': 1.5e-12, 'f32': 1e-4}
MU_TOL = {'f64': 4e-14, 'f32': 1e-6}
# per-k criterion: floor of the denominator (share of the rms spectral amplitude) and the bound on the ratio
TAU = {'f64': 1e-3, 'f32': 1.0}
K_TOL = {'f64': 1e-9, 'f32': 8e-3}
# The same bounds hold for the chirp-z matrix (tests/test_chirpz_matrix_gpu.py: extents without a line-transform plan; the fused
# chirp-z x pass, the three-pass form and the plain DFT kernels, and 255^3).  Measured maxima there:
#   fp64  E 7.6e-15, v 1.7e-13 (chi.grad 1.0e-13), mu 6.7e-16, per k-point 1.9e-10 (10 x 383 x 14 three-pass and fused)
#   fp32  E 7.9e-7,  v 2.4e-5  (chi.grad 1.3e-5),  mu 3.2e-7,  per k-point 4.5e-3 (255^3 potential)
# ... and for the slab-decomposed pipeline (tests/test_slab_matrix_gpu.py: 2, 4 and 8 emulated ranks, nine exchange geometries,
# every term set the slab path serves, both GGA forms, both entry points).  Measured maxima there:
#   fp64  E 9.0e-15, v 1.6e-13 (chi.grad 1.1e-13), mu 1.3e-15, per k-point 4.8e-11 (32 x 64 x 270 on 8 ranks, potential)
#   fp32  E 3.5e-7,  v 1.5e-5  (chi.grad 5.7e-6),  mu 1.5e-7,  per k-point 1.4e-3 (32 x 64 x 270 on 8 ranks, potential)
# and the largest difference between the slabs and one engine on the same inputs (relative; bounds 1e-12 and 5e-6 / 5e-4):
#   fp64  v 1.6e-13 (the Lindhard-factor sets, whose N_e sums in another order; 2.6e-16 for WGC99 + PBE), chi.grad 1.6e-14,
#         energies 4.0e-15, mu 1.4e-15
#   fp32  v 8.4e-7, chi.grad 6.4e-7, energies 5.7e-8, mu 1.4e-7


def spectrum(a):
    """orthonormal real-to-complex spectrum of a real grid (fp64)"""
    return np.fft.rfftn(np.asarray(a, dtype=np.float64), norm='ortho')


def rms_amplitude(ak):
    """rms of |a^_k| over k != 0 (the half spectrum of rfftn stands for the whole one)"""
    p = np.abs(ak) ** 2
    return float(np.sqrt((p.sum() - p[0, 0, 0]) / (p.size - 1)))


def realspace_error(v, vo):
    v, vo = np.asarray(v, dtype=np.float64), np.asarray(vo, dtype=np.float64)
    return float(np.max(np.abs(v - vo)) / (np.max(np.abs(vo)) + 1e-300))


def kspace_error(v, vo, tau, vok=None):
    """max_k |V^_k - Vo^_k| / (|Vo^_k| + tau rms|Vo^|); vok: spectrum(vo) if already at hand"""
    vok = spectrum(vo) if vok is None else vok
    d = np.abs(spectrum(v) - vok)
    return float(np.max(d / (np.abs(vok) + tau * rms_amplitude(vok))))


def errors(v, vo, p, vok=None):
    """(real-space error, per-k error) of v against vo at precision p ('f64' / 'f32')"""
    return realspace_error(v, vo), kspace_error(v, vo, TAU[p], vok)


def check(v, vo, p, what='', vok=None, E=None, Eo=None):
    """assert both criteria (and |E - Eo| <= E_TOL max(1, |Eo|) when energies are given); returns (err_v, err_k)"""
    ev, ek = errors(v, vo, p, vok)
    assert ev < V_TOL[p], ('real space', what, ev, V_TOL[p])
    assert ek < K_TOL[p], ('per k-point', what, ek, K_TOL[p])
    if E is not None:
        assert abs(E - Eo) <= E_TOL[p] * max(1.0, abs(Eo)), ('energy', what, E, Eo)
    return ev, ek


# ------------------------------------------------------------------------------------------------ inputs and probe points
def full_spectrum_inputs(shape, seed):
    """(den, vext, chi) of the matrix: synth.random_density (uniform white noise on a constant density), a random potential
    whose smooth part is weak next to its white noise, chi = sqrt(den) (1 + 0.1 U) -- every k-point carries part of every
    input.  White noise leaves ~1 % of the k-points below a tenth of the rms amplitude, so of the seeds seed, seed + 1000, ...
    the first one whose three fields carry >= 10 % of their rms amplitude at every probe point is used (at most a few tries;
    a generator without that weight -- a smooth or tiled field -- exhausts them and fails here)"""
    pts = list(probe_points(shape).values())
    for s in range(seed, seed + 8000, 1000):
        den = synth.random_density(shape, seed=s)
        vext = synth.random_potential(shape, seed=s + 1, amp=0.1)
        chi = np.sqrt(den) * (1.0 + 0.1 * np.random.default_rng(s + 2).random(shape))
        if all(min_probe_weight(a, pts) >= 0.1 for a in (den, vext, chi)):
            return den, vext, chi
    raise AssertionError('no full-spectrum input for %s from seed %d' % (shape, seed))


def min_probe_weight(a, pts):
    """smallest |a^_k| / rms|a^| over the k-points pts"""
    ak = spectrum(a)
    rms = rms_amplitude(ak)
    return min(abs(ak[k]) for k in pts) / rms


def probe_points(shape):
    """{name: (kx, ky, kz)} in rfftn index space (kz <= n2 / 2) of the k-points the sensitivity test perturbs"""
    n0, n1, n2 = shape
    h2 = n2 // 2

    def off32(n, want):        # an index near `want` that is not a multiple of 32 and not the Nyquist index
        k = want % n
        while k % 32 == 0 or (n % 2 == 0 and k == n // 2) or k == 0:
            k = (k + 1) % n
        return k
    return {
        'x_nyquist': (n0 // 2, off32(n1, 3), off32(h2, 5)),
        'x_folded_half': (n0 // 2 + 1, off32(n1, 7), off32(h2, 2)),
        'y_nyquist': (off32(n0, 9), n1 // 2, off32(h2, 3)),
        'z_nyquist_plane': (off32(n0, 11), off32(n1, 5), h2),
        'kz0_plane_kx_upper_half': (off32(n0, min(n0 // 2 + 5, n0 - 1)), off32(n1, 2), 0),
        'off_the_32_tiling': (off32(n0, 37), off32(n1, 13), off32(h2, 19)),
    }


def perturb(vo, k, rel, tau, vok=None):
    """vo + a single-k-point change of rel (|Vo^_k| + tau rms|Vo^|) -- a per-k error of exactly rel in the measure of the check
    with that tau -- as a real field: the Hermitian partner gets the matching change"""
    vok = spectrum(vo) if vok is None else vok
    amp = rel * (abs(vok[k]) + tau * rms_amplitude(vok))
    dk = np.zeros_like(vok)
    n0, n1, n2 = vo.shape
    self_partner = (k[0] * 2 % n0 == 0) and (k[1] * 2 % n1 == 0) and (k[2] == 0 or 2 * k[2] == n2)
    dk[k] = amp * (1.0 if self_partner else np.exp(0.7j))
    # a kz = 0 / Nyquist-plane point has its partner in the same plane of the half spectrum: put it there too, so that irfftn
    # (which symmetrises those planes) keeps the full change
    if k[2] == 0 or 2 * k[2] == n2:
        kp = ((-k[0]) % n0, (-k[1]) % n1, k[2])
        if kp != tuple(k):
            dk[kp] = np.conj(dk[k])
    return vo + np.fft.irfftn(dk, s=vo.shape, axes=(0, 1, 2), norm='ortho')
