"""Ionic (external) potential from ion positions -- the step right before the energy path.

`read_recpot` restates the reference's recpot parsing (src/professad/ion_utils.py:20-81: units, ion charge from the
first two table entries, Coulomb tail added for interpolation); `ionic_potential` builds v_ext on the GPU through
`ofdft_ionic_potential` (exact or particle-mesh-Ewald structure factor), species by species like
System.__potential_from_ions (src/professad/system.py:183-194).
"""
import ctypes as C
import math

import numpy as np
import torch

# the recpot unit conversion uses its own constants in the reference (ion_utils.py:11-13)
BOHR = 0.529177208607388
HARTREE_TO_EV = 27.2113834279111
POT_CONV = 1.0 / (BOHR * BOHR * BOHR * HARTREE_TO_EV)


def recpot_table(raw, k_max):
    """(ks, v, z) from the raw table in atomic units: uniform k grid, Coulomb tail 4 pi z / k^2 added for k > 0."""
    raw = np.asarray(raw, dtype=np.float64)
    ks, dk = np.linspace(0.0, float(k_max), raw.size, retstep=True)
    z = round((raw[1] - raw[0]) * dk * dk / (-4 * math.pi))                     # ion_utils.py:66
    v = raw.copy()
    v[1:] += 4 * math.pi * z / (ks[1:] * ks[1:])                                # ion_utils.py:67
    return ks, v, z


def recpot_fields(path):
    """(raw table values [file units], k_max [1/angstrom]) of a CASTEP-style .recpot file.

    Layout after the comment block (ion_utils.py:49-73 reads the same fields): one line of two integers, one line with
    k_max, then the table in rows of three numbers; a trailing row with fewer than three entries (the 1000 marker) is
    not part of the table."""
    with open(path, 'r') as fh:
        text = fh.read()
    head, sep, tail = text.partition('END COMMENT')
    if not sep:
        raise ValueError('%s: no END COMMENT marker' % path)
    rows = [ln.split() for ln in tail.splitlines()[1:]]       # [0] is the rest of the marker line
    rows = [r for r in rows if r]
    k_max = float(rows[1][0])                                 # rows[0] = the two integers
    table = [x for r in rows[2:] if len(r) == 3 for x in r]
    return np.asarray(table, dtype=np.float64), k_max


def read_recpot(path):
    """Parse a CASTEP-style .recpot file -> (ks, v, z) as `recpot_table` (units of ion_utils.py:11-13,62-66)."""
    raw, k_max = recpot_fields(path)
    return recpot_table(raw * POT_CONV, k_max * BOHR)


def _f64(engine):
    """The once-per-geometry-step routines are fp64 work: an fp32 engine hands them to its fp64 sibling (same grid,
    same device); densities are widened on the way in, the potential is narrowed on the way out."""
    if engine.dtype == torch.double:
        return engine
    from .engine import engine_for
    return engine_for(engine.global_shape, engine.device)


# ---------------------------------------------------------------------------------------------------- marshalling
_DP = C.POINTER(C.c_double)


def _arg(x):
    """an argument of a C entry: tensors and arrays as pointers, everything else as it is"""
    if torch.is_tensor(x):
        return C.c_void_p(x.data_ptr())
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.POINTER(C.c_int) if x.dtype == np.int32 else _DP)
    return x


def _ion_arrays(frac, charges=None):
    """frac as a contiguous fp64 [n, 3] array; with `charges`: (frac, z [n]), one charge per ion"""
    frac = np.ascontiguousarray(np.asarray(torch.as_tensor(frac).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3))
    if charges is None:
        return frac
    z = np.ascontiguousarray(np.asarray(charges, dtype=np.float64).reshape(-1))
    if z.size != frac.shape[0]:
        raise ValueError('one charge per ion')
    return frac, z


def _species_arrays(frac, tab):
    """(frac [n, 3], ks, v, z) of one species as the C entries take them; the table's shape is checked here, because C reads
    `ks.size` entries of both `ks` and `v`"""
    ks, v, z = tab
    ks = np.ascontiguousarray(ks, dtype=np.float64)
    v = np.ascontiguousarray(v, dtype=np.float64)
    if ks.shape != v.shape or ks.ndim != 1:
        raise ValueError('table k and v must be 1-D arrays of equal length')
    return _ion_arrays(frac), ks, v, float(z)


def _marshal(species):
    """every species through `_species_arrays`, before any engine work"""
    return [_species_arrays(frac, tab) for frac, tab in species]


def _pme_refusal(who, pme_order):
    if pme_order:
        raise NotImplementedError('%s: particle-mesh Ewald (PME, pme_order=%r) is not served; use the exact structure factor '
                                  '(pme_order=None)' % (who, pme_order))


def _species_call(engine, entry, lead, sp, pme_order, tail):
    """one call of a per-species entry: (ctx, *lead, frac, n, ks, v, ntab, z, pme_order, *tail, stream), sp from `_species_arrays`"""
    frac, ks, v, z = sp
    rc = getattr(engine.lib, entry)(engine._ctx, *map(_arg, lead), _arg(frac), frac.shape[0], _arg(ks), _arg(v), ks.size, z,
                                    0 if pme_order is None else int(pme_order), *map(_arg, tail), engine._stream())
    engine._check(rc, entry)


def _species_loop(engine, entry, lead, marshalled, new_out, pme_order=None):
    """`entry` once per species, its output in the buffer new_out(frac) (array or tensor); yields (frac, buffer) after each call"""
    for sp in marshalled:
        out = new_out(sp[0])
        _species_call(engine, entry, lead, sp, pme_order, (out,))
        yield sp[0], out


def ionic_potential(engine, box_vecs, species, pme_order=None):
    """v_ext on the engine's grid.  species: iterable of (frac_coords [n,3], (ks, v, z)) per ion type.
    pme_order None -> exact O(N_ion N_k) structure factor; even int >= 2 -> particle-mesh Ewald."""
    species = _marshal(species)
    want = engine.dtype
    engine = _f64(engine)
    engine.set_cell(box_vecs)
    out = torch.zeros(engine.shape, dtype=torch.double, device=engine.device)
    for i, sp in enumerate(species):
        _species_call(engine, 'ofdft_ionic_potential', (), sp, pme_order, (out, 1 if i else 0))      # (accumulate after the first)
    return out.to(want)


def ion_electron_forces(engine, box_vecs, den, species, pme_order=None):
    """Forces F = -dU/dR of U = int n v_ext on every ion (Ha/bohr), species by species -> list of [n,3] arrays
    (the IonElectron part of System.forces(), system.py:913-923)."""
    species = _marshal(species)
    den = engine._grid_tensor(den, 'den').double()
    engine = _f64(engine)
    engine.set_cell(box_vecs)
    return [f for _frac, f in _species_loop(engine, 'ofdft_ion_electron_forces', (den,), species, np.zeros_like, pme_order)]


def ion_electron_stress(engine, box_vecs, den, species, pme_order=None):
    """Ion-electron stress (3x3, Ha/bohr^3) with the potential rebuilt from the ions at fixed fractional coordinates
    (the IonElectron part of System.stress(), system.py:925-935), summed over species."""
    species = _marshal(species)
    den = engine._grid_tensor(den, 'den').double()
    engine = _f64(engine)
    engine.set_cell(box_vecs)
    total = np.zeros((3, 3))
    for _frac, s in _species_loop(engine, 'ofdft_ion_electron_stress', (den,), species, lambda frac: np.zeros(9), pme_order):
        total += s.reshape(3, 3)
    return total


# Bounds of ion_ion(method=...).  tools/ionion_probe.py measures the rates they stand for (profiles/ionion_cells.jsonl); NOT
# MEASURED yet, so both are set from estimates and are to be replaced by the probe's figures.
# MAX_PAIRS: the pair estimate above which method='cells' / 'auto' refuse to start, meant as about a minute of the cell-list
# kernel.  Estimate: the kernel's listing holds 534 fp64 vector instructions, about 350 of them in the pair loop (erfc, exp,
# sqrt, two divisions, eleven sums); fp64 vector issue on gfx950 is 16 lanes per cycle per SIMD, 256 CUs x 4 SIMDs x 16 x
# 2.4 GHz = 3.9e13 lane-instructions/s, so at most 1.1e11 pairs/s; half of that for a minute: 60 s x 5e10 = 3e12 pairs.
# AUTO_DIRECT_CANDIDATES: below this many (i, j, shift) candidates 'auto' takes the direct kernel (one short launch; the cell
# list first sorts the ions and tests the neighbour cells on the host).
MAX_PAIRS = 3.0e12
AUTO_DIRECT_CANDIDATES = 1.0e7


def _spacings(box):
    """interplanar spacings h_d of the lattice (rows of `box` = lattice vectors)"""
    return 1.0 / np.sqrt(np.sum(np.linalg.inv(box.T) ** 2, axis=1))


def ion_ion_cost(box_vecs, nions, Rc=None, frac=None):
    """What an ion-ion call would cost, without an engine: Rc and Rd as System.__ion_ion_interaction sets them
    (system.py:744-750), `pairs_estimate` = nions^2 (4/3) pi Rc^3 / vol ordered pairs within Rc (each pair counted from both
    ends, as both kernels visit it), and `direct_candidates` = nions^2 prod(2 nmax_d + 1), the (i, j, lattice shift)
    combinations the direct kernel scans, nmax_d = ceil(Rc / h_d + span_d).  span_d is the spread of the fractional
    coordinates along axis d: taken from `frac` when given, 1 (the bound for wrapped coordinates) otherwise."""
    box = np.asarray(torch.as_tensor(box_vecs).detach().cpu().numpy(), dtype=np.float64).reshape(3, 3)
    h = _spacings(box)
    h_max = float(h.max())
    if Rc:
        Rc = float(Rc)
        Rd = math.sqrt(h_max * Rc / 3.0)
    else:
        Rd = 2.0 * h_max
        Rc = 3.0 * Rd * Rd / h_max
    if frac is None:
        span = np.ones(3)
    else:
        f = np.asarray(torch.as_tensor(frac).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3)
        span = f.max(0) - f.min(0)
    nmax = np.ceil(Rc / h + span).astype(np.int64)
    vol = abs(float(np.linalg.det(box)))
    n = int(nions)
    return {'Rc': Rc, 'Rd': Rd, 'pairs_estimate': float(n) * n * 4.0 / 3.0 * math.pi * Rc ** 3 / vol,
            'direct_candidates': float(n) * n * float(np.prod(2 * nmax + 1))}


def ion_ion(engine, box_vecs, frac, charges, Rc=None, Rd=None, method='direct', part=0, nparts=1, max_pairs=None):
    """Ion-ion energy [Ha], forces [n,3] (Ha/bohr) and stress [3,3] (Ha/bohr^3): ion_interaction_sum with System's
    parameter heuristics (ion_utils.py:293-333, system.py:733-754) and its autograd derivatives (system.py:913-935).

    method='direct' (default): every (i, j, lattice shift) is scanned (`ofdft_ion_ion`): right for primitive cells, cost
    nions^2 x shifts.  method='cells': the cell list (`ofdft_ion_ion_cells`), for supercells; it also takes an explicit damping
    radius `Rd` (with `Rc`), and `part` / `nparts`: the share of part `part` of `nparts` contiguous ranges of target cells
    (force rows of its own ions only; the sum over parts is the whole result).  method='auto': the direct kernel below
    AUTO_DIRECT_CANDIDATES candidates, the cell list otherwise.  'cells' and 'auto' raise ValueError when `ion_ion_cost`
    estimates more than `max_pairs` (default MAX_PAIRS) pairs, before any engine work."""
    if method not in ('direct', 'cells', 'auto'):
        raise ValueError("method must be 'direct', 'cells' or 'auto'")
    if Rd is not None and not Rc:
        raise ValueError('Rd needs an explicit Rc')
    frac, z = _ion_arrays(frac, charges)
    if method == 'direct':
        if Rd is not None or part != 0 or nparts != 1:
            raise ValueError("method='direct' derives Rd from Rc and computes the whole sum: Rd, part and nparts need method='cells'")
    else:
        cost = ion_ion_cost(box_vecs, frac.shape[0], Rc, frac)
        if method == 'auto':
            method = 'direct' if (cost['direct_candidates'] < AUTO_DIRECT_CANDIDATES and Rd is None and nparts == 1) else 'cells'
        limit = MAX_PAIRS if max_pairs is None else max_pairs
        if method == 'cells' and cost['pairs_estimate'] > limit:
            raise ValueError('ion_ion: about %.3g pairs within Rc = %.6g bohr (pairs_estimate) exceed max_pairs = %.3g; the direct '
                             'kernel would scan %.3g candidates (direct_candidates).  Pass a smaller Rc or raise max_pairs.'
                             % (cost['pairs_estimate'], cost['Rc'], limit, cost['direct_candidates']))
    E = C.c_double(0.0)
    F = np.zeros_like(frac)
    S = np.zeros(9)
    if method == 'cells':
        _ion_ion_call(engine, box_vecs, 'ofdft_ion_ion_cells', frac, z, Rc, float(Rd) if Rd else 0.0, int(part), int(nparts), C.byref(E), F, S)
    else:
        _ion_ion_call(engine, box_vecs, 'ofdft_ion_ion', frac, z, Rc, C.byref(E), F, S)
    return E.value, F, S.reshape(3, 3)


def _ion_ion_call(engine, box_vecs, entry, frac, z, Rc, *tail):
    """one call of an ion-ion entry on the fp64 engine: (ctx, frac, z, n, Rc, *tail, stream); frac, z from `_ion_arrays`"""
    engine = _f64(engine)
    engine.set_cell(box_vecs)
    rc = getattr(engine.lib, entry)(engine._ctx, _arg(frac), _arg(z), frac.shape[0], float(Rc) if Rc else 0.0, *map(_arg, tail),
                                    engine._stream())
    engine._check(rc, entry)


# ---------------------------------------------------------------------------------------------------- second derivatives
def locate_ion(species, ion):
    """(species index, index within it) of the global ion index `ion` = position in the concatenation of the species"""
    ion = int(ion)
    left = ion
    for s, (frac, _tab) in enumerate(species):
        n = int(np.asarray(torch.as_tensor(frac).shape).prod()) // 3
        if 0 <= left < n:
            return s, left
        left -= n
    raise IndexError('ion index %d outside the %d ions of the species list' % (ion, ion - left))


def ionic_potential_gradient(engine, box_vecs, species, ion, pme_order=None):
    """d v_ext / d R_{ion, x|y|z} on the engine's grid -> [3, n0, n1, n2] (`ofdft_ionic_potential_gradient`: what autograd
    through lattice_sum yields, ion_utils.py:88-137).  `ion` counts over the concatenated species.  Exact structure factor only:
    a `pme_order` raises NotImplementedError (the derivative of the particle-mesh-Ewald spread is not built).  Plain fp64 work:
    an fp32 engine hands it to its fp64 sibling and gets the grids narrowed."""
    _pme_refusal('ionic_potential_gradient', pme_order)
    s, a = locate_ion(species, ion)
    sp = _species_arrays(*species[s])
    want = engine.dtype
    engine = _f64(engine)
    engine.set_cell(box_vecs)
    out = torch.empty((3,) + tuple(engine.shape), dtype=torch.double, device=engine._dev_exact)
    _species_call(engine, 'ofdft_ionic_potential_gradient', (), sp, None, (a, out))
    return out.to(want)


def ion_electron_curvature(engine, box_vecs, den, species, pme_order=None):
    """D[a] = d^2 (int n v_ext) / dR_a dR_a at fixed density for every ion, species by species -> list of [n, 3, 3] arrays
    (Ha/bohr^2; `ofdft_ion_electron_curvature`: the diagonal blocks of the Hessian of IonElectron over lattice_sum, whose
    off-diagonal blocks vanish).  fp64 engines only: the density is the engine's own, as for `Engine.stress`."""
    _pme_refusal('ion_electron_curvature', pme_order)
    species = _marshal(species)
    if engine.dtype != torch.double:
        raise NotImplementedError('ion_electron_curvature is fp64 work (libofdft_hip.so); an fp32 engine does not serve it')
    den = engine._grid_tensor(den, 'den')
    engine.set_cell(box_vecs)
    out = []
    for frac, c6 in _species_loop(engine, 'ofdft_ion_electron_curvature', (den,), species, lambda frac: np.zeros((frac.shape[0], 6))):
        D = np.empty((frac.shape[0], 3, 3))
        for k, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            D[:, i, j] = D[:, j, i] = c6[:, k]
        out.append(D)
    return out


def ion_ion_hessian(engine, box_vecs, frac, charges, rows, Rc=None):
    """d^2 E_ion-ion / dR_p dR_b for p in `rows` -> [len(rows), n, 3, 3] (Ha/bohr^2): a second autograd pass over
    ion_interaction_sum (ion_utils.py:293-333) at a fixed pair list, with the Rd / Rc rules and the pair set of
    `ion_ion(method='direct')` (`ofdft_ion_ion_hessian`).  Plain fp64 work: an fp32 engine hands it to its fp64 sibling."""
    frac, z = _ion_arrays(frac, charges)
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
    if rows.size == 0 or rows.min() < 0 or rows.max() >= frac.shape[0]:
        raise ValueError('rows must name at least one ion, each in [0, %d)' % frac.shape[0])
    H = np.zeros((rows.size, frac.shape[0], 3, 3))
    _ion_ion_call(engine, box_vecs, 'ofdft_ion_ion_hessian', frac, z, Rc, rows, rows.size, H)
    return H


# ---------------------------------------------------------------------------------------------------- strain derivatives
def ionic_potential_strain_gradient(engine, box_vecs, species, pme_order=None):
    """d v_ext / d eps_kl, kl = xx, yy, zz, yz, xz, xy, under h -> h (I + eps) at fixed fractional coordinates -> [6, n0, n1, n2]:
    -delta_kl v_ext + F^-1[S v~'(|k|) (-k_k k_l / |k|)] / vol summed over the species (`ofdft_ionic_potential_strain_gradient`;
    DESIGN.md §9e).  Exact structure factor only.  Plain fp64 work: an fp32 engine hands it to its fp64 sibling."""
    _pme_refusal('ionic_potential_strain_gradient', pme_order)
    species = _marshal(species)
    want = engine.dtype
    engine = _f64(engine)
    engine.set_cell(box_vecs)
    total = None
    new_out = lambda frac: torch.empty((6,) + tuple(engine.shape), dtype=torch.double, device=engine._dev_exact)  # noqa: E731
    for _frac, out in _species_loop(engine, 'ofdft_ionic_potential_strain_gradient', (), species, new_out):
        total = out if total is None else total + out
    return total.to(want)


def ion_electron_strain_hessian(engine, box_vecs, den, species, pme_order=None):
    """d^2 (int n v_ext) / d eps_mn d eps_pq -> [3, 3, 3, 3] (Ha) at fixed grid values of chi (n ~ 1 / det(I + eps)) and fixed
    fractional coordinates, the potential rebuilt from the ions in the strained cell, summed over the species
    (`ofdft_ion_electron_strain_hessian`).  fp64 engines only: the density is the engine's own, as for `Engine.stress`."""
    _pme_refusal('ion_electron_strain_hessian', pme_order)
    species = _marshal(species)
    if engine.dtype != torch.double:
        raise NotImplementedError('ion_electron_strain_hessian is fp64 work (libofdft_hip.so); an fp32 engine does not serve it')
    den = engine._grid_tensor(den, 'den')
    engine.set_cell(box_vecs)
    total = np.zeros(81)
    for _frac, w in _species_loop(engine, 'ofdft_ion_electron_strain_hessian', (den,), species, lambda frac: np.zeros(81)):
        total += w
    return total.reshape(3, 3, 3, 3)


def ion_ion_strain_hessian(engine, box_vecs, frac, charges, Rc=None):
    """d^2 E_ion-ion / d eps_mn d eps_pq -> [3, 3, 3, 3] (Ha) at fixed fractional coordinates: the pair sum over the fixed pair list
    of `ion_ion(method='direct')` with Rd and Rc held (the reference takes h_max from box_vecs.detach()), plus the background
    term through rho ~ 1/J and R_a ~ J^(1/3) (`ofdft_ion_ion_strain_hessian`).  Plain fp64 work."""
    frac, z = _ion_arrays(frac, charges)
    w = np.zeros(81)
    _ion_ion_call(engine, box_vecs, 'ofdft_ion_ion_strain_hessian', frac, z, Rc, w)
    return w.reshape(3, 3, 3, 3)
