"""numpy double of the cell-list ion-ion enumeration (professad_amd/csrc/engine_ion_cells.inc.h, csrc/ion_cells.h): the rule
for the cells per axis, wrapping and binning, the neighbour runs with their distance test, the lattice shift of a wrapped
offset, the tile size and the `part` ownership -- so that the pair set is tested without a GPU (tests/test_ionion_cells_cpu.py)
and tools/ionion_probe.py can record the cells and occupancies a call uses.  Not the product: nothing in professad_amd imports it.
"""
import itertools
import math

import numpy as np

OCCUPANCY = 32.0          # mean ions per cell the rule for m aims at (kIonCellOccupancy)
THREADS = 256             # lanes of a workgroup (kIonCellThreads)


def spacings(box):
    """interplanar spacings h_d (rows of box = lattice vectors)"""
    return 1.0 / np.sqrt(np.sum(np.linalg.inv(box.T) ** 2, axis=1))


def choose_cells(box, nions):
    """m_d = round(h_d / edge), edge = cbrt(OCCUPANCY vol / nions), between 1 and 1024"""
    edge = np.cbrt(OCCUPANCY * abs(np.linalg.det(box)) / nions)
    return tuple(int(min(1024.0, max(1.0, math.floor(h / edge + 0.5)))) for h in spacings(box))


def bin_ions(frac, m):
    """wrapped fractional coordinates, cell of every ion, the sorted order (stable) and cell_start[ncells + 1]"""
    f = frac - np.floor(frac)
    f = f - np.floor(f)
    f[f >= 1.0] = 0.0
    m = np.asarray(m)
    ci = np.minimum(m - 1, (f * m).astype(np.int64))
    cell = (ci[:, 0] * m[1] + ci[:, 1]) * m[2] + ci[:, 2]
    order = np.argsort(cell, kind='stable')
    cell_start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=int(np.prod(m))))])
    return f, cell, order, cell_start


def tile_targets(counts):
    """target ions per tile: the T in {4 .. 256} with the fewest lane slots sum ceil(n_c / T) (T + 2), the larger T on a tie"""
    best, T = None, 4
    t = 4
    while t <= THREADS:
        cost = int(np.sum(-(-np.asarray(counts) // t)) * (t + 2))
        if best is None or cost <= best:
            best, T = cost, t
        t *= 2
    return T


def cell_pair_min_dist2(G, o):
    """smallest v G v over o_d - 1 <= v_d <= o_d + 1: squared distance between the closest points of two cells whose indices
    differ by o (G = Gram matrix of lattice vector d / m_d).  Every active set is solved; feasible stationary points only."""
    o = np.asarray(o, dtype=np.float64)
    best = np.inf
    for st in itertools.product((0, 1, 2), repeat=3):      # 0 free, 1 lower bound, 2 upper bound
        v = np.where(np.array(st) == 1, o - 1.0, o + 1.0)
        free = [d for d in range(3) if st[d] == 0]
        fixed = [d for d in range(3) if st[d] != 0]
        if free:
            rhs = -G[np.ix_(free, fixed)] @ v[fixed] if fixed else np.zeros(len(free))
            v[free] = np.linalg.solve(G[np.ix_(free, free)], rhs)
            if np.any(np.abs(v[free] - o[free]) > 1.0 + 1e-9):
                continue
        best = min(best, float(v @ G @ v))
    return max(best, 0.0)


def neighbour_runs(box, m, Rc, prune=True):
    """runs (o0, o1, lo, hi): offsets |o_d| <= floor(Rc m_d / h_d) + 1, and with `prune` only those whose cells can hold a pair
    within Rc (lo..hi = first and last such o2 of a row)"""
    m = np.asarray(m)
    R = (np.floor(Rc * m / spacings(box)) + 1).astype(int)
    U = box / m[:, None]
    G = U @ U.T
    keep2 = Rc * Rc * (1.0 + 1e-9)
    runs = []
    for o0 in range(-R[0], R[0] + 1):
        for o1 in range(-R[1], R[1] + 1):
            ok = [o2 for o2 in range(-R[2], R[2] + 1) if not prune or cell_pair_min_dist2(G, (o0, o1, o2)) <= keep2]
            if ok:
                runs.append((o0, o1, ok[0], ok[-1]))
    return runs


def owned_cells(ncells, part, nparts):
    """target cells of part `part`: [part ncells // nparts, (part + 1) ncells // nparts)"""
    return part * ncells // nparts, (part + 1) * ncells // nparts


def pairs(box, frac, Rc, m=None, prune=True, part=0, nparts=1):
    """{ion: distances r of its pairs 0 < r <= Rc} for the target ions part `part` owns, walking the cells as the kernel does"""
    box = np.asarray(box, dtype=np.float64)
    frac = np.asarray(frac, dtype=np.float64)
    m = choose_cells(box, frac.shape[0]) if m is None else tuple(m)
    f, cell, order, cell_start = bin_ions(frac, m)
    cart = (f @ box)[order]
    runs = neighbour_runs(box, m, Rc, prune)
    c_lo, c_hi = owned_cells(int(np.prod(m)), part, nparts)
    out = {}
    for c in range(c_lo, c_hi):
        c0, c1, c2 = c // (m[1] * m[2]), (c // m[2]) % m[1], c % m[2]
        targets = range(cell_start[c], cell_start[c + 1])
        found = {t: [] for t in targets}
        for o0, o1, lo, hi in runs:
            q0, w0 = divmod(c0 + o0, m[0])          # floor division: the lattice shift of a wrapped offset
            q1, w1 = divmod(c1 + o1, m[1])
            rowbase = (w0 * m[1] + w1) * m[2]
            a, b = c2 + lo, c2 + hi
            for q in range(a // m[2], b // m[2] + 1):
                s, e = max(a, q * m[2]) - q * m[2], min(b, q * m[2] + m[2] - 1) - q * m[2]
                j0, j1 = cell_start[rowbase + s], cell_start[rowbase + e + 1]
                if j1 == j0:
                    continue
                shifted = cart[j0:j1] + q0 * box[0] + q1 * box[1] + q * box[2]
                for t in targets:
                    r = np.linalg.norm(shifted - cart[t], axis=1)
                    found[t].append(r[(r * r > 1e-24) & (r <= Rc)])
        for t in targets:
            out[int(order[t])] = np.concatenate(found[t]) if found[t] else np.zeros(0)
    return out
