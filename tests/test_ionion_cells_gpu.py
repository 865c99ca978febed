"""Cell-list ion-ion sum (ofdft_ion_ion_cells, csrc/ion_cells.h) on the GPU: the reference's known answers, supercell tiling with
an explicit damping radius, agreement with the direct kernel on one input, the part split, two ranks, error paths.

Tolerances are the ones tests/test_gpu_parity.py applies to the direct kernel: |dE| / nions 1e-10 against known answers and
1e-11 against the oracle, forces 1e-11 Ha/bohr, stress 1e-12 Ha/bohr^3.  Every case that compares pair sums first asserts that
no pair distance lies within 1e-9 bohr of Rc (wrapping changes the last bit of a distance)."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import ionion_cells_double as cd
from oracle import ionion as ii
from professad_amd import _native as N
from professad_amd.engine import Engine
from professad_amd.ions import ion_ion, ion_ion_cost

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
DEV = 'cuda:0'
TRI2 = np.array([[6.5, -0.13, 0.25], [-0.33, 7.21, 0.24], [0.55, 0.04, 6.78]])
FRAC2 = np.array([[0, 0, 0], [0.35, 0.65, 0.45]], dtype=np.float64)


def _spacings(box):
    return 1.0 / np.sqrt(np.sum(np.linalg.inv(box.T) ** 2, axis=1))


def _gap_to_cutoff(box, frac, Rc):
    """min | |R_j + shift - R_i| - Rc | over all pairs and the lattice shifts whose image of the cell comes within Rc + 1"""
    f = frac - np.floor(frac)
    cart = f @ box
    nmax = np.ceil((Rc + 1.0) / _spacings(box) + 1).astype(int)
    G = box @ box.T
    n2 = np.sum(cart * cart, axis=1)
    gap2 = np.inf
    for o in np.stack(np.meshgrid(*[np.arange(-n, n + 1) for n in nmax], indexing='ij'), -1).reshape(-1, 3):
        if cd.cell_pair_min_dist2(G, o) > (Rc + 1.0) ** 2:
            continue
        b = cart + o @ box
        r2 = n2[:, None] + np.sum(b * b, axis=1)[None, :] - 2.0 * cart @ b.T       # |b_j - a_i|^2 (error ~1e-11 << 2 Rc 1e-9)
        gap2 = min(gap2, float(np.abs(r2 - Rc * Rc).min()))
    return gap2 / (2.0 * Rc)


def _supercell(box, frac, n):
    n = np.asarray(n)
    g = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing='ij'), -1).reshape(-1, 1, 3)
    return box * n[:, None], ((frac[None, :, :] + g) / n).reshape(-1, 3), g.shape[0]


def _fcc_al(ncell, seed, amp=0.02):
    a = 7.65
    box = ncell * 0.5 * a * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    g = np.stack(np.meshgrid(*[np.arange(ncell)] * 3, indexing='ij'), -1).reshape(-1, 3)
    frac = (g + 0.25) / ncell + np.random.default_rng(seed).uniform(-amp, amp, (g.shape[0], 3)) / ncell
    return box, frac, np.full(g.shape[0], 3.0)


def test_known_answers_forces_and_stress_through_the_cell_list():
    """the six cases of ion_ion_known_answers.json at Rc = 12 h_max (m = (1, 1, 1): the cell walk is the shift scan), the
    Madelung identity, Si / SiO2 forces and stress against the oracle, and the default-parameter triclinic cell"""
    doc = json.load(open(os.path.join(GOLDEN, 'ion_ion_known_answers.json')))
    eng = Engine((16, 16, 16), DEV)
    E = {}
    for c in doc['cases']:
        box = np.array(c['box'], dtype=np.float64)
        frac = np.array(c['frac'], dtype=np.float64) if c['frac'] is not None else np.array(c['cart'], dtype=np.float64) @ np.linalg.inv(box)
        z = np.array(c['charges'], dtype=np.float64)
        E[c['name']], F, S = ion_ion(eng, box, frac, z, Rc=12 * c['h_max'], method='cells')
        print(c['name'], E[c['name']], c['expected'])
        if c['expected'] is not None:
            assert abs(E[c['name']] - c['expected']) / len(z) < 1e-10, (c['name'], E[c['name']])
        if c['name'] in ('Si', 'SiO2'):
            Rc = 12 * c['h_max']
            Rd = float(np.sqrt(_spacings(box).max() * Rc / 3))
            Fo, So = ii.forces_stress(box, frac @ box, z, Rc, Rd)
            print(c['name'], np.abs(F - Fo).max(), np.abs(S - So).max())
            assert np.abs(F - Fo).max() < 1e-11 and np.abs(S - So).max() < 1e-12, c['name']
    assert abs(4 * E['NaCl_fcc'] - E['NaCl_two'] - doc['madelung']) < 1e-10
    Ed, Fd, Sd = ion_ion(eng, TRI2, FRAC2, [1.0, 1.0], method='cells')
    Rc, Rd = ii.heuristics(TRI2)
    Fo, So = ii.forces_stress(TRI2, FRAC2 @ TRI2, np.array([1.0, 1.0]), Rc, Rd)
    assert abs(Ed - ii.energy(TRI2, FRAC2 @ TRI2, np.array([1.0, 1.0]), Rc, Rd)) < 1e-11
    assert np.abs(Fd - Fo).max() < 1e-11 and np.abs(Sd - So).max() < 1e-12
    eng.close()


def test_supercells_repeat_the_primitive_cell_with_explicit_rd():
    """2-ion triclinic cell (charges 1, 2; Rc = 20, Rd = 3.5) against its 4x4x4 and 6x5x4 supercells: E_super = M E_prim, forces
    repeat, stress equal; the 128-ion supercell also against the oracle.  (The oracle itself holds the identity to 2e-15 /
    2e-16 / 6e-18 up to 128 ions, so the tolerances are the kernel's.)"""
    Rc, Rd = 20.0, 3.5
    z = np.array([1.0, 2.0])
    assert _gap_to_cutoff(TRI2, FRAC2, Rc) > 1e-9
    eng = Engine((16, 16, 16), DEV)
    E1, F1, S1 = ion_ion(eng, TRI2, FRAC2, z, Rc=Rc, Rd=Rd, method='cells')
    Eo = ii.energy(TRI2, FRAC2 @ TRI2, z, Rc, Rd)
    Fo, So = ii.forces_stress(TRI2, FRAC2 @ TRI2, z, Rc, Rd)
    print('prim', abs(E1 - Eo) / 2, np.abs(F1 - Fo).max(), np.abs(S1 - So).max())
    assert abs(E1 - Eo) / 2 < 1e-11 and np.abs(F1 - Fo).max() < 1e-11 and np.abs(S1 - So).max() < 1e-12
    for n in ((4, 4, 4), (6, 5, 4)):
        box, frac, M = _supercell(TRI2, FRAC2, n)
        zs = np.tile(z, M)
        E, F, S = ion_ion(eng, box, frac, zs, Rc=Rc, Rd=Rd, method='cells')
        print(n, abs(E - M * E1) / (2 * M), np.abs(F - np.tile(F1, (M, 1))).max(), np.abs(S - S1).max())
        assert abs(E - M * E1) / (2 * M) < 1e-11
        assert np.abs(F - np.tile(F1, (M, 1))).max() < 1e-11
        assert np.abs(S - S1).max() < 1e-12
        if M == 64:
            Eo = ii.energy(box, frac @ box, zs, Rc, Rd)
            Fo, So = ii.forces_stress(box, frac @ box, zs, Rc, Rd)
            print('oracle 128', abs(E - Eo) / 128, np.abs(F - Fo).max(), np.abs(S - So).max())
            assert abs(E - Eo) / 128 < 1e-11 and np.abs(F - Fo).max() < 1e-11 and np.abs(S - So).max() < 1e-12
    eng.close()


def _mixed_500():
    rng = np.random.default_rng(17)
    box = 4.0 * np.array([[9.1, 0.4, -0.7], [1.3, 8.2, 0.9], [-0.5, 2.1, 10.3]])
    g = np.stack(np.meshgrid(np.arange(5), np.arange(10), np.arange(10), indexing='ij'), -1).reshape(-1, 3)
    frac = (g + 0.5 + rng.uniform(-0.3, 0.3, g.shape)) / np.array([5, 10, 10]) + rng.integers(-1, 2, g.shape)
    return box, frac, rng.integers(1, 4, g.shape[0]).astype(np.float64), 14.0


@pytest.mark.parametrize('case', ['fcc4096', 'tri500'])
def test_cells_match_the_direct_kernel_on_one_input(case):
    """4 096 displaced fcc-Al ions (16^3 primitive cells; heuristic Rd, Rc with direct_candidates < 1e10) and a triclinic 500-ion
    mixed-charge case with coordinates outside [0, 1): the two kernels on the same input"""
    if case == 'fcc4096':
        box, frac, z = _fcc_al(16, seed=7)
        Rc = 40.0
    else:
        box, frac, z, Rc = _mixed_500()
    assert ion_ion_cost(box, len(z), Rc, frac)['direct_candidates'] < 1e10
    assert _gap_to_cutoff(box, frac, Rc) > 1e-9
    eng = Engine((16, 16, 16), DEV)
    Ed, Fd, Sd = ion_ion(eng, box, frac, z, Rc=Rc)
    Ec, Fc, Sc = ion_ion(eng, box, frac, z, Rc=Rc, method='cells')
    print(case, 'dE/N', abs(Ec - Ed) / len(z), 'dF', np.abs(Fc - Fd).max(), 'dS', np.abs(Sc - Sd).max(), 'E/N', Ed / len(z))
    assert abs(Ec - Ed) / len(z) < 1e-11
    assert np.abs(Fc - Fd).max() < 1e-11
    assert np.abs(Sc - Sd).max() < 1e-12
    assert np.abs(Fd).max() > 1e-4                    # displaced ions: the forces are not zero by symmetry
    eng.close()


def test_parts_sum_to_the_whole_and_calls_are_bitwise_reproducible():
    box, frac, z, Rc = _mixed_500()
    eng = Engine((16, 16, 16), DEV)
    E, F, S = ion_ion(eng, box, frac, z, Rc=Rc, method='cells')
    E2, F2, S2 = ion_ion(eng, box, frac, z, Rc=Rc, method='cells')
    assert E == E2 and np.array_equal(F, F2) and np.array_equal(S, S2)
    Es, Fs, Ss, owners = 0.0, np.zeros_like(F), np.zeros_like(S), np.zeros(len(z), dtype=int)
    for part in range(4):
        Ep, Fp, Sp = ion_ion(eng, box, frac, z, Rc=Rc, method='cells', part=part, nparts=4)
        own = np.any(Fp != 0.0, axis=1)
        assert np.array_equal(Fp[own], F[own])            # a target's sums do not depend on the split
        owners += own
        Es, Fs, Ss = Es + Ep, Fs + Fp, Ss + Sp
    assert np.all(owners == 1)                            # every ion's force row comes from exactly one part, zero elsewhere
    assert abs(Es - E) <= 1e-13 * abs(E) and np.abs(Ss - S).max() <= 1e-13 * np.abs(S).max()
    assert np.abs(Fs - F).max() <= 1e-13
    eng.close()


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_dist_engine_ion_ion_on_two_ranks_matches_one_rank(tmp_path):
    """DistEngine.ion_ion: two gloo ranks sharing cuda:0, rank r = part r of 2, one all-reduce (tests/ionion_dist_worker.py)"""
    out = str(tmp_path / 'ionion_dist.json')
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'ionion_dist_worker.py'), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors='replace')[-2000:])
    assert all(p.returncode == 0 for p in procs), '\n----\n'.join(logs)
    w = json.load(open(out))
    print(w)
    assert w['world'] == 2
    assert w['dE_rel'] <= 1e-13 and w['dS_rel'] <= 1e-13 and w['dF'] <= 1e-13


def test_error_paths():
    box, frac, z = TRI2, FRAC2, [1.0, 2.0]
    e32 = Engine((16, 16, 16), DEV, dtype=torch.float32)
    e64 = Engine((16, 16, 16), DEV)
    a = ion_ion(e32, box, frac, z, Rc=20.0, Rd=3.5, method='cells')        # an fp32 engine hands the call to its fp64 sibling
    b = ion_ion(e64, box, frac, z, Rc=20.0, Rd=3.5, method='cells')
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    auto = ion_ion(e64, box, frac, z, Rc=20.0, method='auto')               # few candidates: the direct kernel, bit for bit
    direct = ion_ion(e64, box, frac, z, Rc=20.0)
    assert auto[0] == direct[0] and np.array_equal(auto[1], direct[1])
    with pytest.raises(ValueError):
        ion_ion(e64, box, frac, z, Rc=20.0, Rd=3.5)                         # method='direct' refuses Rd
    with pytest.raises(ValueError):
        ion_ion(e64, box, frac, z, Rc=20.0, method='cells', max_pairs=10.0)
    dp = C.POINTER(C.c_double)
    f = np.ascontiguousarray(frac)
    q = np.array(z)
    E = C.c_double(0.0)
    fresh = Engine((8, 8, 8), DEV)                                          # no ofdft_set_cell yet
    args = (f.ctypes.data_as(dp), q.ctypes.data_as(dp), 2, 20.0, 3.5)
    assert fresh.lib.ofdft_ion_ion_cells(fresh._ctx, *args, 0, 1, C.byref(E), None, None, None) == N.ESTATE
    assert b'ofdft_set_cell' in fresh.lib.ofdft_last_error(fresh._ctx)
    assert e64.lib.ofdft_ion_ion_cells(e64._ctx, *args, 2, 2, C.byref(E), None, None, None) == N.EINVAL       # part >= nparts
    assert e32.lib.ofdft_ion_ion_cells(e32._ctx, *args, 0, 1, C.byref(E), None, None, None) == N.EINVAL       # fp32 library
    assert e64.lib.ofdft_ion_ion_cells(e64._ctx, *args, 0, 1, C.byref(E), None, None, None) == N.OK           # E only
    assert E.value == b[0]
    for e in (e32, e64, fresh):
        e.close()
