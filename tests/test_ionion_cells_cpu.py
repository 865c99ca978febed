"""Cell-list ion-ion sum, the parts that need no GPU: the enumeration (numpy double of the host side and the kernel's walk)
against the oracle's pair list, the cost estimate and its refusal of hopeless calls, and the ABI declaration."""
import os
import re

import numpy as np
import pytest

import ionion_cells_double as cd
from oracle import ionion as ii
from professad_amd import _native as N
from professad_amd import ions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRI = np.array([[9.1, 0.4, -0.7], [1.3, 8.2, 0.9], [-0.5, 2.1, 10.3]])


def _tri_case():
    frac = np.random.default_rng(5).uniform(-0.7, 1.9, (23, 3))
    return TRI, frac


@pytest.mark.parametrize('Rc', [4.0, 11.0, 23.0])
@pytest.mark.parametrize('m', [(1, 1, 1), (2, 3, 1), (4, 4, 4), (5, 2, 7)])
def test_double_pair_counts_and_inverse_distance_sums_match_oracle(m, Rc):
    """triclinic box, 23 ions with fractional coordinates in (-0.7, 1.9), Rc below and above the box: per-ion pair counts and
    sum 1/r of the cell walk (with and without the distance test on cell pairs) equal the oracle's shift scan"""
    box, frac = _tri_case()
    ref_far = ii.pairs(box, frac @ box, Rc + 1e-6)
    r_all = np.concatenate([p[3] for p in ref_far])
    assert np.abs(r_all - Rc).min() > 1e-9
    ref = ii.pairs(box, frac @ box, Rc)
    cnt = np.zeros(23, dtype=int)
    inv = np.zeros(23)
    for i, j, d, r in ref:
        cnt[i] += r.size
        inv[i] += np.sum(1.0 / r)
    for prune in (False, True):
        got = cd.pairs(box, frac, Rc, m=m, prune=prune)
        assert sorted(got) == list(range(23))
        assert [got[i].size for i in range(23)] == list(cnt), (m, Rc, prune)
        assert np.allclose([np.sum(1.0 / got[i]) for i in range(23)], inv, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize('nparts', [1, 3, 4])
def test_parts_own_every_target_ion_exactly_once(nparts):
    box, frac = _tri_case()
    whole = cd.pairs(box, frac, 11.0, m=(2, 3, 1))
    seen = []
    for part in range(nparts):
        got = cd.pairs(box, frac, 11.0, m=(2, 3, 1), part=part, nparts=nparts)
        seen += list(got)
        for i, r in got.items():
            assert np.array_equal(r, whole[i])         # a target's walk does not depend on the split
    assert sorted(seen) == list(range(23))
    lo_hi = [cd.owned_cells(6, p, nparts) for p in range(nparts)]
    assert lo_hi[0][0] == 0 and lo_hi[-1][1] == 6 and all(a[1] == b[0] for a, b in zip(lo_hi, lo_hi[1:]))


def test_cell_rule_and_tile_size():
    """m_d = round(h_d / cbrt(32 vol / nions)); the tile is the T with the fewest lane slots"""
    a = 7.65
    assert cd.choose_cells(np.eye(3) * a, 4) == (1, 1, 1)
    assert cd.choose_cells(np.eye(3) * 16 * a, 4 * 16 ** 3) == (8, 8, 8)           # 32 ions per cell
    assert cd.choose_cells(np.diag([4 * a, 4 * a, 32 * a]), 4 * 4 * 4 * 32) == (2, 2, 16)
    assert cd.tile_targets([32] * 512) == 32
    assert cd.tile_targets([2]) == 4
    assert cd.tile_targets([500]) == 256
    assert cd.tile_targets([20] * 100) in (4, 8, 16, 32)
    # the distance test never drops a cell pair that holds a pair within Rc (brute force on random points of both cells)
    rng = np.random.default_rng(3)
    m = np.array([2, 3, 1])
    U = TRI / m[:, None]
    G = U @ U.T
    for o in [(0, 0, 0), (1, 0, 0), (2, -1, 1), (-3, 2, 0), (1, 1, -2)]:
        t = rng.uniform(-1, 1, (4000, 3)) + np.array(o)
        d2 = np.einsum('pi,ij,pj->p', t, G, t)
        assert cd.cell_pair_min_dist2(G, o) <= d2.min() + 1e-12


def test_ion_ion_cost_matches_oracle_heuristics_and_direct_candidates():
    rng = np.random.default_rng(11)
    for box, n, Rc in ((TRI, 23, None), (TRI, 23, 17.5), (np.diag([6.0, 7.5, 11.0]), 8, None), (np.diag([6.0, 7.5, 11.0]), 8, 30.0)):
        frac = rng.uniform(0.05, 0.9, (n, 3))
        cost = ions.ion_ion_cost(box, n, Rc, frac=frac)
        Rc_o, Rd_o = ii.heuristics(box, Rc)
        assert cost['Rc'] == pytest.approx(Rc_o, rel=1e-15) and cost['Rd'] == pytest.approx(Rd_o, rel=1e-15)
        h = 1.0 / np.sqrt(np.sum(np.linalg.inv(box.T) ** 2, axis=1))
        # the direct path (csrc/engine_ions_stress.inc.h): nmax_d = ceil(Rc / h_d + span_d), block (chunk, i) scans nions x shifts
        nmax = np.ceil(Rc_o / h + (frac.max(0) - frac.min(0))).astype(int)
        assert cost['direct_candidates'] == n * n * np.prod(2 * nmax + 1)
        assert cost['pairs_estimate'] == pytest.approx(n * n * 4 / 3 * np.pi * Rc_o ** 3 / abs(np.linalg.det(box)), rel=1e-14)
        # without coordinates: the bound for wrapped ones
        assert ions.ion_ion_cost(box, n, Rc)['direct_candidates'] >= cost['direct_candidates']


def test_cells_refuses_a_default_cutoff_supercell_before_touching_the_engine():
    """131 072 ions in a 245-bohr cube at the default Rc (= 12 h_max = 2 940 bohr): ~1e14 pairs"""
    n = 131072
    box = np.eye(3) * 245.0
    frac = np.random.default_rng(2).random((n, 3))
    cost = ions.ion_ion_cost(box, n)
    assert cost['Rc'] == pytest.approx(2940.0) and cost['pairs_estimate'] > 1e14 and cost['pairs_estimate'] > ions.MAX_PAIRS
    for method in ('cells', 'auto'):
        with pytest.raises(ValueError) as e:
            ions.ion_ion(None, box, frac, np.full(n, 3.0), method=method)           # engine None: it must not be reached
        assert 'pairs_estimate' in str(e.value) and 'direct_candidates' in str(e.value)
        assert '%.3g' % cost['pairs_estimate'] in str(e.value) and '%.3g' % cost['direct_candidates'] in str(e.value)
    with pytest.raises(ValueError):
        ions.ion_ion(None, box, frac[:4], np.ones(4), Rc=20.0, Rd=3.0)              # direct derives Rd itself
    with pytest.raises(ValueError):
        ions.ion_ion(None, box, frac[:4], np.ones(4), part=1, nparts=2)


def test_abi_declares_and_binds_the_cell_list_entry():
    assert 'ofdft_ion_ion_cells' in N.EXPORTS
    header = open(os.path.join(ROOT, 'include', 'ofdft_hip.h')).read()
    decl = re.search(r'int\s+ofdft_ion_ion_cells\(([^;]*)\);', header)
    assert decl and decl.group(1).count(',') == 11                   # twelve parameters
    for dtype in (N.F64, N.F32):
        lib = N.load(dtype)
        assert hasattr(lib, 'ofdft_ion_ion_cells')
        assert len(lib.ofdft_ion_ion_cells.argtypes) == 12
    # the fp32 library refuses per-geometry work; a null context is EINVAL in both
    assert N.load(N.F32).ofdft_ion_ion_cells(None, None, None, 0, 0.0, 0.0, 0, 1, None, None, None, None) == N.EINVAL
    assert N.load(N.F64).ofdft_ion_ion_cells(None, None, None, 0, 0.0, 0.0, 0, 1, None, None, None, None) == N.EINVAL
