"""The slab-decomposed (x-slab, nranks > 1) pipeline against the fp64 oracle and against one engine, per term set.

P ranks are emulated as P contexts in one process (tests/local_ranks.py): the kernels, the exchange layout (records per peer and
x plane, 8-plane kz blocks plus the remainder planes, XfLayout strides, the WGC99 table laid out like the buffers, the kz-chunk
views) and the step sequence are those of a P-GPU job; only the all-to-all is a copy.  Term sets, oracle, cells and inputs are
those of the extent matrix (tests/test_extent_matrix_gpu.py), the comparison is tests/spectral_check.py (real space and per
k-point), both builds, both OFDFT_OPT_GGA_SPLIT values, both entry points (density in / chi in).

What the slab path serves of M.TERM_SETS: everything but wts_exp (refused by ofdft_dist_begin); a Laplacian-dependent GGA
(pgslr_h, pgsl025) only with the split chain (OFDFT_OPT_GGA_SPLIT 0 is refused by ofdft_dist_begin); OFDFT_NLK is refused by
ofdft_set_terms.

Geometries (shape, P, cell), each for one property of the exchange layout -- all nine are admitted by ofdft_create_dist
(line_extent_ok / row_extent_ok, n2 / 2 <= 512):
  16 x 16 x 16, 8, tri      nxl = nyl = 2, one kz block (nzc = 9: 8 + 1 remainder plane)
  8 x 8 x 32, 8, ortho      nxl = nyl = 1
  64 x 32 x 48, 4, ortho    mixed-radix z row (24 points), orthogonal cell (WGC99 table fold on one GPU, not on slabs)
  96 x 48 x 120, 4, tri     mixed-radix on all axes, nzc = 61: 7 blocks + 5 remainder planes
  32 x 64 x 270, 8, ortho   no remainder planes (nzc = 136 = 17 x 8); 270 is a row extent (OFDFT_MIXED_LINES)
  16 x 16 x 1024, 2, tri    n2 / 2 = 512, the admitted maximum
  512 x 16 x 16, 2, ortho   long exchanged x lines
  1024 x 8 x 16, 8, ortho   the longest x line, nyl = 1
  64 x 64 x 32, 2, tri      nxl = nyl = 32, two kz blocks: the smallest shape xchg_chunks_for cuts into chunks
n2 = 8 (nzc = 5: no kz block, remainder planes only) has no row plan (row_extent_ok: powers of two from 16), so a slab context
on 16 x 16 x 8 is refused at create; that is asserted below.

Bounds: against the oracle those of tests/spectral_check.py, unchanged (the maxima measured here are recorded there); against
one engine 1e-12 (fp64, as tests/test_dist_gpu.py: test_eight_rank_geometry_in_one_process) and 5e-6 / 5e-4 (fp32, as its
_check_worker_results).
"""
import time

import numpy as np
import pytest
import torch

import spectral_check as sc
import test_chirpz_matrix_gpu as C
import test_extent_matrix_gpu as M
from local_ranks import LocalRanks
from professad_amd import _native as N
from professad_amd.distributed import HipStages
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = M.DEV

GEOMETRIES = [
    ((16, 16, 16), 8, 'tri'),
    ((8, 8, 32), 8, 'ortho'),
    ((64, 32, 48), 4, 'ortho'),
    ((96, 48, 120), 4, 'tri'),
    ((32, 64, 270), 8, 'ortho'),
    ((16, 16, 1024), 2, 'tri'),
    ((512, 16, 16), 2, 'ortho'),
    ((1024, 8, 16), 8, 'ortho'),
    ((64, 64, 32), 2, 'tri'),
]
# (shape, P, cell, kz chunks): two blocks in two chunks; seven blocks + five remainder planes in chunks of 2, 2 and 3 blocks
CHUNKED = [((64, 64, 32), 2, 'tri', 2), ((64, 64, 120), 2, 'tri', 3)]
SERVED = [ts for ts in M.TERM_SETS if ts != 'wts_exp']
# slabs against one engine, relative: energies per term and mu to max(1, |.|), v and chi.grad to their max magnitude
SINGLE_TOL = {'f64': dict(E=1e-12, mu=1e-12, g=1e-12, v=1e-12), 'f32': dict(E=5e-6, mu=5e-6, g=5e-4, v=5e-4)}
REFUSED_SPLIT0 = 'Laplacian-dependent Pauli-Gaussian members need the split-derivative GGA chain'
REFUSED_WTS = 'the stabilised Wang-Teter style functional .* is served by single-GPU contexts'
REFUSED_NLK = 'OFDFT_NLK .* is served by single-GPU contexts'
REFUSED_DIVISIBLE = 'slab decomposition needs n0 and n1 divisible by the rank count 4'
REFUSED_EXTENT = 'the slab-decomposed path needs extents with a line-transform plan'


def _gid(g):
    return '%dx%dx%d-P%d-%s' % (g[0] + (g[1], g[2]))


def _tensors(fields, dt):
    return [torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV) for a in fields]


def _set_split(loc, gs):
    for s in loc.st:
        s.set_option(N.OPT_GGA_SPLIT, gs)


def _kinds(loc):
    return [int(s.query(N.Q_XPASS_KINDS)) for s in loc.st]


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _field_rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _checked(bad, what, *a, **kw):
    """sc.check, its failure collected instead of raised: one report covers the whole case"""
    try:
        sc.check(*a, **kw)
    except AssertionError as e:
        bad.append((what, 'oracle') + e.args)


def run_case(shape, P, cell, ts):
    o = M.oracle(shape, cell, ts)
    names, params, _ = M.TERM_SETS[ts]
    box = torch.as_tensor(o['box'])
    bad = []
    for p in ('f64', 'f32'):
        dt = M.DTYPES[p]
        den, vext, chi = _tensors((o['den'], o['vext'], o['chi']), dt)
        ref = Engine(shape, DEV, dtype=dt).set_cell(box).set_terms(names, params)
        ref.set_option(N.OPT_GRAPH, 0).set_option(N.OPT_RESIDENT, 0)
        loc = LocalRanks(shape, DEV, P, dtype=dt).set_cell(box).set_terms(names, params)
        try:
            for gs in (0, 1):          # (the refused form first: the served one then runs on contexts that have refused a call)
                what = (shape, P, cell, ts, p, 'gga_split=%d' % gs)
                _set_split(loc, gs)
                ref.set_option(N.OPT_GGA_SPLIT, gs)
                if ts in M.LAPLACIAN_GGA and gs == 0:
                    with pytest.raises(RuntimeError, match=REFUSED_SPLIT0):
                        loc.energy_potential(den, vext)
                    with pytest.raises(RuntimeError, match=REFUSED_SPLIT0):
                        loc.closure(chi, o['n_elec'], vext)
                    continue
                E, v = loc.energy_potential(den, vext)
                k1 = _kinds(loc)
                Ec, mu, g = loc.closure(chi, o['n_elec'], vext)
                k2 = _kinds(loc)
                Er, vr = ref.energy_potential(den, vext)
                Ecr, mur, gr = ref.energy_grad_chi(chi, o['n_elec'], vext)
                rec = C.measure(o, p, E, v, Ec, mu, g)
                one = dict(dE=max(_rel(E[k], Er[k]) for k in Er), dEc=max(_rel(Ec[k], Ecr[k]) for k in Ecr), dmu=_rel(mu, mur),
                           dv=_field_rel(v, vr), dg=_field_rel(g, gr))
                M._record(shape=shape, P=P, cell=cell, ts=ts, dtype=p, gsplit=gs, kinds=[k1, k2], **rec, **one)
                # the oracle: both criteria and the energy, for either entry point; mu
                _checked(bad, what + ('potential',), v.cpu().numpy(), o['v'], p, what, o['vk'], sum(E.values()), o['E'])
                _checked(bad, what + ('closure',), g.cpu().numpy(), o['g'], p, what, o['gk'], sum(Ec.values()), o['Ec'])
                if not rec['err_mu'] <= sc.MU_TOL[p]:
                    bad.append((what, 'oracle', 'mu', mu, o['mu']))
                # one engine on the same inputs
                tol = SINGLE_TOL[p]
                for key, bound in (('dE', tol['E']), ('dEc', tol['E']), ('dmu', tol['mu']), ('dv', tol['v']), ('dg', tol['g'])):
                    if not one[key] <= bound:
                        bad.append((what, 'single engine', key, one[key], bound))
                # a fused x pass ran on every rank, and not the chirp-z one
                for k in k1 + k2:
                    if not k or k & N.XPASS_CHIRPZ:
                        bad.append((what, 'kinds', k1, k2))
                        break
        finally:
            loc.close()
            ref.close()
    assert not bad, bad


@pytest.mark.parametrize('ts', SERVED)
@pytest.mark.parametrize('shape,P,cell', GEOMETRIES, ids=[_gid(g) for g in GEOMETRIES])
def test_slab_pipeline_matches_the_oracle_and_one_engine(shape, P, cell, ts):
    t0 = time.time()
    try:
        run_case(shape, P, cell, ts)
    finally:
        M._ORACLE.pop((shape, cell, ts), None)          # (no other case uses it)
    M._record(shape=shape, P=P, cell=cell, ts=ts, seconds=time.time() - t0)


def _same(a, b):
    """bitwise equality of two results of LocalRanks.energy_potential / closure"""
    if a[0] != b[0]:
        return False
    return all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a[1:], b[1:]))


def _evaluations(loc, ts, den, vext, chi, n_elec):
    """every served (GGA form, entry point) of a term set, each twice in a row with changed input (the buffers alternate)"""
    out = []
    for gs in (1, 0):
        if ts in M.LAPLACIAN_GGA and gs == 0:
            continue
        _set_split(loc, gs)
        out += [loc.energy_potential(den, vext), loc.energy_potential(den * 1.02, vext),
                loc.closure(chi, n_elec, vext), loc.closure(chi * 1.01, n_elec, vext)]
    return out


@pytest.mark.parametrize('ts', SERVED)
@pytest.mark.parametrize('shape,P,cell,K', CHUNKED, ids=['%s-K%d' % (_gid(g[:3]), g[3]) for g in CHUNKED])
def test_kz_chunked_exchange_is_bitwise_the_unchunked_one_for_every_term_set(shape, P, cell, K, ts):
    names, params, _ = M.TERM_SETS[ts]
    fields = M.inputs(shape, cell)
    box = M.make_cell(shape, cell)
    n_elec = float(np.floor(fields[0].mean() * abs(np.linalg.det(box))) + 0.3)
    for p in ('f64', 'f32'):
        den, vext, chi = _tensors(fields, M.DTYPES[p])
        out = {}
        for k in (1, K):
            loc = LocalRanks(shape, DEV, P, dtype=M.DTYPES[p]).set_cell(torch.as_tensor(box)).set_terms(names, params)
            loc.set_xchg_chunks(k)
            try:
                assert loc.st[0].nchunks == k, (shape, P, k)
                out[k] = _evaluations(loc, ts, den, vext, chi, n_elec)
            finally:
                loc.close()
        assert len(out[1]) == len(out[K]) >= 4
        for i, (a, b) in enumerate(zip(out[K], out[1])):
            assert _same(a, b), (shape, P, K, ts, p, 'evaluation %d' % i)
        assert not _same(out[1][0], out[1][1]) and not _same(out[1][2], out[1][3])      # the second evaluation is another one


# ------------------------------------------------------------------------------------------------------------ refusals
R_SHAPE, R_P, R_CELL, R_TS = (16, 16, 16), 2, 'tri', 'wgc98_lkt_pbe'


class _Small:
    """inputs of the refusal tests and the result of the served term set on fresh contexts (what a context must still give
    after it has refused a call)"""

    def __init__(self):
        fields = M.inputs(R_SHAPE, R_CELL)
        self.box = torch.as_tensor(M.make_cell(R_SHAPE, R_CELL))
        self.n_elec = float(np.floor(fields[0].mean() * abs(np.linalg.det(self.box.numpy()))) + 0.3)
        self.den, self.vext, self.chi = _tensors(fields, torch.double)
        self.names, self.params, _ = M.TERM_SETS[R_TS]
        loc = self.ranks().set_terms(self.names, self.params)
        self.fresh = self.served(loc)
        loc.close()

    def ranks(self):
        return LocalRanks(R_SHAPE, DEV, R_P).set_cell(self.box)

    def served(self, loc):
        return [loc.energy_potential(self.den, self.vext), loc.closure(self.chi, self.n_elec, self.vext)]

    def still_serves(self, loc):
        got = self.served(loc.set_terms(self.names, self.params))
        return all(_same(a, b) for a, b in zip(got, self.fresh))


@pytest.fixture(scope='module')
def small():
    return _Small()


def test_stabilised_wang_teter_is_refused_on_slabs(small):
    names, params, _ = M.TERM_SETS['wts_exp']
    loc = small.ranks().set_terms(names, params)
    try:
        with pytest.raises(RuntimeError, match=REFUSED_WTS):
            loc.closure(small.chi, small.n_elec, small.vext)
        with pytest.raises(RuntimeError, match=REFUSED_WTS):
            loc.energy_potential(small.den, small.vext)
        assert small.still_serves(loc)
    finally:
        loc.close()


def test_tabulated_kernel_term_is_refused_on_slabs(small):
    loc = small.ranks().set_terms(small.names, small.params)
    try:
        with pytest.raises(RuntimeError, match=REFUSED_NLK):
            loc.set_terms(['tf', 'vw', 'nlk'], {'nlk_kind': 2.0})
        # a refused ofdft_set_terms leaves the context as it was: the earlier term set is still the active one
        assert all(_same(a, b) for a, b in zip(small.served(loc), small.fresh))
        assert small.still_serves(loc)
    finally:
        loc.close()


def test_laplacian_gga_with_the_three_component_chain_is_refused_on_slabs(small):
    names, params, _ = M.TERM_SETS['pgslr_h']
    loc = small.ranks().set_terms(names, params)
    try:
        _set_split(loc, 0)
        with pytest.raises(RuntimeError, match=REFUSED_SPLIT0):
            loc.closure(small.chi, small.n_elec, small.vext)
        with pytest.raises(RuntimeError, match=REFUSED_SPLIT0):
            loc.energy_potential(small.den, small.vext)
        _set_split(loc, 1)
        loc.closure(small.chi, small.n_elec, small.vext)          # the same term set, served
        assert small.still_serves(loc)
    finally:
        loc.close()


def test_extents_not_divisible_by_the_rank_count_are_refused_at_create(small):
    for shape in ((18, 16, 16), (16, 18, 16)):
        with pytest.raises(ValueError, match='slab decomposition needs n0 and n1 divisible by the number of ranks'):
            HipStages(shape, DEV, nranks=4, rank=0)          # the host-side plan refuses first ...
        with pytest.raises(RuntimeError, match=REFUSED_DIVISIBLE):
            Engine(shape, DEV, nranks=4, rank=0)             # ... and ofdft_create_dist on its own
    loc = small.ranks()
    try:
        assert small.still_serves(loc)
    finally:
        loc.close()


def test_rows_of_eight_points_are_refused_at_create(small):
    """n2 = 8 would be zero kz blocks and five remainder planes; there is no 8-point row plan (row_extent_ok), so the grid is not
    on the fused path on one GPU and a slab context is refused"""
    shape = (16, 16, 8)
    one = Engine(shape, DEV)
    assert int(one.query(N.Q_FAST_PATH)) == 0
    one.close()
    for rank in (0, 1):
        with pytest.raises(RuntimeError, match=REFUSED_EXTENT):
            Engine(shape, DEV, nranks=2, rank=rank)
    loc = small.ranks()
    try:
        assert small.still_serves(loc)
    finally:
        loc.close()
