"""P ranks of the slab decomposition emulated in ONE process on one GPU (test / diagnostics only).

Every rank is its own `ofdft_ctx` (created with nranks=P, rank=r); the all-to-all of each stage is done by copying
peer chunks between the contexts' exchange buffers, the all-reduces by summing on the host.  This runs the very
kernels, pack / un-pack geometry and stage sequence an 8-GPU job runs, at rank counts a one-GPU box cannot host
as processes.

The per-geometry-step routines (ofdft_stress, ofdft_ionic_potential, ofdft_ion_electron_forces, ofdft_ion_electron_stress)
make several collective calls inside ONE C call, so the P contexts cannot be stepped from one thread the way `_stages` steps
the hot path.  They run on P threads, one per context (ctypes releases the GIL during the C call, the callbacks take it
again), with the callbacks of ofdft_set_collectives built on a shared barrier: `ThreadCollectives`, which knows nothing of
torch (the copy and the stream synchronisation are handed in) and is tested on numpy buffers in
tests/test_local_collectives_cpu.py.
"""
import threading
import time

import numpy as np
import torch

from professad_amd import _native as N
from professad_amd.distributed import HipStages, _RawDeviceBuffer


class ThreadCollectives:
    """Equal-split all-to-all and all-reduce (sum) between P threads of one process.

    copy(recv, recv_offset, send, send_offset, nbytes) moves bytes between two published buffers (whatever handles the
    ranks pass to `all_to_all`); sync(stream) waits for the stream a callback was given.  `all_to_all` and `all_reduce` are
    what the C callbacks return: 0, or 1 after any failure -- nothing is raised, the exception is kept in `cb_error[rank]`.
    No failure becomes a hang: a rank that fails aborts the barrier, a broken barrier fails every waiting callback, and
    every wait is bounded by `timeout`."""

    def __init__(self, nranks, copy, sync=None, timeout=60.0):
        self.P = int(nranks)
        self.copy = copy
        self.sync = sync if sync is not None else (lambda stream: None)
        self.timeout = float(timeout)
        self.barrier = threading.Barrier(self.P, timeout=self.timeout)
        self._xchg = [None] * self.P          # published (send, recv, nbytes) of the all-to-all in flight
        self._vec = [None] * self.P           # published host vectors of the all-reduce in flight
        self.cb_error = [None] * self.P       # first exception inside a callback, per rank
        self.rank_errors = [None] * self.P    # what each rank's function raised in the last `run`
        self.calls = [0, 0]                   # all-to-alls and all-reduces completed (counted by rank 0)

    def _failed(self, rank, e):
        if self.cb_error[rank] is None:
            self.cb_error[rank] = e
        self.barrier.abort()
        return 1

    def all_to_all(self, rank, send, recv, nbytes, stream=None):
        """chunk p of `recv` <- chunk `rank` of rank p's `send`, chunks of `nbytes` bytes"""
        try:
            P, nbytes = self.P, int(nbytes)
            self._xchg[rank] = (send, recv, nbytes)
            self.sync(stream)                         # what this rank wrote into its send buffer is complete
            self.barrier.wait()
            sizes = [x[2] for x in self._xchg]        # (every rank sees the same list: all of them fail, or none)
            if any(n != nbytes for n in sizes):
                raise ValueError('all-to-all: the ranks passed different nbytes %r' % (sizes,))
            for p in range(P):
                self.copy(recv, p * nbytes, self._xchg[p][0], rank * nbytes, nbytes)
            self.sync(stream)
            self.barrier.wait()                       # nobody's send buffer is reused before every peer has read it
            if rank == 0:
                self.calls[0] += 1
            return 0
        except BaseException as e:  # noqa: BLE001  (nothing may propagate across the C ABI)
            return self._failed(rank, e)

    def all_reduce(self, rank, vec):
        """in-place sum over the ranks of a 1-D float64 host vector, added in rank order on every rank (deterministic, and
        bitwise the same everywhere)"""
        try:
            self._vec[rank] = np.array(vec, dtype=np.float64, copy=True)
            self.barrier.wait()
            if any(v.shape != self._vec[rank].shape for v in self._vec):
                raise ValueError('all-reduce: the ranks passed different counts %r' % ([v.shape for v in self._vec],))
            acc = self._vec[0].copy()
            for p in range(1, self.P):
                acc += self._vec[p]
            vec[:] = acc
            self.barrier.wait()                       # the published vectors are replaced only after everybody has summed
            if rank == 0:
                self.calls[1] += 1
            return 0
        except BaseException as e:  # noqa: BLE001
            return self._failed(rank, e)

    def run(self, fn, join_timeout=None):
        """fn(rank) on P threads -> [fn(0), ..., fn(P - 1)].  If a rank raised, the first rank's OWN error is raised here
        (an exception inside its callback, else what its function raised) in preference to the BrokenBarrierError the others
        then meet; `rank_errors` keeps what every rank raised."""
        P = self.P
        self.barrier = threading.Barrier(P, timeout=self.timeout)
        self.cb_error = [None] * P
        out, exc = [None] * P, [None] * P

        def work(r):
            try:
                out[r] = fn(r)
            except BaseException as e:  # noqa: BLE001
                exc[r] = e
                self.barrier.abort()          # the peers must not wait for a rank that is gone

        threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
        for t in threads:
            t.start()
        deadline = time.monotonic() + (self.timeout + 10.0 if join_timeout is None else join_timeout)
        for t in threads:
            t.join(max(0.0, deadline - time.monotonic()))
        self.rank_errors = exc
        stuck = [r for r, t in enumerate(threads) if t.is_alive()]
        if stuck:
            self.barrier.abort()
            raise RuntimeError('ranks %r did not return' % (stuck,))
        broken = threading.BrokenBarrierError
        follow = None
        for r in range(P):
            if exc[r] is None:
                continue
            cb = self.cb_error[r]
            if cb is not None and not isinstance(cb, broken):
                raise cb from exc[r]
            if cb is None and not isinstance(exc[r], broken):
                raise exc[r]
            if follow is None:
                follow = exc[r]
        if follow is not None:
            raise follow
        return out


def _identical(a, b):
    """bitwise equality of two host results (dicts / lists of arrays, arrays, floats)"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_identical(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_identical(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


class LocalRanks:
    def __init__(self, shape, device, nranks, dtype=torch.double):
        self.P = nranks
        self.dev = device
        self.st = [HipStages(shape, device, nranks=nranks, rank=r, dtype=dtype) for r in range(nranks)]
        self.npts = int(np.prod(shape))
        self.compute_s = [0.0] * nranks
        self.exchanged_bytes = 0          # bytes in all ranks' send buffers (incl. the diagonal chunks)
        self.coll = None                  # ThreadCollectives of the geometry-step routines (set up at their first use)

    def set_cell(self, box):
        for s in self.st:
            s.set_cell(box)
        self.box = np.asarray(torch.as_tensor(box).cpu().numpy(), dtype=np.float64).reshape(3, 3)
        self.vol = float(abs(np.linalg.det(self.box)))
        return self

    def set_terms(self, names, params=None):
        for s in self.st:
            s.set_terms(names, params)
        return self

    def _timed(self, r, fn, *a):
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        out = fn(*a)
        torch.cuda.synchronize(self.dev)
        self.compute_s[r] += time.perf_counter() - t0
        return out

    def set_xchg_chunks(self, n):
        for s in self.st:
            s.set_xchg_chunks(n)
        return self

    legacy_stage_api = False      # True: sequence with ofdft_dist_stage (whole stages; one chunk only) instead of ofdft_dist_step

    def advance(self, how, *where):
        """`how` = 'step' (step, chain, chunk) or 'stage' (stage, chain) on every rank, then the equal-split all-to-all over the
        region the ranks returned (nothing when nothing crosses)"""
        P = self.P
        ex = [self._timed(r, getattr(s, how), *where) for r, s in enumerate(self.st)]
        if ex[0] is None:
            return
        self.exchanged_bytes += sum(e[0].numel() for e in ex)
        for r in range(P):
            rc = ex[r][1].chunk(P)
            for p in range(P):
                rc[p].copy_(ex[p][0].chunk(P)[r])

    def finish(self):
        return sum(self._timed(r, s.finish) for r, s in enumerate(self.st))

    def _stages(self):
        if self.legacy_stage_api:
            calls = [('stage', k, chain) for k in (1, 2, 3, 4) for chain in (0, 1)]
        else:              # chunk k of the exchange: one equal-split all-to-all over the chunk's region
            calls = [('step', step, chain, k) for step in (1, 2, 3, 4, 5, 6) for chain in (0, 1) for k in range(self.st[0].nchunks)]
        for call in calls:
            self.advance(*call)
        return self.finish()

    def closure(self, chi, n_elec, vext, sequence=None):
        """full-grid chi / v_ext (device tensors) -> (E_terms, mu, full-grid dE/dchi); `sequence`: what runs between the ranks'
        begin and the energies in place of `_stages` (calls of `advance`, then `finish`, whose sums it returns)"""
        sl = [s.plan.x_range() for s in self.st]
        chis = [chi[x].contiguous() for x in sl]
        vexts = [vext[x].contiguous() if vext is not None else None for x in sl]
        s2 = sum(self._timed(r, s.sumsq, chis[r], True) for r, s in enumerate(self.st))
        cscale = n_elec / (s2 / self.npts * self.vol)
        vs = [torch.empty_like(c) for c in chis]
        for r, s in enumerate(self.st):
            self._timed(r, s.begin, chis[r], True, cscale, n_elec, vexts[r], vs[r])
        gs = (sequence or self._stages)()
        out = []
        for r, s in enumerate(self.st):
            E, vn = s.energies(gs)
            mu = vn / n_elec
            out.append(self._timed(r, s.chi_grad, chis[r], vs[r], cscale, mu))
        return E, mu, torch.cat(out)

    def energy_potential(self, den, vext):
        """full-grid density / v_ext (device tensors) -> (E_terms, full-grid dE/dn): the sequence of
        professad_amd.distributed.run_potential (density in, N_e from the ranks' summed densities)"""
        sl = [s.plan.x_range() for s in self.st]
        dens = [den[x].contiguous() for x in sl]
        vexts = [vext[x].contiguous() if vext is not None else None for x in sl]
        nsum = sum(self._timed(r, s.sumsq, dens[r], False) for r, s in enumerate(self.st))
        nel = nsum / self.npts * self.vol
        vs = [torch.empty_like(d) for d in dens]
        for r, s in enumerate(self.st):
            self._timed(r, s.begin, dens[r], False, 1.0, nel, vexts[r], vs[r])
        gs = self._stages()
        for s in self.st:
            E, _ = s.energies(gs)
        return E, torch.cat(vs)

    # ---- the per-geometry-step routines: one thread per context, collectives through ThreadCollectives
    COLLECTIVE_TIMEOUT = 60.0

    def _collectives(self):
        if self.coll is not None:
            return self.coll
        P, dev, views = self.P, self.dev, {}

        def view(ptr, tot):          # engine-owned device memory as a flat uint8 tensor (as HipStages.enable_collectives)
            v = views.get((ptr, tot))
            if v is None:
                v = views[(ptr, tot)] = torch.as_tensor(_RawDeviceBuffer(ptr, tot), device=dev)
            return v

        def copy(recv, roff, send, soff, n):
            view(recv, P * n)[roff:roff + n].copy_(view(send, P * n)[soff:soff + n])

        def sync(stream):
            # the callback runs on the thread that made the engine call, whose current torch stream is the one that call was given
            cur = torch.cuda.current_stream(dev)
            if int(stream or 0) != int(cur.cuda_stream):
                raise RuntimeError('the all-to-all callback was given a stream that is not the calling thread\'s current one')
            cur.synchronize()

        coll = ThreadCollectives(P, copy, sync, timeout=self.COLLECTIVE_TIMEOUT)
        for r, s in enumerate(self.st):
            def a2a(user, send, recv, nbytes, stream, r=r):
                return coll.all_to_all(r, int(send or 0), int(recv or 0), int(nbytes), stream)

            def allreduce(user, buf, count, r=r):
                return coll.all_reduce(r, np.ctypeslib.as_array(buf, shape=(int(count),)))

            s._callbacks = (N.A2A_FN(a2a), N.ALLREDUCE_FN(allreduce))          # (kept alive as long as the context)
            s._check(s.lib.ofdft_set_collectives(s._ctx, s._callbacks[0], s._callbacks[1], None), 'ofdft_set_collectives')
        self.coll = coll
        return coll

    def _on_ranks(self, fn, same=True):
        """fn(rank, context) on every rank's own thread -> the list of results; with `same`, all ranks must have returned
        bitwise identical host results, and that one result is returned"""
        coll = self._collectives()

        def work(r):
            with torch.cuda.device(self.dev):
                return fn(r, self.st[r])

        out = coll.run(work)
        if not same:
            return out
        for r in range(1, self.P):
            assert _identical(out[0], out[r]), ('rank %d returned another result than rank 0' % r, out[0], out[r])
        return out[0]

    def _slabs(self, full):
        return [full[s.plan.x_range()].contiguous() for s in self.st]

    def stress(self, den):
        """full-grid density -> per-term stress of the full system (Engine.stress on every rank's slab)"""
        dens = self._slabs(den)
        return self._on_ranks(lambda r, s: s.stress(dens[r]))

    def ionic_potential(self, species, order=None):
        """-> full-grid v_ext of the ions (each rank builds its x-slab)"""
        from professad_amd.ions import ionic_potential
        return torch.cat(self._on_ranks(lambda r, s: ionic_potential(s, self.box, species, pme_order=order), same=False))

    def ion_electron_forces(self, den, species, order=None):
        from professad_amd.ions import ion_electron_forces
        dens = self._slabs(den)
        return self._on_ranks(lambda r, s: ion_electron_forces(s, self.box, dens[r], species, pme_order=order))

    def ion_electron_stress(self, den, species, order=None):
        from professad_amd.ions import ion_electron_stress
        dens = self._slabs(den)
        return self._on_ranks(lambda r, s: ion_electron_stress(s, self.box, dens[r], species, pme_order=order))

    def close(self):
        for s in self.st:
            s.close()
