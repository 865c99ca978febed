"""The collectives of the ranks emulated in one process (tests/local_ranks.py: ThreadCollectives) on numpy buffers: the
barrier-and-copy logic the slab geometry-step tests (tests/test_slab_geometry_step_gpu.py) rely on, without a GPU.

A "C call" here is a Python function that makes collective calls and raises when one of them returns non-zero, as
Engine._check does for an entry point whose callback failed."""
import functools
import threading
import time

import numpy as np
import pytest

from local_ranks import ThreadCollectives

RANKS = (2, 4, 8)
TIMEOUT = 20.0          # of the barrier; the failure cases must return far inside it
PROMPT = 5.0


def _copy(recv, roff, send, soff, n):
    recv[roff:roff + n] = send[soff:soff + n]


def _ok(rc):
    if rc:
        raise RuntimeError('callback failed (%d)' % rc)


def _send(p, P, nbytes):
    """rank p's send buffer: chunk r carries (p, r) in every byte pair"""
    return np.concatenate([np.resize(np.array([17 * p + 1, 29 * r + 3, p ^ r], dtype=np.uint8), nbytes) for r in range(P)])


@pytest.mark.parametrize('P', RANKS)
def test_all_to_all_is_the_block_transpose(P):
    nbytes, rounds = 48, 3
    synced = []
    coll = ThreadCollectives(P, _copy, sync=lambda stream: synced.append(stream), timeout=TIMEOUT)
    send = [[_send(p, P, nbytes) + k for p in range(P)] for k in range(rounds)]
    recv = [[np.zeros(P * nbytes, dtype=np.uint8) for _ in range(P)] for _ in range(rounds)]

    def rank(r):
        for k in range(rounds):          # several exchanges in one call, as ofdft_stress makes them
            _ok(coll.all_to_all(r, send[k][r], recv[k][r], nbytes, stream=100 + r))
        return r

    assert coll.run(rank) == list(range(P))
    for k in range(rounds):
        for r in range(P):
            for p in range(P):
                want = send[k][p][r * nbytes:(r + 1) * nbytes]
                assert np.array_equal(recv[k][r][p * nbytes:(p + 1) * nbytes], want), (k, r, p)
    assert coll.calls == [rounds, 0]
    assert sorted(set(synced)) == [100 + r for r in range(P)] and len(synced) == 2 * rounds * P


@pytest.mark.parametrize('P', RANKS)
def test_all_reduce_is_bitwise_the_rank_ordered_sum_on_every_rank(P):
    rng = np.random.default_rng(40 + P)
    vecs = [rng.standard_normal(7) * 10.0 ** rng.integers(-15, 15, 7) for _ in range(P)]
    for p, x in enumerate(([1e16, 1.0, -1e16] + [1.0] * P)[:P]):          # a column whose sum depends on the order of its terms
        vecs[p][0] = x
    want = functools.reduce(lambda a, b: a + b, vecs)
    other = functools.reduce(lambda a, b: a + b, vecs[::-1])
    assert P == 2 or want[0] != other[0]          # (two terms commute; from three on the data tell the orders apart)
    coll = ThreadCollectives(P, _copy, timeout=TIMEOUT)

    def rank(r):
        v = vecs[r].copy()
        _ok(coll.all_reduce(r, v))
        w = v.copy()
        _ok(coll.all_reduce(r, w))                  # a second one right behind it: the published vectors are not reused early
        return v, w

    out = coll.run(rank)
    for r in range(P):
        assert np.array_equal(out[r][0], want), r
        assert np.array_equal(out[r][1], functools.reduce(lambda a, b: a + b, [want] * P)), r
    assert coll.calls == [0, 2]


@pytest.mark.parametrize('P', RANKS)
def test_mismatched_nbytes_is_reported_and_nothing_is_copied(P):
    coll = ThreadCollectives(P, _copy, timeout=TIMEOUT)
    recv = [np.zeros(P * 16, dtype=np.uint8) for _ in range(P)]

    def rank(r):
        _ok(coll.all_to_all(r, np.ones(P * 16, dtype=np.uint8), recv[r], 8 if r == P - 1 else 16))

    t0 = time.monotonic()
    with pytest.raises(ValueError, match='different nbytes'):
        coll.run(rank)
    assert time.monotonic() - t0 < PROMPT
    assert all(isinstance(e, RuntimeError) for e in coll.rank_errors)          # every rank's call failed
    assert not any(r.any() for r in recv)

    def rank2(r):          # mismatched counts of an all-reduce likewise
        _ok(coll.all_reduce(r, np.ones(3 if r == 0 else 4)))

    with pytest.raises(ValueError, match='different counts'):
        coll.run(rank2)


class _Refused(Exception):
    pass


@pytest.mark.parametrize('peers_wait', (False, True), ids=['at-once', 'peers-waiting'])
@pytest.mark.parametrize('P', RANKS)
def test_a_rank_that_raises_before_its_first_collective_fails_the_others_promptly(P, peers_wait):
    coll = ThreadCollectives(P, _copy, timeout=TIMEOUT)
    bad = P - 1

    def rank(r):
        if r == bad:
            end = time.monotonic() + PROMPT
            while peers_wait and coll.barrier.n_waiting < P - 1 and time.monotonic() < end:
                pass          # until the peers are inside the barrier (else they find it broken on arrival)
            raise _Refused('rank %d' % r)
        v = np.ones(4)
        _ok(coll.all_reduce(r, v))
        return v

    t0 = time.monotonic()
    with pytest.raises(_Refused, match='rank %d' % bad):
        coll.run(rank)
    assert time.monotonic() - t0 < PROMPT < TIMEOUT
    for r in range(P):
        if r != bad:          # the follow-up failures: a broken barrier inside the callback, "callback failed" from the call
            assert isinstance(coll.cb_error[r], threading.BrokenBarrierError), r
            assert isinstance(coll.rank_errors[r], RuntimeError), r
    assert coll.cb_error[bad] is None


@pytest.mark.parametrize('P', RANKS)
def test_every_rank_refusing_gives_every_rank_its_own_error_and_the_object_serves_again(P):
    coll = ThreadCollectives(P, _copy, timeout=TIMEOUT)

    def refuse(r):
        raise _Refused('rank %d' % r)

    t0 = time.monotonic()
    with pytest.raises(_Refused, match='rank 0'):
        coll.run(refuse)
    assert time.monotonic() - t0 < PROMPT
    assert [str(e) for e in coll.rank_errors] == ['rank %d' % r for r in range(P)]

    def rank(r):          # a new run starts from a whole barrier
        v = np.full(2, float(r))
        _ok(coll.all_reduce(r, v))
        return v

    assert all(np.array_equal(v, np.full(2, P * (P - 1) / 2.0)) for v in coll.run(rank))
