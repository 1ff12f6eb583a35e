"""rns_io_recv_batch_chain (batch.recv_batch_chain) on an AF_UNIX SOCK_DGRAM socketpair: the
batched recv_packet (netif.rs:65-83: new_prealloc(MRU), readv, trim_tail) into pool buffers."""
import os
import socket

import numpy as np
import pytest

from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import recv_batch_chain

BUF = 512


@pytest.fixture
def pair():
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 1 << 20)
    a.setblocking(False)  # a full queue fails the test at once
    yield a, b
    a.close()
    b.close()


def payload(i, n):
    return (np.arange(n, dtype=np.uint32) * 7 + i * 13 + 1).astype(np.uint8).tobytes()


def make_pool(nbuf, seed=3):
    pool = np.full(nbuf * BUF, 0xEE, dtype=np.uint8)
    free = np.random.default_rng(seed).permutation(nbuf).astype(np.uint32)  # a pool that has been in use
    return pool, free


def check(pool, free0, free, res, sent, buf=BUF):
    """The chains hold exactly `sent`, the CSR is right and free is permuted as specified."""
    n, off, ln, first, nf = res
    assert n == len(sent) and first.shape == (n + 1,) and first[0] == 0 and int(first[-1]) == nf
    assert off.shape == ln.shape == (nf,)
    for i, p in enumerate(sent):
        f0, f1 = int(first[i]), int(first[i + 1])
        assert f1 - f0 == -(-len(p) // buf)
        assert [int(x) for x in ln[f0:f1]] == [buf] * (f1 - f0 - 1) + [len(p) - (f1 - f0 - 1) * buf]
        got = b"".join(pool[int(o):int(o) + int(k)].tobytes() for o, k in zip(off[f0:f1], ln[f0:f1]))
        assert got == p, i
    assert np.array_equal(off, free[:nf].astype(np.uint64) * np.uint64(buf))  # in use, in fragment order
    assert sorted(free.tolist()) == sorted(free0.tolist())                     # a permutation
    assert len(set(free[:nf].tolist())) == nf


def test_sizes_become_chains(pair):
    a, b = pair
    sizes = [1, 511, 512, 513, 1500, 2048]
    sent = [payload(i, s) for i, s in enumerate(sizes)]
    for p in sent:
        a.send(p)
    pool, free = make_pool(64)
    free0 = free.copy()
    res = recv_batch_chain(b.fileno(), pool, free, timeout_ms=1000)
    check(pool, free0, free, res, sent)
    assert np.diff(res[3].astype(np.int64)).tolist() == [1, 1, 1, 2, 3, 4]
    # what is still free is exactly the set of unused buffers
    used = set(free[:res[4]].tolist())
    assert set(free[res[4]:].tolist()) == set(free0.tolist()) - used


def test_many_rounds(pair):
    a, b = pair
    sent = [payload(i, 1 + (i * 37) % 700) for i in range(130)]  # more than two recvmmsg rounds of 64
    for p in sent:
        a.send(p)
    pool, free = make_pool(4 * 130 + 8)
    free0 = free.copy()
    res = recv_batch_chain(b.fileno(), pool, free, timeout_ms=1000)
    check(pool, free0, free, res, sent)


def test_empty_datagram_loses_nothing(pair):
    a, b = pair
    msgs = [payload(0, 100), b"", payload(1, 600), b"", b"", payload(2, 33)]
    for p in msgs:
        a.send(p)
    pool, free = make_pool(32)
    free0 = free.copy()
    res = recv_batch_chain(b.fileno(), pool, free, timeout_ms=1000)
    check(pool, free0, free, res, [p for p in msgs if p])


def test_oversize_is_dropped_and_takes_no_buffer(pair):
    a, b = pair
    msgs = [payload(0, 700), payload(1, 2049), payload(2, 2048), payload(3, 4000), payload(4, 5)]
    for p in msgs:
        a.send(p)
    pool, free = make_pool(40)
    free0 = free.copy()
    res = recv_batch_chain(b.fileno(), pool, free, mru=2048, timeout_ms=1000)
    check(pool, free0, free, res, [msgs[0], msgs[2], msgs[4]])
    assert res[4] == 2 + 4 + 1


def test_mru_that_is_no_multiple_of_the_buffer(pair):
    a, b = pair
    msgs = [payload(0, 1000), payload(1, 1001), payload(2, 999)]
    for p in msgs:
        a.send(p)
    pool, free = make_pool(16)
    free0 = free.copy()
    res = recv_batch_chain(b.fileno(), pool, free, mru=1000, timeout_ms=1000)
    check(pool, free0, free, res, [msgs[0], msgs[2]])


def test_stops_when_the_free_list_cannot_hold_another(pair):
    a, b = pair
    sent = [payload(i, 100) for i in range(5)]
    for p in sent:
        a.send(p)
    pool, free = make_pool(6)  # each datagram is offered 4 buffers and keeps 1: 6 -> 5 -> 4 -> 3 free
    free0 = free.copy()
    res = recv_batch_chain(b.fileno(), pool, free, timeout_ms=1000)
    check(pool, free0, free, res, sent[:3])
    free2 = np.ascontiguousarray(free[res[4]:])  # the rest of the free list cannot hold a datagram
    assert recv_batch_chain(b.fileno(), pool, free2, timeout_ms=0)[0] == 0
    pool3, free3 = make_pool(8)
    f30 = free3.copy()
    check(pool3, f30, free3, recv_batch_chain(b.fileno(), pool3, free3, timeout_ms=1000), sent[3:])


def test_max_pkts(pair):
    a, b = pair
    sent = [payload(i, 50 + i) for i in range(10)]
    for p in sent:
        a.send(p)
    pool, free = make_pool(64)
    free0 = free.copy()
    check(pool, free0, free, recv_batch_chain(b.fileno(), pool, free, max_pkts=4, timeout_ms=1000), sent[:4])


def test_timeout_returns_zero(pair):
    _, b = pair
    pool, free = make_pool(8)
    free0 = free.copy()
    n, off, ln, first, nf = recv_batch_chain(b.fileno(), pool, free, timeout_ms=20)
    assert (n, nf) == (0, 0) and first.tolist() == [0] and off.size == ln.size == 0
    assert np.array_equal(free, free0)


def test_packet_pipe_takes_the_readv_path():
    """A descriptor that is no socket (here a packet-mode pipe, as a TUN fd: one datagram per
    read): one readv per datagram, mru + 1 bytes offered so that a longer one shows."""
    r, w = os.pipe2(os.O_DIRECT)
    try:
        msgs = [payload(0, 513), payload(1, 2049), payload(2, 2048), payload(3, 1)]
        for p in msgs:
            os.write(w, p)
        pool, free = make_pool(24)
        free0 = free.copy()
        res = recv_batch_chain(r, pool, free, timeout_ms=1000)
        check(pool, free0, free, res, [msgs[0], msgs[2], msgs[3]])
    finally:
        os.close(r)
        os.close(w)


def test_rejects():
    lib = _lib.load()
    pool, free = make_pool(16)
    with pytest.raises(ValueError):
        recv_batch_chain(0, pool, free, buf_bytes=512, mru=512 * _lib.RNS_IO_MAX_FRAGS + 1)
    with pytest.raises(ValueError):
        recv_batch_chain(0, pool, free.astype(np.int64))
    with pytest.raises(ValueError):
        recv_batch_chain(0, pool, np.array([16], dtype=np.uint32))
    off = np.zeros(16, np.uint64)
    ln = np.zeros(16, np.uint32)
    first = np.zeros(5, np.uint32)
    import ctypes
    nf = ctypes.c_uint32()
    args = (pool.ctypes.data, 512, free.ctypes.data, 16)
    outs = (off.ctypes.data, ln.ctypes.data, first.ctypes.data, ctypes.byref(nf), 0)
    assert lib.rns_io_recv_batch_chain(0, *args, 512 * 8 + 1, 4, *outs) == _lib.RNS_E_INVALID
    assert lib.rns_io_recv_batch_chain(-1, *args, 2048, 4, *outs) == _lib.RNS_E_INVALID
    assert lib.rns_io_recv_batch_chain(0, None, 512, free.ctypes.data, 16, 2048, 4, *outs) == _lib.RNS_E_INVALID
    assert lib.rns_io_recv_batch_chain(0, *args, 2048, 0, *outs) == _lib.RNS_E_INVALID
    assert lib.rns_io_recv_batch_chain(0, *args, 0, 4, *outs) == _lib.RNS_E_INVALID
