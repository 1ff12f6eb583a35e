"""rns_io_recv_batch_pool (batch.recv_batch_pool) on an AF_UNIX SOCK_DGRAM socketpair: the receive
loop of rns_io_recv_batch_chain with the compact outputs.  Every case sends the same datagrams down
two socketpairs and compares the two entries' outputs for the same initial free list."""
import ctypes
import socket

import numpy as np
import pytest

from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import recv_batch_chain, recv_batch_pool

BUF = 512


def payload(i, n):
    return (np.arange(n, dtype=np.uint32) * 7 + i * 13 + 1).astype(np.uint8).tobytes()


def both(msgs, nbuf, permuted, buf=BUF, **kw):
    """Send msgs to both entries over pools of nbuf buffers: (chain result, its pool and free list,
    pool result, its pool and free list, the initial free list)."""
    free0 = (np.random.default_rng(3).permutation(nbuf) if permuted else np.arange(nbuf)).astype(np.uint32)
    out = []
    for recv in (recv_batch_chain, recv_batch_pool):
        a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
        try:
            a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 1 << 20)
            a.setblocking(False)  # a full queue fails the test at once
            for p in msgs:
                a.send(p)
            pool, free = np.full(nbuf * buf, 0xEE, dtype=np.uint8), free0.copy()
            out += [recv(b.fileno(), pool, free, buf_bytes=buf, timeout_ms=1000 if msgs else 20, **kw), pool, free]
        finally:
            a.close()
            b.close()
    return (*out, free0)


def agree(res, kept, buf=BUF):
    """The four equalities, and the kept datagrams' bytes."""
    (n, off, ln, first, nf), pool_c, free_c, (n2, len16, blk, nf2), pool_p, free_p, free0 = res
    assert n2 == n == len(kept) and nf2 == nf
    assert np.array_equal(free_p, free_c)                                     # h_free permuted identically
    assert sorted(free_p.tolist()) == sorted(free0.tolist())
    assert len16.dtype == np.uint16 and len16.shape == (n,)
    sums = np.add.reduceat(ln.astype(np.int64), first[:-1].astype(np.int64)) if n else np.zeros(0, np.int64)
    assert np.array_equal(len16.astype(np.int64), sums)                       # per-datagram sums of frag_len
    assert np.array_equal(blk, first[:-1:64])                                 # blk_first[b] == first[64 * b]
    assert np.array_equal(pool_p, pool_c)                                     # the pool bytes
    assert [int(x) for x in len16] == [len(p) for p in kept]
    rows = pool_p.reshape(-1, buf)
    for i, p in enumerate(kept):
        idx = free_p[int(first[i]):int(first[i + 1])]
        assert rows[idx].tobytes()[:len(p)] == p, i


@pytest.mark.parametrize("permuted", [False, True])
def test_same_outputs_as_the_chain_entry(permuted):
    sent = [payload(i, s) for i, s in enumerate([1, 511, 512, 513, 1500, 2048])]
    sent += [payload(i, 1 + (i * 37) % 700) for i in range(130)]  # more than two recvmmsg rounds, three blocks
    res = both(sent, 4 * len(sent) + 8, permuted)
    agree(res, sent)
    assert res[3][2].shape == (3,)


@pytest.mark.parametrize("permuted", [False, True])
def test_oversize_dropped_and_empty_skipped(permuted):
    msgs = [payload(0, 700), payload(1, 2049), b"", payload(2, 2048), payload(3, 4000), b"", b"", payload(4, 5)]
    res = both(msgs, 40, permuted, mru=2048)
    agree(res, [msgs[0], msgs[3], msgs[7]])
    assert res[3][3] == 2 + 4 + 1


@pytest.mark.parametrize("permuted", [False, True])
def test_free_list_and_max_pkts_caps(permuted):
    sent = [payload(i, 100) for i in range(5)]
    agree(both(sent, 6, permuted), sent[:3])  # each is offered 4 buffers and keeps 1: 6 -> 5 -> 4 -> 3 free
    agree(both(sent, 64, permuted, max_pkts=4), sent[:4])
    agree(both(sent, 3, permuted), [])        # fewer free buffers than one datagram is offered


def test_other_buffer_sizes_and_timeout():
    sent = [payload(i, s) for i, s in enumerate([63, 64, 65, 200, 512])]
    agree(both(sent, 64, True, buf=64, mru=512), sent, buf=64)
    agree(both(sent, 8, True, buf=2048), sent, buf=2048)
    res = both([], 8, True)
    agree(res, [])
    assert res[3][1].size == res[3][2].size == 0 and np.array_equal(res[5], res[6])


def test_rejects():
    lib = _lib.load()
    pool = np.zeros(16 * BUF, dtype=np.uint8)
    free = np.arange(16, dtype=np.uint32)
    with pytest.raises(ValueError):
        recv_batch_pool(0, pool, free, buf_bytes=512, mru=512 * _lib.RNS_IO_MAX_FRAGS + 1)
    with pytest.raises(ValueError):
        recv_batch_pool(0, pool, free, buf_bytes=500)
    with pytest.raises(ValueError):
        recv_batch_pool(0, pool, free, buf_bytes=32768, mru=65536)
    with pytest.raises(ValueError):
        recv_batch_pool(0, pool, free.astype(np.int64))
    with pytest.raises(ValueError):
        recv_batch_pool(0, pool, np.array([16], dtype=np.uint32))
    len16 = np.zeros(16, np.uint16)
    blk = np.zeros(1, np.uint32)
    nf = ctypes.c_uint32()
    args = (pool.ctypes.data, 9, free.ctypes.data, 16)
    outs = (len16.ctypes.data, blk.ctypes.data, ctypes.byref(nf), 0)
    call = lib.rns_io_recv_batch_pool
    assert call(0, *args, 512 * _lib.RNS_IO_MAX_FRAGS + 1, 4, *outs) == _lib.RNS_E_INVALID  # ceil(mru / buf) > 8
    assert call(0, pool.ctypes.data, 6, free.ctypes.data, 16, 64 * 8 + 1, 4, *outs) == _lib.RNS_E_INVALID
    assert call(0, pool.ctypes.data, 15, free.ctypes.data, 16, 65536, 4, *outs) == _lib.RNS_E_INVALID  # mru > 65535
    for log2 in (5, 16):
        assert call(0, pool.ctypes.data, log2, free.ctypes.data, 16, 32, 4, *outs) == _lib.RNS_E_INVALID
    assert call(-1, *args, 2048, 4, *outs) == _lib.RNS_E_INVALID
    assert call(0, None, 9, free.ctypes.data, 16, 2048, 4, *outs) == _lib.RNS_E_INVALID
    assert call(0, *args, 2048, 0, *outs) == _lib.RNS_E_INVALID
    assert call(0, *args, 0, 4, *outs) == _lib.RNS_E_INVALID
    assert call(0, *args, 2048, 4, None, blk.ctypes.data, ctypes.byref(nf), 0) == _lib.RNS_E_INVALID
    assert call(0, *args, 2048, 4, len16.ctypes.data, None, ctypes.byref(nf), 0) == _lib.RNS_E_INVALID
    assert call(0, *args, 2048, 4, len16.ctypes.data, blk.ctypes.data, None, 0) == _lib.RNS_E_INVALID
