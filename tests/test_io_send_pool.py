"""rns_io_send_batch_pool (batch.send_batch_pool) on an AF_UNIX SOCK_DGRAM socketpair: every
datagram leaves as one message gathered from its head bytes (the end of its head buffer) and its
payload buffers."""
import socket

import numpy as np
import pytest

from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import send_batch_pool
from test_gpu_tx import outgoing
from test_gpu_tx_chain_packed import cut
from tx_pool_helper import lay_pool

BUF = 512


def send_and_drain(pool, idx, blk, hl, pl, buf=BUF, expect=None):
    """Send the batch; returns (the call's result or the ChecksumError status, what arrived)."""
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    try:
        a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 4 << 20)
        b.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 4 << 20)
        a.setblocking(False)  # a full queue fails the test at once
        b.setblocking(False)
        try:
            r = send_batch_pool(a.fileno(), pool, idx, blk, hl, pl, buf)
        except _lib.ChecksumError as e:
            r = e.status
        got = []
        while True:
            try:
                got.append(b.recv(70000))
            except BlockingIOError:
                break
        return r, got
    finally:
        a.close()
        b.close()


def test_datagrams_arrive_whole():
    """About 150 datagrams of every kind, more than two sendmmsg rounds and three blocks."""
    pkts = [p for p in outgoing(170, 0x5E2D) if p][:150]
    heads, pays = cut(pkts)
    keep = [i for i in range(len(pkts)) if heads[i] and 1 + -(-len(pays[i]) // BUF) <= _lib.RNS_IO_MAX_FRAGS]
    heads, pays = [heads[i] for i in keep], [pays[i] for i in keep]
    assert len(heads) >= 140 and any(len(p) > 2 * BUF for p in pays) and any(len(p) == 0 for p in pays)
    pool, idx, blk, hl, pl, _ = lay_pool(heads, pays, BUF, shuffled=True, seed=11)
    r, got = send_and_drain(pool, idx, blk, hl, pl)
    assert r == len(heads)
    assert got == [h + p for h, p in zip(heads, pays)]


def test_head_only_and_other_buffer_sizes():
    heads = [bytes(range(40)), bytes(range(1, 29)), bytes(range(100))]
    pays = [b"", bytes(range(200)) * 3, b"x"]
    for buf in (256, 2048):
        pool, idx, blk, hl, pl, _ = lay_pool(heads, pays, buf, shuffled=True, seed=buf)
        r, got = send_and_drain(pool, idx, blk, hl, pl, buf)
        assert r == 3 and got == [h + p for h, p in zip(heads, pays)]
    pool, idx, blk, hl, pl, _ = lay_pool(heads[:1], pays[:1], BUF)
    assert send_and_drain(pool, idx, blk, hl, pl) == (1, [heads[0]])     # a head-only datagram is sent


def test_too_many_fragments_sends_nothing():
    heads = [bytes(range(40))] * 3
    pays = [b"a" * 100, b"b" * (7 * BUF + 1), b"c" * 100]               # 1 + 8 = 9 fragments
    pool, idx, blk, hl, pl, _ = lay_pool(heads, pays, BUF)
    assert send_and_drain(pool, idx, blk, hl, pl) == (_lib.RNS_E_INVALID, [])
    pays[1] = b"b" * (7 * BUF)                                          # 8 fragments go out
    pool, idx, blk, hl, pl, _ = lay_pool(heads, pays, BUF)
    r, got = send_and_drain(pool, idx, blk, hl, pl)
    assert r == 3 and got == [h + p for h, p in zip(heads, pays)]


def test_empty_head_and_bad_arguments():
    heads = [bytes(range(40)), b"", bytes(range(40))]
    pays = [b"a" * 100, b"b" * 100, b""]
    pool, idx, blk, hl, pl, _ = lay_pool(heads, pays, BUF)
    assert send_and_drain(pool, idx, blk, hl, pl) == (_lib.RNS_E_INVALID, [])
    lib = _lib.load()
    args = (pool.ctypes.data, 9, idx.ctypes.data, blk.ctypes.data, hl.ctypes.data, pl.ctypes.data)
    assert lib.rns_io_send_batch_pool(-1, *args, 3) == _lib.RNS_E_INVALID
    for log2 in (7, 16):
        assert lib.rns_io_send_batch_pool(0, args[0], log2, *args[2:], 3) == _lib.RNS_E_INVALID
    for k in range(6):
        if k != 1:
            bad = list(args)
            bad[k] = None
            assert lib.rns_io_send_batch_pool(0, *bad, 3) == _lib.RNS_E_INVALID
    with pytest.raises(ValueError):
        send_batch_pool(0, pool, idx, blk, hl, pl, 500)
    with pytest.raises(ValueError):
        send_batch_pool(0, pool, idx[:-1], blk, hl, pl)                  # blk_first points past buf_idx
    with pytest.raises(ValueError):
        send_batch_pool(0, pool[:BUF], idx, blk, hl, pl)                 # a buffer outside the pool
    with pytest.raises(ValueError):
        send_batch_pool(0, pool, idx, blk, hl[:2], pl)
