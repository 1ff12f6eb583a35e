"""Receive verify of datagrams held in fixed-size pool buffers, over compact descriptors.

recv_packet (netif.rs:65-83) leaves a datagram as a chain of full pool buffers and one partly
filled one, so the chain is implied by the datagram's length and its buffers' indices:
``recv_batch_pool`` receives into that form, ``rx_verify_pool`` verifies it on the device
(rns_rx_verify_pool_dev) and ``rx_pool_layout`` computes the index for given lengths.  The
functions are re-exported by ``batch``, whose argument checks they use.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .batch import (_I32, _U16, _call, _descriptors, _local_addrs, _per_packet, _recv_chain_args, _status)


def _buf_log2(buf_bytes: int) -> int:
    """log2 of a pool's buffer size: a power of two in 64..32768 (rns_rx_verify_pool_dev)."""
    buf_bytes = int(buf_bytes)
    if buf_bytes & (buf_bytes - 1) or not 64 <= buf_bytes <= 32768:
        raise ValueError("buf_bytes must be a power of two in 64..32768")
    return buf_bytes.bit_length() - 1


def rx_pool_layout(length, buf_bytes: int = 512):
    """The pool form's index of datagrams of the given lengths (rns_rx_pool_layout): datagram i
    takes ``ceil(length[i] / buf_bytes)`` buffer indices from ``first[i]`` on.  Returns
    (blk_first uint32 [ceil(n/64)], first uint32 [n+1], n_frags)."""
    ln = np.asarray(length)
    if ln.ndim != 1:
        raise ValueError("length must be 1-D")
    if ln.size and (int(ln.max()) > 0xFFFF or int(ln.min()) < 0):
        raise ValueError("the pool form holds u16 datagram lengths (<= 65535)")
    log2 = _buf_log2(buf_bytes)
    l16 = np.ascontiguousarray(ln, dtype=np.uint16)
    n = int(l16.size)
    nb = (n + 63) // 64
    blk, first = np.zeros(max(nb, 1), dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    nf = ctypes.c_uint64(0)
    st = _lib.load().rns_rx_pool_layout(l16.ctypes.data, n, log2, blk.ctypes.data, first.ctypes.data, ctypes.byref(nf))
    _lib.check(st, "rns_rx_pool_layout")
    return blk[:nb], first, int(nf.value)


def rx_verify_pool(pool: torch.Tensor, buf_idx: torch.Tensor, blk_first: torch.Tensor, len16: torch.Tensor,
                   local_ipv4: bytes, local_ipv6: bytes, *, buf_bytes: int = 512, status: torch.Tensor | None = None,
                   l4_sum: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Receive verify of datagrams held in fixed-size pool buffers (rns_rx_verify_pool_dev):
    buffer k = ``pool[k * buf_bytes:]``, datagram i = ``len16[i]`` bytes in the buffers
    ``buf_idx[first_i : first_i + ceil(len16[i] / buf_bytes)]``, all full but the last, with
    ``first_i`` = ``blk_first[i // 64]`` + the buffers of the datagrams before i in its block of 64
    (see ``rx_pool_layout``; ``recv_batch_pool`` produces all three).  Exactly the results of
    ``rx_verify_chain`` on the chains this expands to, from a third of the descriptor bytes.
    Returns ``(status, l4_sum)`` as rx_verify_chain does."""
    dev = _descriptors(pool, ("buf_idx", buf_idx, _I32), ("blk_first", blk_first, _I32), ("len16", len16, _U16))
    log2 = _buf_log2(buf_bytes)
    n, nf = len16.numel(), buf_idx.numel()
    if blk_first.numel() < (n + 63) // 64:
        raise ValueError("blk_first needs one entry per 64 datagrams")
    if n > _lib.RNS_CHAIN_MAX_PACKETS or nf >= 2 ** 32:
        raise ValueError(f"at most {_lib.RNS_CHAIN_MAX_PACKETS} datagrams and 2^32-1 buffers per pool call")
    if pool.data_ptr() & 15:
        raise ValueError("the pool must start 16-byte aligned")
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    status = _status(status, n, dev)
    _call("rns_rx_verify_pool_dev", dev, pool.data_ptr(), pool.numel(), log2, buf_idx.data_ptr(), nf,
          blk_first.data_ptr(), len16.data_ptr(), n, ip4, ip6, status.data_ptr(),
          _per_packet(l4_sum, "l4_sum", n, dev))
    return status, l4_sum


def recv_batch_pool(fd: int, pool: np.ndarray, free: np.ndarray, buf_bytes: int = 512, mru: int = 2048,
                    max_pkts: int | None = None, timeout_ms: int = 0):
    """``recv_batch_chain`` with the compact descriptors of ``rx_verify_pool``
    (rns_io_recv_batch_pool): the same receive loop and the same permutation of ``free``, whose
    first ``n_frags`` entries are then ``buf_idx`` itself.  Returns ``(n, len16 uint16 [n],
    blk_first uint32 [ceil(n/64)], n_frags)``."""
    log2 = _buf_log2(buf_bytes)
    if int(mru) > 0xFFFF:
        raise ValueError("mru must be at most 65535 (the pool form's lengths are u16)")
    buf_bytes, mru, n_free, max_pkts = _recv_chain_args(pool, free, buf_bytes, mru, max_pkts)
    len16 = np.empty(max(max_pkts, 1), dtype=np.uint16)
    blk_first = np.zeros(max((max_pkts + 63) // 64, 1), dtype=np.uint32)
    if max_pkts <= 0:
        return 0, len16[:0], blk_first[:0], 0
    nf = ctypes.c_uint32(0)
    r = _lib.load().rns_io_recv_batch_pool(int(fd), pool.ctypes.data, log2, free.ctypes.data, n_free, mru, max_pkts,
                                           len16.ctypes.data, blk_first.ctypes.data, ctypes.byref(nf), int(timeout_ms))
    if r < 0:
        raise _lib.ChecksumError(r, "rns_io_recv_batch_pool")
    return r, len16[:r], blk_first[:(r + 63) // 64], int(nf.value)
