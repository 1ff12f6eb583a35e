"""ICMP echo responder: icmp_input's reply built on the device.

icmp_input_v4 / icmp_input_v6 (icmp.rs:44-85) verify an echo request, copy its payload into fresh
buffers, prepend a zeroed 4-byte ICMP header, checksum the reply and hand it to ip_output_v4 / v6.
``rx_icmp_echo_pool`` does all of it for a batch held in the pool form (``pool.rx_verify_pool``'s
layout): every accepted echo request becomes a finished reply in a transmit pool, its buffers drawn
from a free list on the device, described by the compact descriptors ``pool.tx_fill_pool`` and
``pool.send_batch_pool`` take (rns_rx_icmp_echo_pool_dev).  ``echo_host`` is the same function in
numpy over host pools — the host's path for the requests the device leaves (``RNS_ECHO_NOBUF``) —
and ``echo_respond`` one receive -> device -> send step.  The functions are re-exported by
``batch``, whose argument checks they use.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .batch import _I32, _U8, _call, _local_addrs, _nonnull, _per_packet, _status, _work_bytes, _workspace
from .pool import (_be_sum, _buf_log2, _cap_and_ids, _fold, _host_datagrams, _ip_head_bytes, _new, _pool_batch, _send_built,
                   _stage_rx, _tx_outputs, _TxFormHost, recv_batch_pool)


def echo_work(n_pkts: int) -> int:
    """Bytes of workspace ``rx_icmp_echo_pool`` needs for ``n_pkts`` datagrams (rns_rx_icmp_echo_work)."""
    return _work_bytes("rns_rx_icmp_echo_work", int(n_pkts))


def rx_icmp_echo_pool(rx_pool: torch.Tensor, buf_idx: torch.Tensor, blk_first: torch.Tensor, len16: torch.Tensor,
                      local_ipv4: bytes, local_ipv6: bytes, tx_pool: torch.Tensor, free: torch.Tensor, *,
                      buf_bytes: int = 512, reply_cap: int | None = None, ip_id_base: int = 0,
                      ip_id_add: torch.Tensor | None = None, status: torch.Tensor | None = None,
                      l4_sum: torch.Tensor | None = None, echo: torch.Tensor | None = None,
                      tx_blk_first: torch.Tensor | None = None, tx_head_len8: torch.Tensor | None = None,
                      tx_pay_len16: torch.Tensor | None = None, tx_src: torch.Tensor | None = None,
                      count: torch.Tensor | None = None, work: torch.Tensor | None = None):
    """ICMP echo responder over pool buffers (rns_rx_icmp_echo_pool_dev).  ``rx_pool`` / ``buf_idx`` /
    ``blk_first`` / ``len16`` as for ``rx_verify_pool`` (``buf_bytes`` a power of two in 256..32768, the
    same for both pools); ``free`` = int32 indices of free buffers of ``tx_pool``, taken in order.
    Every accepted echo request (IPv4 type 8, IPv6 type 128) within ``reply_cap`` (default: one per
    datagram) and the free list becomes a finished reply: reply r has its head (24 / 44 bytes, both
    checksums filled, source = the local address, IPv4 id = ``ip_id_base`` + ``ip_id_add[0]`` + the IPv4
    replies before it) at the end of its first buffer and its payload in the following ones, and the
    replies' buffers are ``free[:count[1]]`` in order — the ``buf_idx`` of the transmit pool form, with
    ``tx_blk_first`` / ``tx_head_len8`` / ``tx_pay_len16`` its other descriptors and ``tx_src[r]`` the
    request's index.  ``echo[i]`` holds RNS_ECHO_* bits; ``count`` = (replies, buffers, IPv4 replies),
    int32 on the device: nothing is synchronised here, the counts stay on the device until the caller
    reads them.  Returns ``(status, l4_sum, echo, tx_blk_first, tx_head_len8, tx_pay_len16, tx_src,
    count)``; status and l4_sum are ``rx_verify_pool``'s."""
    dev, log2, n, nf = _pool_batch(rx_pool, buf_idx, blk_first, len16, buf_bytes, 256, ("tx_pool", tx_pool, _U8),
                                   ("free", free, _I32), more_bufs=free.numel())
    n_free = free.numel()
    if rx_pool.data_ptr() & 15 or tx_pool.data_ptr() & 15:
        raise ValueError("the pools must start 16-byte aligned")
    cap = _cap_and_ids(reply_cap, n, ip_id_base, ip_id_add, dev, "reply_cap must be a datagram count")
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    status = _status(status, n, dev)
    echo = _new(echo, "echo", n, torch.uint8, dev)
    tx_blk_first, tx_head_len8, tx_pay_len16, tx_src, count = _tx_outputs(cap, dev, tx_blk_first, tx_head_len8, tx_pay_len16,
                                                                          tx_src, count)
    need = echo_work(n)
    work = _workspace(work, need, dev, torch.int64, f"work needs {need} bytes (echo_work) on {dev}")
    ptr = _nonnull(dev)
    _call("rns_rx_icmp_echo_pool_dev", dev, rx_pool.data_ptr(), rx_pool.numel(), log2, buf_idx.data_ptr(), nf,
          ptr(blk_first), ptr(len16), n, ip4, ip6, ptr(tx_pool), tx_pool.numel(), free.data_ptr(), n_free, cap,
          int(ip_id_base), None if ip_id_add is None else ip_id_add.data_ptr(), tx_blk_first.data_ptr(),
          tx_head_len8.data_ptr(), tx_pay_len16.data_ptr(), tx_src.data_ptr(), count.data_ptr(), ptr(status),
          _per_packet(l4_sum, "l4_sum", n, dev), echo.data_ptr(), work.data_ptr(), work.numel() * 8)
    return status, l4_sum, echo, tx_blk_first, tx_head_len8, tx_pay_len16, tx_src, count


# ---------------------------------------------------------------------------
# the same on the host
# ---------------------------------------------------------------------------
def echo_host(rx_pool: np.ndarray, buf_idx, blk_first, len16, local_ipv4: bytes, local_ipv6: bytes, tx_pool: np.ndarray,
              free, *, buf_bytes: int = 512, reply_cap: int | None = None, ip_id_base: int = 0, ip_id_add: int = 0):
    """``rx_icmp_echo_pool`` in numpy over host pools (uint8 arrays; ``tx_pool`` is written in place, and
    may be ``rx_pool``): the same requests, allocation, descriptors, counts and reply bytes — the host's
    path for the requests the device leaves with RNS_ECHO_NOBUF, and what the GPU tests compare with.
    Returns ``(status uint8 [n], l4_sum uint16 [n], echo uint8 [n], tx_blk_first uint32, tx_head_len8
    uint8, tx_pay_len16 uint16, tx_src uint32, count uint32 [3])``, the descriptor arrays cut to the
    replies.  The bytes after a payload's end in its last buffer stay as they were."""
    B = int(buf_bytes)
    log2 = _buf_log2(B, 256)
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    n = len(len16)
    tx = _TxFormHost(tx_pool, free, B, n if reply_cap is None else int(reply_cap), ip_id_base, ip_id_add)
    status, l4_sum, echo = np.zeros(n, np.uint8), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    for i, T, d, st, l4, h, v6 in _host_datagrams(rx_pool, buf_idx, blk_first, len16, ip4, ip6, B, log2):
        status[i], l4_sum[i] = st, l4
        if not (st & _lib.RNS_RX_ACCEPT) or T - h < 4 or (d[6] if v6 else d[9]) != (58 if v6 else 1) or \
                d[h] != (128 if v6 else 8):
            continue
        pay = d[h + 4:]
        echo[i], bufs, ident = tx.take(len(pay), not v6, i)
        if bufs is None:
            continue
        src, peer = (ip6, d[8:24]) if v6 else (ip4, d[12:16])
        icmp = bytearray([129 if v6 else 0, 0, 0, 0])
        seed = _fold(_be_sum(ip6) + _be_sum(peer) + 4 + len(pay) + 58) if v6 else 0
        icmp[2:4] = (_fold(seed + _be_sum(icmp) + _be_sum(pay)) ^ 0xFFFF).to_bytes(2, "big")
        tx.place(bufs, _ip_head_bytes(6 if v6 else 4, 58 if v6 else 1, 4 + len(pay), src, peer, ident) + bytes(icmp), pay)
    return (status, l4_sum, echo) + tx.result()


def echo_respond(fd_in: int, fd_out: int, rx_pool: np.ndarray, rx_free: np.ndarray, tx_pool: np.ndarray, tx_free: np.ndarray,
                 local_ipv4: bytes, local_ipv6: bytes, *, buf_bytes: int = 512, mru: int = 2048, max_pkts: int | None = None,
                 ip_id_base: int = 0, device: str = "cuda:0", timeout_ms: int = 0):
    """One receive -> device -> send step: ``recv_batch_pool`` from ``fd_in`` into the host ``rx_pool``,
    the used buffers to the device, ``rx_icmp_echo_pool`` into a device copy of ``tx_pool``'s shape, the
    12-byte count read back, only the buffers ``tx_free[:count[1]]`` copied back into ``tx_pool``, and
    ``send_batch_pool`` to ``fd_out``.  Returns ``(datagrams received, replies sent, echo uint8 [n],
    count)``; requests with RNS_ECHO_NOBUF are the caller's to answer (``echo_host``)."""
    B = int(buf_bytes)
    n, len16, blk_first, nf = recv_batch_pool(fd_in, rx_pool, rx_free, B, mru, max_pkts, timeout_ms)
    if n == 0:
        return 0, 0, np.zeros(0, np.uint8), np.zeros(3, np.uint32)
    dev = torch.device(device)
    d_rx, d_idx, to_dev = _stage_rx(rx_pool, rx_free, nf, B, dev)
    d_tx = torch.zeros(tx_pool.size, dtype=torch.uint8, device=dev)
    out = rx_icmp_echo_pool(d_rx, d_idx, to_dev(blk_first.astype(np.uint32), np.int32), to_dev(len16, np.int16), local_ipv4,
                            local_ipv6, d_tx, to_dev(tx_free.astype(np.uint32), np.int32), buf_bytes=B, ip_id_base=ip_id_base)
    sent, cnt = _send_built(fd_out, tx_pool, tx_free, d_tx, (out[3], out[4], out[5], out[7]), B)
    return n, sent, out[2].cpu().numpy()[:n], cnt
