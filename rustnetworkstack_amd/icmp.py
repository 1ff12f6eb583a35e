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
from .batch import _I32, _U8, _call, _local_addrs, _nonnull, _per_packet, _require_cuda, _status, _work_bytes, _workspace
from .pool import (_be_sum, _buf_log2, _fold, _host_datagrams, _new, _pool_batch, recv_batch_pool, send_batch_pool)


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
    cap = n if reply_cap is None else int(reply_cap)
    if not 0 <= cap <= _lib.RNS_CHAIN_MAX_PACKETS or not 0 <= int(ip_id_base) <= 0xFFFF:
        raise ValueError("reply_cap must be a datagram count and ip_id_base a u16")
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    if ip_id_add is not None:
        _require_cuda(ip_id_add, "ip_id_add", _I32)
        if ip_id_add.numel() < 1 or ip_id_add.device != dev:
            raise ValueError(f"ip_id_add must be an int32 tensor (at least 1 entry) on {dev}")
    status = _status(status, n, dev)
    echo = _new(echo, "echo", n, torch.uint8, dev)
    tx_blk_first = _new(tx_blk_first, "tx_blk_first", (cap + 63) // 64, torch.int32, dev)
    tx_head_len8 = _new(tx_head_len8, "tx_head_len8", cap, torch.uint8, dev)
    tx_pay_len16 = _new(tx_pay_len16, "tx_pay_len16", cap, torch.uint16, dev)
    tx_src = _new(tx_src, "tx_src", cap, torch.int32, dev)
    count = _new(count, "count", 3, torch.int32, dev)
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
    free = np.asarray(free, dtype=np.uint32).astype(np.int64)
    n, n_free = len(len16), len(free)
    cap = n if reply_cap is None else int(reply_cap)
    tx_bufs = tx_pool.size >> log2
    status, l4_sum, echo = np.zeros(n, np.uint8), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    heads, pays, srcs, firsts = [], [], [], []
    R = F = V = 0
    full = False
    for i, T, d, st, l4, h, v6 in _host_datagrams(rx_pool, buf_idx, blk_first, len16, ip4, ip6, B, log2):
        status[i], l4_sum[i] = st, l4
        if not (st & _lib.RNS_RX_ACCEPT) or T - h < 4 or (d[6] if v6 else d[9]) != (58 if v6 else 1) or \
                d[h] != (128 if v6 else 8):
            continue
        pay = d[h + 4:]
        nfr = 1 + -(-len(pay) // B)
        R, F = R + 1, F + nfr
        if full or R > cap or F > n_free:
            full = True  # (both counts are monotone: every later request is past them too)
            echo[i] = _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_NOBUF
            continue
        bufs = free[F - nfr:F]
        if (R - 1) % 64 == 0:
            firsts.append(F - nfr)
        pays.append(len(pay))
        srcs.append(i)
        if (bufs >= tx_bufs).any():
            echo[i] = _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BADBUF
            heads.append(0)
            V += 0 if v6 else 1
            continue
        echo[i] = _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BUILT
        if v6:
            peer = d[8:24]
            icmp = bytearray([129, 0, 0, 0])
            seed = _fold(_be_sum(ip6) + _be_sum(peer) + 4 + len(pay) + 58)
            ip = bytes([0x60, 0, 0, 0]) + (4 + len(pay)).to_bytes(2, "big") + bytes([58, 64]) + ip6 + peer
        else:
            peer = d[12:16]
            icmp = bytearray(4)
            seed = 0
            ipb = bytearray([0x45, 0]) + ((24 + len(pay)) & 0xFFFF).to_bytes(2, "big") + \
                ((int(ip_id_base) + int(ip_id_add) + V) & 0xFFFF).to_bytes(2, "big") + bytes([0, 0, 64, 1, 0, 0]) + ip4 + peer
            ipb[10:12] = (_fold(_be_sum(ipb)) ^ 0xFFFF).to_bytes(2, "big")
            ip = bytes(ipb)
            V += 1
        icmp[2:4] = (_fold(seed + _be_sum(icmp) + _be_sum(pay)) ^ 0xFFFF).to_bytes(2, "big")
        head = ip + bytes(icmp)
        heads.append(len(head))
        at = (int(bufs[0]) << log2) + B - len(head)
        tx_pool[at:at + len(head)] = np.frombuffer(head, dtype=np.uint8)
        for j in range(nfr - 1):
            part = pay[j * B:(j + 1) * B]
            at = int(bufs[1 + j]) << log2
            tx_pool[at:at + len(part)] = np.frombuffer(part, dtype=np.uint8)
    # the counts: the answered requests are a prefix of the requests
    nrep = len(pays)
    nbuf = int(sum(1 + -(-p // B) for p in pays))
    return (status, l4_sum, echo, np.array(firsts, dtype=np.uint32), np.array(heads, dtype=np.uint8),
            np.array(pays, dtype=np.uint16), np.array(srcs, dtype=np.uint32), np.array([nrep, nbuf, V], dtype=np.uint32))


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
    rows = rx_pool.reshape(-1, B)
    used = torch.from_numpy(rx_free[:nf].astype(np.int64))
    d_rx = torch.zeros(rows.shape, dtype=torch.uint8, device=dev)
    d_rx[used.to(dev)] = torch.from_numpy(rows[rx_free[:nf]]).to(dev)  # the received buffers only
    d_tx = torch.zeros(tx_pool.size, dtype=torch.uint8, device=dev)
    to_dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)  # noqa: E731
    out = rx_icmp_echo_pool(d_rx.reshape(-1), to_dev(rx_free[:nf].astype(np.uint32), np.int32),
                            to_dev(blk_first.astype(np.uint32), np.int32), to_dev(len16, np.int16), local_ipv4, local_ipv6,
                            d_tx, to_dev(tx_free.astype(np.uint32), np.int32), buf_bytes=B, ip_id_base=ip_id_base)
    echo, tx_blk_first, tx_head_len8, tx_pay_len16, count = out[2], out[3], out[4], out[5], out[7]
    cnt = count.cpu().numpy().view(np.uint32)  # the one synchronisation: 12 bytes
    nrep, nbuf = int(cnt[0]), int(cnt[1])
    sent = 0
    if nrep:
        taken = tx_free[:nbuf].astype(np.int64)
        tx_pool.reshape(-1, B)[taken] = d_tx.reshape(-1, B)[torch.from_numpy(taken).to(dev)].cpu().numpy()
        sent = send_batch_pool(fd_out, tx_pool, tx_free[:nbuf], tx_blk_first.cpu().numpy().view(np.uint32)[:(nrep + 63) // 64],
                               tx_head_len8.cpu().numpy()[:nrep], tx_pay_len16.view(torch.int16).cpu().numpy().view(np.uint16)[:nrep], B)
    return n, sent, echo.cpu().numpy()[:n], cnt
