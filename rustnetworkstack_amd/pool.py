"""Receive verify and transmit finalize of datagrams held in fixed-size pool buffers, over
compact descriptors.

recv_packet (netif.rs:65-83) leaves a datagram as a chain of full pool buffers and one partly
filled one, so the chain is implied by the datagram's length and its buffers' indices:
``recv_batch_pool`` receives into that form, ``rx_verify_pool`` verifies it on the device
(rns_rx_verify_pool_dev) and ``rx_pool_layout`` computes the index for given lengths.  The
transmit side is its twin: append_from_slice (buf.rs:385-420) fills whole buffers and a last one
with the remainder, alloc_header (buf.rs:262-291) prepends a buffer whose data sits at its end, so
a datagram is implied by its head length, its payload length and its buffers' indices.
``tx_pool_layout`` computes the index, ``tx_fill_pool`` finalizes on the device
(rns_tx_fill_pool_dev) and ``send_batch_pool`` sends from that form.  The functions are re-exported
by ``batch``, whose argument checks they use; ``_pool_batch`` and ``_host_datagrams`` are what the
verify's consumers (``place``, ``icmp``, ``udp``) share, ``_cap_and_ids``, ``_tx_outputs``, ``_TxFormHost``,
``_stage_rx`` and ``_send_built`` what the builders into the transmit form (``icmp``, ``udp``) share.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .batch import (_I32, _U8, _U16, _call, _descriptors, _local_addrs, _per_packet, _recv_chain_args, _require_cuda,
                    _status)


def _buf_log2(buf_bytes: int, lowest: int = 64) -> int:
    """log2 of a pool's buffer size: a power of two in 64..32768 (rns_rx_verify_pool_dev), in
    256..32768 for the transmit form (rns_tx_fill_pool_dev: every u8 head length fits a buffer)."""
    buf_bytes = int(buf_bytes)
    if buf_bytes & (buf_bytes - 1) or not lowest <= buf_bytes <= 32768:
        raise ValueError(f"buf_bytes must be a power of two in {lowest}..32768")
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


def _pool_batch(pool: torch.Tensor, buf_idx: torch.Tensor, blk_first: torch.Tensor, len16: torch.Tensor, buf_bytes: int,
                lowest: int, *more, more_bufs: int = 0, demux: bool = False):
    """The checks every call over the pool receive form opens with, but the pool's alignment (``more``: further
    ``_descriptors`` entries; ``more_bufs``: a second buffer count under the cap; ``demux``: the demux's cap).
    Returns ``(device, log2 of buf_bytes, datagrams, buffer indices)``."""
    dev = _descriptors(pool, ("buf_idx", buf_idx, _I32), ("blk_first", blk_first, _I32), ("len16", len16, _U16), *more)
    log2 = _buf_log2(buf_bytes, lowest)
    n, nf = len16.numel(), buf_idx.numel()
    if blk_first.numel() < (n + 63) // 64:
        raise ValueError("blk_first needs one entry per 64 datagrams")
    many, what = ((nf << log2) >= 2 ** 36, "2^36 bytes of buffers per demux call") if demux else \
        (nf >= 2 ** 32 or more_bufs >= 2 ** 32, "2^32-1 buffers per pool call")
    if n > _lib.RNS_CHAIN_MAX_PACKETS or many:
        raise ValueError(f"at most {_lib.RNS_CHAIN_MAX_PACKETS} datagrams and {what}")
    return dev, log2, n, nf


def _new(t: torch.Tensor | None, name: str, n: int, dtype, dev) -> torch.Tensor:
    """An output tensor of at least n entries: the caller's, or a new one."""
    if t is None:
        return torch.empty(max(n, 1), dtype=dtype, device=dev)
    _require_cuda(t, name, (dtype,) if dtype not in _U16 else _U16)
    if t.numel() < n or t.device != dev:
        raise ValueError(f"{name} needs at least {n} entries on {dev}")
    return t


def _np(t, dtype):
    if isinstance(t, torch.Tensor):
        t = t.cpu().numpy()
    return np.ascontiguousarray(t).reshape(-1).view(dtype)


def _cap_and_ids(cap, default: int, ip_id_base: int, ip_id_add, dev, what: str) -> int:
    """A builder's cap (``default`` where None) and IPv4 id arguments, checked; ``what`` names the cap in the
    message.  Returns the cap."""
    cap = default if cap is None else int(cap)
    if not 0 <= cap <= _lib.RNS_CHAIN_MAX_PACKETS or not 0 <= int(ip_id_base) <= 0xFFFF:
        raise ValueError(f"{what} and ip_id_base a u16")
    if ip_id_add is not None:
        _require_cuda(ip_id_add, "ip_id_add", _I32)
        if ip_id_add.numel() < 1 or ip_id_add.device != dev:
            raise ValueError(f"ip_id_add must be an int32 tensor (at least 1 entry) on {dev}")
    return cap


def _tx_outputs(cap: int, dev, tx_blk_first, tx_head_len8, tx_pay_len16, tx_src, count):
    """The transmit form's descriptors for ``cap`` datagrams and the three counts: the caller's tensors, or new ones."""
    return (_new(tx_blk_first, "tx_blk_first", (cap + 63) // 64, torch.int32, dev),
            _new(tx_head_len8, "tx_head_len8", cap, torch.uint8, dev),
            _new(tx_pay_len16, "tx_pay_len16", cap, torch.uint16, dev),
            _new(tx_src, "tx_src", cap, torch.int32, dev), _new(count, "count", 3, torch.int32, dev))


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
    dev, log2, n, nf = _pool_batch(pool, buf_idx, blk_first, len16, buf_bytes, 64)
    if pool.data_ptr() & 15:
        raise ValueError("the pool must start 16-byte aligned")
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    status = _status(status, n, dev)
    _call("rns_rx_verify_pool_dev", dev, pool.data_ptr(), pool.numel(), log2, buf_idx.data_ptr(), nf,
          blk_first.data_ptr(), len16.data_ptr(), n, ip4, ip6, status.data_ptr(),
          _per_packet(l4_sum, "l4_sum", n, dev))
    return status, l4_sum


# --- the pool receive form on the host: what echo_host and demux_host are written over ---
def _be_sum(b) -> int:
    """Sum of the big-endian 16-bit words of b, an odd last byte zero-padded (util.rs:89-99)."""
    a = np.frombuffer(bytes(b), dtype=np.uint8).astype(np.int64)
    return int(a[0::2].sum()) * 256 + int(a[1::2].sum())


def _fold(x: int) -> int:
    while x > 0xFFFF:  # util.rs:101-103
        x = (x & 0xFFFF) + (x >> 16)
    return x


def _verify_host(d: bytes, len0: int, local4: bytes, local6: bytes):
    """(status, l4_sum, ip header length, is IPv6) of one datagram whose first buffer holds len0
    bytes, as rns_rx_verify_pool_dev decides them (ip.rs:38-131, tcp.rs:838-850, icmp.rs:44-75)."""
    bad = (_lib.RNS_RX_MALFORMED, 0, 0, False)
    T = len(d)
    if T == 0:
        return bad
    ver = d[0] >> 4
    st = 0
    if ver == 4:
        hdr = (d[0] & 0xF) * 4
        if hdr == 0 or len0 < 16 or hdr > len0:
            return bad
        if _fold(_be_sum(d[:hdr])) == 0xFFFF:
            st |= _lib.RNS_RX_IP_OK
        if (((d[6] << 8) | d[7]) & 0x3FFF) != 0:
            st |= _lib.RNS_RX_FRAGMENT
        proto, src, local = d[9], d[12:16], local4
    elif ver == 6:
        hdr = 40
        if len0 < 24 or T < 40:
            return bad
        st |= _lib.RNS_RX_IP_OK
        proto, src, local = d[6], d[8:24], local6
    else:
        return bad
    l4len, l4 = T - hdr, 0
    if proto in (6, 1, 58):
        if proto == 58 and ver == 4:
            return bad
        seed = 0 if proto == 1 else _fold(_be_sum(src) + _be_sum(local6 if proto == 58 else local) +
                                          (l4len >> 16) + (l4len & 0xFFFF) + proto)
        l4 = _fold(seed + _be_sum(d[hdr:])) ^ 0xFFFF
        if l4 == 0:
            st |= _lib.RNS_RX_L4_OK
    elif proto == 17:
        st |= _lib.RNS_RX_L4_UNCHECKED
    else:
        st |= _lib.RNS_RX_UNKNOWN_PROTO
    if (st & _lib.RNS_RX_IP_OK) and not (st & _lib.RNS_RX_FRAGMENT) and \
            (st & (_lib.RNS_RX_L4_OK | _lib.RNS_RX_L4_UNCHECKED)):
        st |= _lib.RNS_RX_ACCEPT
    return st, l4, hdr, ver == 6


def _host_datagrams(rx_pool: np.ndarray, buf_idx, blk_first, len16, ip4: bytes, ip6: bytes, B: int, log2: int):
    """The pool receive form on the host, one ``(i, T, d, status, l4_sum, ip header length, is IPv6)`` per
    datagram: its length, its bytes gathered from its buffers and ``_verify_host``'s verdict — or, for a
    datagram whose buffers are not all inside ``buf_idx`` and the pool, ``d`` empty and RNS_RX_MALFORMED."""
    buf_idx = np.asarray(buf_idx, dtype=np.uint32).astype(np.int64)
    blk_first = np.asarray(blk_first, dtype=np.uint32).astype(np.int64)
    len16 = np.asarray(len16, dtype=np.uint16).astype(np.int64)
    nfr = -(-len16 // B)
    for i in range(len(len16)):
        T, nf = int(len16[i]), int(nfr[i])
        gi = int(blk_first[i // 64]) + int(nfr[64 * (i // 64):i].sum())  # the running fragment index of its block
        ok = nf != 0 and gi + nf <= len(buf_idx)
        frags = []
        for j in range(nf if ok else 0):
            at, ln = int(buf_idx[gi + j]) << log2, min(B, T - j * B)
            ok = ok and at + ln <= rx_pool.size
            frags.append(rx_pool[at:at + ln].tobytes())
        if ok:
            d = b"".join(frags)
            yield (i, T, d) + _verify_host(d, min(T, B), ip4, ip6)
        else:
            yield i, T, b"", _lib.RNS_RX_MALFORMED, 0, 0, False


# --- the pool transmit form on the host: what echo_host and send_host are written over ---
assert (_lib.RNS_ECHO_REQUEST, _lib.RNS_ECHO_BUILT, _lib.RNS_ECHO_NOBUF, _lib.RNS_ECHO_BADBUF) == \
    (_lib.RNS_UDPTX_SEND, _lib.RNS_UDPTX_BUILT, _lib.RNS_UDPTX_NOBUF, _lib.RNS_UDPTX_BADBUF)


def _ip_head_bytes(family: int, proto: int, l4_len: int, src: bytes, dst: bytes, ident: int) -> bytes:
    """ip_output_v4 / ip_output_v6 (ip.rs:133-177) in front of ``l4_len`` bytes: the lengths as u16, hop limit 64,
    the IPv4 header checksum filled."""
    if family == 6:
        return bytes([0x60, 0, 0, 0]) + (l4_len & 0xFFFF).to_bytes(2, "big") + bytes([proto, 64]) + src + dst
    ipb = bytearray([0x45, 0]) + ((20 + l4_len) & 0xFFFF).to_bytes(2, "big") + ident.to_bytes(2, "big") + \
        bytes([0, 0, 64, proto, 0, 0]) + src + dst
    ipb[10:12] = (_fold(_be_sum(ipb)) ^ 0xFFFF).to_bytes(2, "big")
    return bytes(ipb)


class _TxFormHost:
    """The allocation of transmit buffers from a free list under a cap, as rns_k_pool_txform.hpp's tx_alloc does
    it, with the descriptors and counts that go with it: ``take`` per item in order, ``place`` for each built
    one, ``result`` at the end."""

    def __init__(self, tx_pool: np.ndarray, free, B: int, cap: int, ip_id_base: int = 0, ip_id_add: int = 0):
        self.pool, self.B, self.log2, self.cap = tx_pool, B, B.bit_length() - 1, cap
        self.tx_bufs = tx_pool.size >> self.log2
        self.free = np.asarray(free, dtype=np.uint32).astype(np.int64)
        self.id0 = int(ip_id_base) + int(ip_id_add)
        self.R = self.F = self.V = 0
        self.full = False
        self.heads, self.pays, self.srcs, self.firsts = [], [], [], []

    def take(self, payload_len: int, v4: bool, src: int):
        """Item ``src``'s ``(status bits, buffers, IPv4 id)``: the buffers are None unless it is built (NOBUF:
        past the cap or the free list; BADBUF: a buffer outside the pool, its descriptors kept with a head
        length of 0 and its id taken)."""
        nfr = 1 + -(-payload_len // self.B)
        self.R, self.F = self.R + 1, self.F + nfr
        if self.full or self.R > self.cap or self.F > len(self.free):
            self.full = True  # (both counts are monotone: every later item is past them too)
            return _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_NOBUF, None, 0
        bufs = self.free[self.F - nfr:self.F]
        if (self.R - 1) % 64 == 0:
            self.firsts.append(self.F - nfr)
        self.pays.append(payload_len)
        self.srcs.append(src)
        ident = (self.id0 + self.V) & 0xFFFF
        self.V += 1 if v4 else 0
        if (bufs >= self.tx_bufs).any():
            self.heads.append(0)
            return _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BADBUF, None, ident
        return _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BUILT, bufs, ident

    def place(self, bufs, head: bytes, payload: bytes):
        """The head at the end of the first buffer, the payload from the start of the following ones."""
        self.heads.append(len(head))
        at = (int(bufs[0]) << self.log2) + self.B - len(head)
        self.pool[at:at + len(head)] = np.frombuffer(head, dtype=np.uint8)
        for j in range(len(bufs) - 1):
            part = payload[j * self.B:(j + 1) * self.B]
            at = int(bufs[1 + j]) << self.log2
            self.pool[at:at + len(part)] = np.frombuffer(part, dtype=np.uint8)

    def result(self):
        """``(tx_blk_first uint32, tx_head_len8 uint8, tx_pay_len16 uint16, tx_src uint32, count uint32 [3])``, the
        descriptor arrays cut to the built items (a prefix of the items)."""
        nbuf = int(sum(1 + -(-p // self.B) for p in self.pays))
        return (np.array(self.firsts, dtype=np.uint32), np.array(self.heads, dtype=np.uint8),
                np.array(self.pays, dtype=np.uint16), np.array(self.srcs, dtype=np.uint32),
                np.array([len(self.pays), nbuf, self.V], dtype=np.uint32))


def _stage_rx(rx_pool: np.ndarray, rx_free: np.ndarray, nf: int, B: int, dev):
    """A receive's used buffers on the device: ``(a zeroed pool of rx_pool's shape with the buffers rx_free[:nf]
    copied in, those indices as buf_idx, to_dev)``; ``to_dev(array, view dtype)`` stages a descriptor array."""
    def to_dev(a, t):
        return torch.from_numpy(np.ascontiguousarray(a).view(t)).to(dev)
    rows = rx_pool.reshape(-1, B)
    d_rx = torch.zeros(rows.shape, dtype=torch.uint8, device=dev)
    d_rx[torch.from_numpy(rx_free[:nf].astype(np.int64)).to(dev)] = torch.from_numpy(rows[rx_free[:nf]]).to(dev)
    return d_rx.reshape(-1), to_dev(rx_free[:nf].astype(np.uint32), np.int32), to_dev


def _send_built(fd_out: int, tx_pool: np.ndarray, tx_free: np.ndarray, d_tx: torch.Tensor, outs, B: int):
    """What a builder left in the device pool ``d_tx``, sent: ``outs`` = its ``(tx_blk_first, tx_head_len8,
    tx_pay_len16, count)``; the 12-byte count read back (the one synchronisation), only the buffers
    ``tx_free[:count[1]]`` copied back into ``tx_pool``, ``send_batch_pool`` to ``fd_out``.  Returns ``(datagrams
    sent, count uint32 [3])``."""
    tx_blk_first, tx_head_len8, tx_pay_len16, count = outs
    cnt = _np(count, np.uint32)
    nb, nbuf = int(cnt[0]), int(cnt[1])
    if nb == 0:
        return 0, cnt
    taken = tx_free[:nbuf].astype(np.int64)
    tx_pool.reshape(-1, B)[taken] = d_tx.reshape(-1, B)[torch.from_numpy(taken).to(d_tx.device)].cpu().numpy()
    return send_batch_pool(fd_out, tx_pool, tx_free[:nbuf], _np(tx_blk_first, np.uint32)[:(nb + 63) // 64],
                           _np(tx_head_len8, np.uint8)[:nb], _np(tx_pay_len16.view(torch.int16), np.uint16)[:nb], B), cnt


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


def tx_pool_layout(pay_len, buf_bytes: int = 512):
    """The pool transmit form's index of datagrams with the given payload lengths
    (rns_tx_pool_layout): datagram i takes ``1 + ceil(pay_len[i] / buf_bytes)`` buffer indices from
    ``first[i]`` on, the head buffer first.  Returns (blk_first uint32 [ceil(n/64)], first uint32
    [n+1], n_frags)."""
    pl = np.asarray(pay_len)
    if pl.ndim != 1:
        raise ValueError("pay_len must be 1-D")
    if pl.size and (int(pl.max()) > 0xFFFF or int(pl.min()) < 0):
        raise ValueError("the pool form holds u16 payload lengths (<= 65535)")
    log2 = _buf_log2(buf_bytes, 256)
    p16 = np.ascontiguousarray(pl, dtype=np.uint16)
    n = int(p16.size)
    nb = (n + 63) // 64
    blk, first = np.zeros(max(nb, 1), dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    nf = ctypes.c_uint64(0)
    st = _lib.load().rns_tx_pool_layout(p16.ctypes.data, n, log2, blk.ctypes.data, first.ctypes.data, ctypes.byref(nf))
    _lib.check(st, "rns_tx_pool_layout")
    return blk[:nb], first, int(nf.value)


def tx_fill_pool(pool: torch.Tensor, buf_idx: torch.Tensor, blk_first: torch.Tensor, head_len8: torch.Tensor,
                 pay_len16: torch.Tensor, *, buf_bytes: int = 512, status: torch.Tensor | None = None) -> torch.Tensor:
    """Transmit finalize of datagrams held in fixed-size pool buffers (rns_tx_fill_pool_dev): buffer
    k = ``pool[k * buf_bytes:]``, datagram i = the LAST ``head_len8[i]`` bytes of its head buffer
    followed by ``pay_len16[i]`` payload bytes in buffers read from their start, all full but the
    last; its ``1 + ceil(pay_len16[i] / buf_bytes)`` indices are ``buf_idx[first_i:]`` with
    ``first_i`` = ``blk_first[i // 64]`` + the buffers of the datagrams before i in its block of 64
    (see ``tx_pool_layout``).  Exactly the bytes and the uint8 status per datagram of
    ``tx_fill_chain`` on the chains this expands to.  A head buffer must not be named twice."""
    dev = _descriptors(pool, ("buf_idx", buf_idx, _I32), ("blk_first", blk_first, _I32),
                       ("head_len8", head_len8, _U8), ("pay_len16", pay_len16, _U16))
    log2 = _buf_log2(buf_bytes, 256)
    n, nf = pay_len16.numel(), buf_idx.numel()
    if head_len8.numel() != n:
        raise ValueError("head_len8 and pay_len16 must have one entry per datagram each")
    if blk_first.numel() < (n + 63) // 64:
        raise ValueError("blk_first needs one entry per 64 datagrams")
    if n > _lib.RNS_CHAIN_MAX_PACKETS or nf >= 2 ** 32:
        raise ValueError(f"at most {_lib.RNS_CHAIN_MAX_PACKETS} datagrams and 2^32-1 buffers per pool call")
    if pool.data_ptr() & 15:
        raise ValueError("the pool must start 16-byte aligned")
    status = _status(status, n, dev)
    _call("rns_tx_fill_pool_dev", dev, pool.data_ptr(), pool.numel(), log2, buf_idx.data_ptr(), nf,
          blk_first.data_ptr(), head_len8.data_ptr(), pay_len16.data_ptr(), n, status.data_ptr())
    return status


def send_batch_pool(fd: int, pool: np.ndarray, buf_idx: np.ndarray, blk_first: np.ndarray, head_len8: np.ndarray,
                    pay_len16: np.ndarray, buf_bytes: int = 512) -> int:
    """Send datagrams held in the pool transmit form (rns_io_send_batch_pool): each goes out as one
    datagram gathered from its head bytes and its payload buffers, as ``send_batch_chain`` sends
    the chains the form expands to.  Returns the number of datagrams sent."""
    log2 = _buf_log2(buf_bytes, 256)
    if pool.dtype != np.uint8 or not pool.flags["C_CONTIGUOUS"]:
        raise ValueError("pool must be a contiguous uint8 array")
    buf_idx = np.ascontiguousarray(buf_idx, dtype=np.uint32)
    blk_first = np.ascontiguousarray(blk_first, dtype=np.uint32)
    head_len8 = np.ascontiguousarray(head_len8, dtype=np.uint8)
    pay_len16 = np.ascontiguousarray(pay_len16, dtype=np.uint16)
    n = int(pay_len16.shape[0])
    if head_len8.shape[0] != n or blk_first.shape[0] < (n + 63) // 64:
        raise ValueError("head_len8 and pay_len16 need one entry per datagram, blk_first one per 64")
    nfr = 1 + (pay_len16.astype(np.int64) + int(buf_bytes) - 1) // int(buf_bytes)
    for b in range((n + 63) // 64):  # every block's buffers lie inside buf_idx, and inside the pool
        end = int(blk_first[b]) + int(nfr[64 * b:64 * b + 64].sum())
        if end > buf_idx.shape[0]:
            raise ValueError("blk_first points past buf_idx")
    if buf_idx.shape[0] and int(buf_idx.max()) >= pool.shape[0] // int(buf_bytes):
        raise ValueError("buf_idx names a buffer outside the pool")
    r = _lib.load().rns_io_send_batch_pool(int(fd), pool.ctypes.data, log2, buf_idx.ctypes.data, blk_first.ctypes.data,
                                           head_len8.ctypes.data, pay_len16.ctypes.data, n)
    if r < 0:
        raise _lib.ChecksumError(r, "rns_io_send_batch_pool")
    return r
