"""UDP receive demux: udp_input's socket queues built on the device.

udp_input (udp.rs:126-148) reads a datagram's ports, looks the destination port up in PORT_MAP and
pushes (source address, source port, payload) onto that socket's receive_queue; udp_recv
(udp.rs:75-98) pops the queue front first.  ``rx_udp_demux_pool`` does the first half for a batch held
in the pool form (``pool.rx_verify_pool``'s layout): every accepted UDP datagram to a bound port becomes
a 32-byte record and a payload copied to a 16-byte-aligned place, the records and the payloads of a
socket contiguous and in arrival order (rns_rx_udp_demux_pool_dev).  ``demux_host`` is the same function
in numpy over a host pool — the host's path for the entries the device leaves (``RNS_UDP_NOROOM``) and
what the GPU tests compare with — ``drain`` the list repeated udp_recv calls would return, and
``udp_demux`` one receive -> device -> drain step.

The send build is the other half: udp_send -> udp_output -> ip_output_v4 / ip_output_v6 (udp.rs:101-114 and
150-173, ip.rs:133-177) for a batch.  ``tx_udp_send_pool`` reads the demux's records as sends back to their
senders (or a host's own records) and builds every datagram, both checksums filled, in a transmit pool in the
form ``pool.tx_fill_pool`` and ``pool.send_batch_pool`` take (rns_tx_udp_send_pool_dev); ``send_host`` is the
same function in numpy — the host's path for what the device leaves (``RNS_UDPTX_NOBUF``) — and ``udp_echo`` the
reference's udp_echo application as one receive -> demux -> send -> sendmmsg step.

The functions are re-exported by ``batch``, whose argument checks they use.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .batch import (_I32, _U8, _U16, _call, _descriptors, _local_addrs, _nonnull, _per_packet, _require_cuda, _status,
                    _work_bytes, _workspace)
from .pool import (_be_sum, _buf_log2, _cap_and_ids, _fold, _host_datagrams, _ip_head_bytes, _new, _np, _pool_batch, _send_built,
                   _stage_rx, _tx_outputs, _TxFormHost, recv_batch_pool, send_batch_pool)

REC = np.dtype([("ip", "u1", 16), ("src", "<u4"), ("off16", "<u4"), ("sport", "<u2"), ("len", "<u2"), ("family", "u1"),
                ("flags", "u1"), ("pad", "u1", 2)])  # rns_udp_rec
assert REC.itemsize == 32
NO_POS = 0xFFFFFFFF


class UdpDemux(NamedTuple):
    """What a demux call leaves: torch tensors from ``rx_udp_demux_pool``, numpy arrays from ``demux_host``."""
    status: object   # uint8 [n]: rx_verify_pool's
    l4_sum: object   # uint16 [n] or None
    udp: object      # uint8 [n]: RNS_UDP_* bits
    pos: object      # uint32 [n]: the record's position, 0xffffffff if none
    rec: object      # the records (REC on the host; uint8 [rec_cap * 32] on the device)
    q_first: object  # uint32 [n_socks + 1]
    count: object    # uint32 [2]: entries, 16-byte units
    data: object     # uint8: the payloads


def port_table(ports) -> np.ndarray:
    """PORT_MAP as the demux's table (rns_rx_udp_port_table_build): uint16 [65536], ``ports[s]`` -> s, every
    other entry RNS_UDP_NO_SOCK.  A duplicate port (udp_open's "Port already in use") or more than
    RNS_UDP_MAX_SOCKS ports raise."""
    p = np.ascontiguousarray(np.asarray(ports, dtype=np.int64).reshape(-1))
    if p.size and (int(p.min()) < 0 or int(p.max()) > 0xFFFF):
        raise ValueError("ports are u16")
    p16 = p.astype(np.uint16)
    tbl = np.empty(65536, dtype=np.uint16)
    _lib.check(_lib.load().rns_rx_udp_port_table_build(p16.ctypes.data if p16.size else None, int(p16.size), tbl.ctypes.data),
               "rns_rx_udp_port_table_build")
    return tbl


def demux_work(n_pkts: int, n_socks: int) -> int:
    """Bytes of workspace ``rx_udp_demux_pool`` needs (rns_rx_udp_demux_work)."""
    return _work_bytes("rns_rx_udp_demux_work", int(n_pkts), int(n_socks))


def rx_udp_demux_pool(rx_pool: torch.Tensor, buf_idx: torch.Tensor, blk_first: torch.Tensor, len16: torch.Tensor,
                      local_ipv4: bytes, local_ipv6: bytes, port_tbl: torch.Tensor | None, n_socks: int, *,
                      buf_bytes: int = 512, rec_cap: int | None = None, data: torch.Tensor | None = None,
                      rec: torch.Tensor | None = None, status: torch.Tensor | None = None,
                      l4_sum: torch.Tensor | None = None, udp: torch.Tensor | None = None, pos: torch.Tensor | None = None,
                      q_first: torch.Tensor | None = None, count: torch.Tensor | None = None,
                      work: torch.Tensor | None = None) -> UdpDemux:
    """UDP receive demux over pool buffers (rns_rx_udp_demux_pool_dev).  ``rx_pool`` / ``buf_idx`` /
    ``blk_first`` / ``len16`` as for ``rx_verify_pool`` (``buf_bytes`` a power of two in 128..32768);
    ``port_tbl`` = ``port_table(ports)`` on the device as int16 / uint16 [65536] (None with ``n_socks`` 0).
    Every accepted UDP datagram whose destination port maps to a socket s < ``n_socks`` becomes entry
    ``pos[i]`` of the socket-major queues: ``rec`` (uint8, 32 bytes per record, ``REC``) and its payload at
    ``data[16 * off16:]``; socket s owns records ``q_first[s]:q_first[s + 1]``.  ``rec_cap`` (default: one
    per datagram) and ``data`` (default: one byte per pool-buffer byte in use, so nothing is cut) bound what
    is written; entries past them get RNS_UDP_NOROOM.  Nothing is synchronised here.  Returns a
    ``UdpDemux`` of device tensors (``udp`` uint8 [n], ``pos`` / ``q_first`` / ``count`` int32)."""
    dev, log2, n, nf = _pool_batch(rx_pool, buf_idx, blk_first, len16, buf_bytes, 128, demux=True)
    n_socks = int(n_socks)
    if not 0 <= n_socks <= _lib.RNS_UDP_MAX_SOCKS:
        raise ValueError(f"n_socks must be at most {_lib.RNS_UDP_MAX_SOCKS}")
    if rx_pool.data_ptr() & 15:
        raise ValueError("the pool must start 16-byte aligned")
    if n_socks:
        _require_cuda(port_tbl, "port_tbl", _U16)
        if port_tbl.numel() != 65536 or port_tbl.device != dev:
            raise ValueError(f"port_tbl must have 65536 entries on {dev}")
    cap = n if rec_cap is None else int(rec_cap)
    if not 0 <= cap <= _lib.RNS_CHAIN_MAX_PACKETS:
        raise ValueError("rec_cap must be a datagram count")
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    if data is None:
        data = torch.empty(max(nf << log2, 16), dtype=torch.uint8, device=dev)
    rec = _new(rec, "rec", 32 * cap, torch.uint8, dev)
    for name, t in (("data", data), ("rec", rec)):
        _require_cuda(t, name, _U8)
        if t.device != dev or t.data_ptr() & 15:
            raise ValueError(f"{name} must be 16-byte aligned on {dev}")
    status = _status(status, n, dev)
    udp = _new(udp, "udp", n, torch.uint8, dev)
    pos = _new(pos, "pos", n, torch.int32, dev)
    q_first = _new(q_first, "q_first", n_socks + 1, torch.int32, dev)
    count = _new(count, "count", 2, torch.int32, dev)
    need = demux_work(n, n_socks)
    if work is None:
        work = torch.empty(-(-max(need, 16) // 8), dtype=torch.int64, device=dev)
    _require_cuda(work, "work", (torch.int64,))
    if work.numel() * 8 < need or work.device != dev or work.data_ptr() & 15:
        raise ValueError(f"work needs {need} bytes (demux_work), 16-byte aligned, on {dev}")
    ptr = _nonnull(dev)
    _call("rns_rx_udp_demux_pool_dev", dev, rx_pool.data_ptr(), rx_pool.numel(), log2, buf_idx.data_ptr(), nf,
          ptr(blk_first), ptr(len16), n, ip4, ip6, port_tbl.data_ptr() if n_socks else None, n_socks,
          data.data_ptr(), data.numel(), rec.data_ptr(), cap, q_first.data_ptr(), count.data_ptr(), ptr(status),
          _per_packet(l4_sum, "l4_sum", n, dev), ptr(udp), ptr(pos), work.data_ptr(), work.numel() * 8)
    return UdpDemux(status, l4_sum, udp, pos, rec, q_first, count, data)


# ---------------------------------------------------------------------------
# the same on the host
# ---------------------------------------------------------------------------
def demux_host(rx_pool: np.ndarray, buf_idx, blk_first, len16, local_ipv4: bytes, local_ipv6: bytes, port_tbl, n_socks: int,
               *, buf_bytes: int = 512, rec_cap: int | None = None, data: np.ndarray | None = None,
               rec: np.ndarray | None = None) -> UdpDemux:
    """``rx_udp_demux_pool`` in numpy over a host pool (uint8 array): the same decode, lookup, queue order,
    cut, records and payload bytes — the host's path for the entries the device leaves with
    RNS_UDP_NOROOM, and what the GPU tests compare with.  ``data`` (uint8) and ``rec`` (``REC``) are written
    in place where given (``rec_cap`` defaults to ``len(rec)``, else to one per datagram); the bytes after a
    payload's end up to the next 16-byte boundary stay as they were.  Returns a ``UdpDemux`` of numpy
    arrays."""
    B = int(buf_bytes)
    log2 = _buf_log2(B, 128)
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    n, n_frags, n_socks = len(len16), len(buf_idx), int(n_socks)
    if not 0 <= n_socks <= _lib.RNS_UDP_MAX_SOCKS:
        raise ValueError(f"n_socks must be at most {_lib.RNS_UDP_MAX_SOCKS}")
    tbl = np.asarray(port_tbl, dtype=np.uint16) if n_socks else None
    cap = (n if rec is None else len(rec)) if rec_cap is None else int(rec_cap)
    if data is None:
        data = np.zeros(max(n_frags << log2, 16), dtype=np.uint8)
    if rec is None:
        rec = np.zeros(cap, dtype=REC)
    status, l4_sum, udp = np.zeros(n, np.uint8), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    pos = np.full(n, NO_POS, dtype=np.uint32)
    entries = []  # (socket, datagram, source address, source port, family, payload)
    for i, T, d, st, l4, h, v6 in _host_datagrams(rx_pool, buf_idx, blk_first, len16, ip4, ip6, B, log2):
        status[i], l4_sum[i] = st, l4
        if not (st & _lib.RNS_RX_ACCEPT) or (d[6] if v6 else d[9]) != 17 or T - h < 8:
            continue
        udp[i] = _lib.RNS_UDP_DGRAM
        dport = (d[h + 2] << 8) | d[h + 3]
        s = int(tbl[dport]) if n_socks else _lib.RNS_UDP_NO_SOCK
        if s >= n_socks:
            continue  # "No socket listening"
        udp[i] |= _lib.RNS_UDP_SOCK
        entries.append((s, i, d[8:24] if v6 else d[12:16] + bytes(12), (d[h] << 8) | d[h + 1], 6 if v6 else 4, d[h + 8:]))
    # socket-major, arrival order within a socket: a stable sort by socket
    entries.sort(key=lambda e: e[0])
    q_first = np.zeros(n_socks + 1, dtype=np.uint32)
    off = 0
    for k, (s, i, ip, sport, fam, pay) in enumerate(entries):
        q_first[s + 1:] += 1
        units = -(-len(pay) // 16)
        if k < cap and 16 * (off + units) <= data.size:
            udp[i] |= _lib.RNS_UDP_QUEUED
            pos[i] = k
            rec[k] = (np.frombuffer(ip, dtype=np.uint8), i, off, sport, len(pay), fam, udp[i], (0, 0))
            data[16 * off:16 * off + len(pay)] = np.frombuffer(pay, dtype=np.uint8)
        else:
            udp[i] |= _lib.RNS_UDP_NOROOM
        off += units
    return UdpDemux(status, l4_sum, udp, pos, rec, q_first, np.array([len(entries), off], dtype=np.uint32), data)


def drain(result: UdpDemux, s: int):
    """What repeated udp_recv calls on socket ``s`` would return after the batch, front first: a list of
    ``(source address bytes (4 or 16), source port, payload bytes)``.  Entries the cut left out
    (RNS_UDP_NOROOM: no record) end the list: they are the host's to queue, behind these."""
    q = _np(result.q_first, np.uint32)
    cnt = _np(result.count, np.uint32)
    rec, data = _np(result.rec, np.uint8), _np(result.data, np.uint8)
    pos = np.sort(_np(result.pos, np.uint32))
    out = []
    for k in range(int(q[s]), int(q[s + 1])):
        if k * 32 + 32 > rec.size or k >= int(cnt[0]) or pos[np.searchsorted(pos, k) % pos.size] != k:
            break  # cut: its record was not written
        r = rec[32 * k:32 * k + 32].view(REC)[0]
        at = 16 * int(r["off16"])
        out.append((r["ip"][:4 if r["family"] == 4 else 16].tobytes(), int(r["sport"]), data[at:at + int(r["len"])].tobytes()))
    return out


def udp_demux(fd: int, pool: np.ndarray, free: np.ndarray, ports, local_ipv4: bytes, local_ipv6: bytes, *,
              buf_bytes: int = 512, mru: int = 2048, max_pkts: int | None = None, device: str = "cuda:0",
              timeout_ms: int = 0):
    """One receive -> device -> drain step: ``recv_batch_pool`` from ``fd`` into the host ``pool``, the used
    buffers to the device, ``rx_udp_demux_pool`` over the table of ``ports``, the result read back.  Returns
    ``(datagrams received, UdpDemux of numpy arrays)``; ``drain(result, s)`` is then socket s's queue."""
    B = int(buf_bytes)
    ports = list(ports)
    n, len16, blk_first, nf = recv_batch_pool(fd, pool, free, B, mru, max_pkts, timeout_ms)
    if n == 0:
        z = np.zeros(0, np.uint8)
        return 0, UdpDemux(z, np.zeros(0, np.uint16), z, np.zeros(0, np.uint32), np.zeros(0, REC),
                           np.zeros(len(ports) + 1, np.uint32), np.zeros(2, np.uint32), z)
    d_rx, d_idx, to_dev = _stage_rx(pool, free, nf, B, torch.device(device))
    r = rx_udp_demux_pool(d_rx, d_idx, to_dev(blk_first.astype(np.uint32), np.int32), to_dev(len16, np.int16), local_ipv4,
                          local_ipv6, to_dev(port_table(ports), np.int16) if ports else None, len(ports), buf_bytes=B)
    cnt = _np(r.count, np.uint32)  # the one synchronisation the host needs first: 8 bytes
    nrec, nunits = int(cnt[0]), int(cnt[1])
    return n, UdpDemux(_np(r.status, np.uint8), None, _np(r.udp, np.uint8)[:n], _np(r.pos, np.uint32)[:n],
                       _np(r.rec[:32 * nrec], np.uint8).view(REC), _np(r.q_first, np.uint32), cnt,
                       _np(r.data[:16 * nunits], np.uint8))


# ---------------------------------------------------------------------------
# the send build: udp_send -> udp_output -> ip_output for a batch of records read as sends
# ---------------------------------------------------------------------------
class UdpSend(NamedTuple):
    """What a send build leaves: torch tensors from ``tx_udp_send_pool``, numpy arrays from ``send_host`` (there
    the descriptor arrays are cut to the built datagrams)."""
    send: object          # uint8 [n_recs]: RNS_UDPTX_* bits
    tx_blk_first: object  # uint32: buffers before datagram 64 * b
    tx_head_len8: object  # uint8: 28 / 48, 0 for RNS_UDPTX_BADBUF
    tx_pay_len16: object  # uint16
    tx_src: object        # uint32: the record's index
    count: object         # uint32 [3]: datagrams, buffers taken, IPv4 ids taken


def udp_send_work(n_recs: int) -> int:
    """Bytes of workspace ``tx_udp_send_pool`` needs for ``n_recs`` records (rns_tx_udp_send_work)."""
    return _work_bytes("rns_tx_udp_send_work", int(n_recs))


def tx_udp_send_pool(data: torch.Tensor, rec: torch.Tensor, q_first: torch.Tensor, sock_port: torch.Tensor,
                     local_ipv4: bytes, local_ipv6: bytes, tx_pool: torch.Tensor, free: torch.Tensor, *,
                     buf_bytes: int = 512, n_recs: int | None = None, send_cap: int | None = None, ip_id_base: int = 0,
                     ip_id_add: torch.Tensor | None = None, send: torch.Tensor | None = None,
                     tx_blk_first: torch.Tensor | None = None, tx_head_len8: torch.Tensor | None = None,
                     tx_pay_len16: torch.Tensor | None = None, tx_src: torch.Tensor | None = None,
                     count: torch.Tensor | None = None, work: torch.Tensor | None = None) -> UdpSend:
    """UDP send build over pool buffers (rns_tx_udp_send_pool_dev).  ``data`` / ``rec`` / ``q_first`` as
    ``rx_udp_demux_pool`` leaves them (``rec`` uint8, 32 bytes per record, ``REC``; ``n_recs`` defaults to all of
    ``rec``: the records past ``q_first[-1]`` are no sends), or a host's own sends grouped by socket with flags =
    RNS_UDP_QUEUED; ``sock_port`` = the sockets' ports, int16 / uint16 [n_socks]; ``free`` = int32 indices of free
    buffers of ``tx_pool``, taken in order (``buf_bytes`` a power of two in 256..32768).  Record k is a send to its
    address and port from its socket's port; every send within ``send_cap`` (default: one per record) and the
    free list becomes a finished datagram: datagram r has its head (28 / 48 bytes, both checksums filled, source =
    the local address, IPv4 id = ``ip_id_base`` + ``ip_id_add[0]`` + the IPv4 sends before it) at the end of its
    first buffer and its payload in the following ones, and the datagrams' buffers are ``free[:count[1]]`` in
    order — the ``buf_idx`` of the transmit pool form, with ``tx_blk_first`` / ``tx_head_len8`` / ``tx_pay_len16``
    its other descriptors and ``tx_src[r]`` the record's index.  ``send[k]`` holds RNS_UDPTX_* bits; ``count`` =
    (datagrams, buffers, IPv4 datagrams), int32 on the device: nothing is synchronised here.  Returns a
    ``UdpSend`` of device tensors."""
    dev = _descriptors(data, ("rec", rec, _U8), ("q_first", q_first, _I32), ("sock_port", sock_port, _U16),
                       ("tx_pool", tx_pool, _U8), ("free", free, _I32))
    log2 = _buf_log2(buf_bytes, 256)
    n_socks = sock_port.numel()
    if not 1 <= n_socks <= _lib.RNS_UDP_MAX_SOCKS or q_first.numel() < n_socks + 1:
        raise ValueError(f"sock_port needs 1..{_lib.RNS_UDP_MAX_SOCKS} ports and q_first one entry more")
    n = rec.numel() // 32 if n_recs is None else int(n_recs)
    if not 0 <= n <= min(rec.numel() // 32, _lib.RNS_CHAIN_MAX_PACKETS):
        raise ValueError("n_recs must be a count of the 32-byte records in rec")
    for name, t in (("data", data), ("rec", rec), ("tx_pool", tx_pool)):
        if t.data_ptr() & 15:
            raise ValueError(f"{name} must start 16-byte aligned")
    n_free = free.numel()
    cap = _cap_and_ids(send_cap, n, ip_id_base, ip_id_add, dev, "send_cap must be a record count")
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    send = _new(send, "send", n, torch.uint8, dev)
    tx_blk_first, tx_head_len8, tx_pay_len16, tx_src, count = _tx_outputs(cap, dev, tx_blk_first, tx_head_len8, tx_pay_len16,
                                                                          tx_src, count)
    need = udp_send_work(n)
    work = _workspace(work, need, dev, torch.int64, f"work needs {need} bytes (udp_send_work) on {dev}")
    ptr = _nonnull(dev)
    _call("rns_tx_udp_send_pool_dev", dev, ptr(data), data.numel(), ptr(rec), n, q_first.data_ptr(), sock_port.data_ptr(),
          n_socks, ip4, ip6, ptr(tx_pool), tx_pool.numel(), log2, free.data_ptr(), n_free, cap, int(ip_id_base),
          None if ip_id_add is None else ip_id_add.data_ptr(), tx_blk_first.data_ptr(), tx_head_len8.data_ptr(),
          tx_pay_len16.data_ptr(), tx_src.data_ptr(), count.data_ptr(), send.data_ptr(), work.data_ptr(), work.numel() * 8)
    return UdpSend(send, tx_blk_first, tx_head_len8, tx_pay_len16, tx_src, count)


def send_host(data: np.ndarray, rec, q_first, sock_port, local_ipv4: bytes, local_ipv6: bytes, tx_pool: np.ndarray, free, *,
              buf_bytes: int = 512, n_recs: int | None = None, send_cap: int | None = None, ip_id_base: int = 0,
              ip_id_add: int = 0) -> UdpSend:
    """``tx_udp_send_pool`` in numpy over host arrays (``data`` / ``tx_pool`` uint8, ``rec`` a ``REC`` array or its
    bytes; ``tx_pool`` is written in place): the same sends, sockets, allocation, descriptors, counts and datagram
    bytes — the host's path for the sends the device leaves with RNS_UDPTX_NOBUF, and what the GPU tests compare
    with.  Returns a ``UdpSend`` of numpy arrays, the descriptor arrays cut to the built datagrams.  The bytes
    after a payload's end in its last buffer stay as they were."""
    B = int(buf_bytes)
    log2 = _buf_log2(B, 256)
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    rec = _np(rec, np.uint8)
    rec = rec[:rec.size // 32 * 32].view(REC)
    q = np.asarray(q_first, dtype=np.uint32).astype(np.int64)
    ports = np.asarray(sock_port).astype(np.uint16)
    n_socks = len(ports)
    if not 1 <= n_socks <= _lib.RNS_UDP_MAX_SOCKS or len(q) < n_socks + 1:
        raise ValueError(f"sock_port needs 1..{_lib.RNS_UDP_MAX_SOCKS} ports and q_first one entry more")
    n = len(rec) if n_recs is None else int(n_recs)
    tx = _TxFormHost(tx_pool, free, B, n if send_cap is None else int(send_cap), ip_id_base, ip_id_add)
    send = np.zeros(n, np.uint8)
    for k in range(min(n, int(q[n_socks]))):
        r = rec[k]
        fam, ln, at = int(r["family"]), int(r["len"]), 16 * int(r["off16"])
        if not int(r["flags"]) & _lib.RNS_UDP_QUEUED or fam not in (4, 6) or at + ln > data.size:
            continue
        s = max(int(np.searchsorted(q[:n_socks], k, side="right")) - 1, 0)
        pay = data[at:at + ln].tobytes()
        send[k], bufs, ident = tx.take(ln, fam == 4, k)
        if bufs is None:
            continue
        ulen = (8 + ln) & 0xFFFF  # udp.rs:152 `as u16`
        dst = r["ip"][:4 if fam == 4 else 16].tobytes()
        src = ip4 if fam == 4 else ip6
        udp = bytearray(int(ports[s]).to_bytes(2, "big") + int(r["sport"]).to_bytes(2, "big") + ulen.to_bytes(2, "big") + b"\0\0")
        udp[6:8] = (_fold(_be_sum(src) + _be_sum(dst) + 17 + ulen + _be_sum(udp) + _be_sum(pay)) ^ 0xFFFF).to_bytes(2, "big")
        tx.place(bufs, _ip_head_bytes(fam, 17, 8 + ln, src, dst, ident) + bytes(udp), pay)
    return UdpSend(send, *tx.result())


def udp_echo(fd_in: int, fd_out: int, rx_pool: np.ndarray, rx_free: np.ndarray, tx_pool: np.ndarray, tx_free: np.ndarray,
             ports, local_ipv4: bytes, local_ipv6: bytes, *, buf_bytes: int = 512, mru: int = 2048,
             max_pkts: int | None = None, rec_cap: int | None = None, send_cap: int | None = None, ip_id_base: int = 0,
             device: str = "cuda:0", timeout_ms: int = 0):
    """The reference's udp_echo application (udp_recv, then udp_send back to the sender) for one batch:
    ``recv_batch_pool`` from ``fd_in`` into the host ``rx_pool``, the used buffers to the device,
    ``rx_udp_demux_pool`` over the sockets bound to ``ports``, ``tx_udp_send_pool`` over its records with nothing read
    back in between, the 12-byte count read back, only the buffers ``tx_free[:count[1]]`` copied back into
    ``tx_pool``, and ``send_batch_pool`` to ``fd_out``.  Every buffer is free again when a ``send_batch_pool``
    returns (the free lists are the caller's arrays, unchanged), so the entries the device left — RNS_UDP_NOROOM
    of the demux, RNS_UDPTX_NOBUF of the send build — are then answered from the host ``rx_pool`` by ``demux_host``
    and ``send_host`` in as many further sends as the transmit pool asks for: nothing the reference would answer is
    dropped (a datagram that needs more buffers than ``tx_free`` holds raises).  Returns ``(datagrams received,
    datagrams sent, udp uint8 [n], (entries, built on the device, built on the host))``."""
    B = int(buf_bytes)
    ports = list(ports)
    n, len16, blk_first, nf = recv_batch_pool(fd_in, rx_pool, rx_free, B, mru, max_pkts, timeout_ms)
    if n == 0 or not ports:
        return n, 0, np.zeros(n, np.uint8), (0, 0, 0)
    dev = torch.device(device)
    d_rx, d_idx, to_dev = _stage_rx(rx_pool, rx_free, nf, B, dev)
    d_tx = torch.zeros(tx_pool.size, dtype=torch.uint8, device=dev)
    cap = n if rec_cap is None else int(rec_cap)
    d_rec = torch.zeros(32 * max(cap, 1), dtype=torch.uint8, device=dev)  # zeroed: a record the cut leaves is no send
    r = rx_udp_demux_pool(d_rx, d_idx, to_dev(blk_first.astype(np.uint32), np.int32), to_dev(len16, np.int16), local_ipv4,
                          local_ipv6, to_dev(port_table(ports), np.int16), len(ports), buf_bytes=B, rec_cap=cap, rec=d_rec)
    s = tx_udp_send_pool(r.data, r.rec, r.q_first, to_dev(np.array(ports, dtype=np.uint16), np.int16), local_ipv4, local_ipv6,
                         d_tx, to_dev(tx_free.astype(np.uint32), np.int32), buf_bytes=B, n_recs=cap, send_cap=send_cap,
                         ip_id_base=ip_id_base)
    sent, cnt = _send_built(fd_out, tx_pool, tx_free, d_tx, (s.tx_blk_first, s.tx_head_len8, s.tx_pay_len16, s.count), B)
    nbuilt, ids = int(cnt[0]), int(cnt[2])
    udp = _np(r.udp, np.uint8)[:n]
    entries = int(_np(r.count, np.uint32)[0])
    host_built = 0
    if nbuilt < entries:
        # the host's path: the whole batch demultiplexed uncut (the same positions), the device's datagrams struck out
        h = demux_host(rx_pool, rx_free[:nf], blk_first, len16, local_ipv4, local_ipv6, port_table(ports), len(ports), buf_bytes=B)
        done = np.zeros(entries, dtype=bool)
        done[_np(s.tx_src, np.uint32)[:nbuilt]] = True
        while not done.all():
            h.rec["flags"][:entries][done] = 0
            t = send_host(h.data, h.rec, h.q_first, ports, local_ipv4, local_ipv6, tx_pool, tx_free, buf_bytes=B,
                          ip_id_base=(int(ip_id_base) + ids) & 0xFFFF)
            k = int(t.count[0])
            if k == 0:
                raise ValueError("a datagram needs more buffers than tx_free holds")
            sent += send_batch_pool(fd_out, tx_pool, tx_free[:int(t.count[1])], t.tx_blk_first, t.tx_head_len8, t.tx_pay_len16, B)
            done[t.tx_src] = True
            ids += int(t.count[2])
            host_built += k
    return n, sent, udp, (entries, nbuilt, host_built)
