"""TCP listen responder: tcp_input's SYN-ACKs and RSTs built on the device.

When a segment's key is not in PORT_MAP, tcp_input (tcp.rs:579-615) answers it with RST|ACK — unless it is a
SYN to a port with a listen socket: then handle_new_connection (tcp.rs:894-936) creates the socket, answers
SYN|ACK and inserts it, so every later segment of that key finds it.  ``rx_tcp_listen_pool`` does that for a
batch the placement has decoded (``place.rx_tcp_place_pool``'s meta records over the same pool form): every
unmatched segment is classified, the replies are built, both checksums filled, into 64-byte slots in batch
order, and every new connection leaves an accept record — its key and the new socket's state
(rns_rx_tcp_listen_pool_dev).  ``listen_host`` is the same function in numpy over a host pool — the host's
path for what the device leaves (``RNS_CONN_NOBUF``, ``RNS_CONN_HOST``, ``RNS_CONN_LATER``) and what the GPU
tests compare with —, ``tcp_listen`` verify + placement + responder on one stream, and ``accept_merge`` the
step that makes the next batch's segments of the new connections match in the placement.

The functions are re-exported by ``batch``, whose argument checks they use.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .batch import _I32, _U8, _U16, _call, _local_addrs, _nonnull, _require_cuda, _work_bytes, _workspace
from .flow import FLOW_DTYPE
from .place import KEY_DTYPE, META_DTYPE, _keys, rx_tcp_place_pool
from .pool import _be_sum, _buf_log2, _fold, _new, _np, _pool_batch

ACCEPT_DTYPE = np.dtype([("key", KEY_DTYPE), ("flow", FLOW_DTYPE), ("src", "<u4"), ("listener", "<u2"), ("mss", "<u2")])
assert ACCEPT_DTYPE.itemsize == 72  # rns_tcp_accept
REPLY_SLOT = 64  # bytes per reply slot
_M32 = 0xFFFFFFFF
_SYN_OPTIONS = bytes([2, 4, 0x05, 0xDC])  # send_packet's MSS 1500 (tcp.rs:431)


class TcpListen(NamedTuple):
    """What a responder call leaves: torch tensors from ``rx_tcp_listen_pool``, numpy arrays from ``listen_host``."""
    conn: object      # uint8 [n]: RNS_CONN_* bits
    out: object       # uint8 [reply_cap * 64]: the reply slots (None with reply_cap 0)
    rep_src: object   # uint32 [reply_cap]: the answered datagram's index
    rep_len8: object  # uint8 [reply_cap]: 40 / 60 (RST), 44 / 64 (SYN-ACK)
    accept: object    # the accept records (ACCEPT_DTYPE on the host; uint8 [reply_cap * 72] on the device)
    count: object     # uint32 [3]: replies, IPv4 replies, accepts — as if reply_cap were unbounded


def key_hash(key6) -> int:
    """The flow table's hash (rns_rx_flow_table_build) of a key's six little-endian dwords: the slot a key's probe
    starts at, in the placement's table and in the responder's, is ``key_hash(k) & (slots - 1)``."""
    h = 0x9E3779B9
    for w in key6:
        h = ((h ^ int(w)) * 0x85EBCA6B) & _M32
        h ^= h >> 15
    return h


def listen_slots(n_pkts: int) -> int:
    """Slots of the responder's key table for ``n_pkts`` datagrams: a power of two >= 2 * n_pkts and >= 64."""
    s = 64
    while s < 2 * int(n_pkts):
        s <<= 1
    return s


def listen_work(n_pkts: int) -> int:
    """Bytes of workspace ``rx_tcp_listen_pool`` needs for ``n_pkts`` datagrams (rns_rx_tcp_listen_work)."""
    return _work_bytes("rns_rx_tcp_listen_work", int(n_pkts))


def rx_tcp_listen_pool(pool: torch.Tensor, buf_idx: torch.Tensor, blk_first: torch.Tensor, len16: torch.Tensor,
                       local_ipv4: bytes, local_ipv6: bytes, meta: torch.Tensor, listen_tbl: torch.Tensor | None,
                       n_listen: int, iss: torch.Tensor | None, *, buf_bytes: int = 512, reply_cap: int | None = None,
                       ip_id_base: int = 0, ip_id_add: torch.Tensor | None = None, out: torch.Tensor | None = None,
                       rep_src: torch.Tensor | None = None, rep_len8: torch.Tensor | None = None,
                       accept: torch.Tensor | None = None, count: torch.Tensor | None = None,
                       conn: torch.Tensor | None = None, work: torch.Tensor | None = None) -> TcpListen:
    """TCP listen responder over pool buffers (rns_rx_tcp_listen_pool_dev).  ``pool`` / ``buf_idx`` / ``blk_first`` /
    ``len16`` and ``meta`` as ``rx_tcp_place_pool`` took and left them (``buf_bytes`` a power of two in 128..32768);
    ``listen_tbl`` = ``udp.port_table(listening ports)`` on the device as int16 / uint16 [65536] (None with
    ``n_listen`` 0); ``iss`` int32 [>= reply_cap]: accept a's initial send sequence number.  Every segment the
    placement decoded without a flow gets its RNS_CONN_* bits in ``conn``; reply k (the k-th RST or SYN-ACK in batch
    order, IPv4 id = ``ip_id_base`` + ``ip_id_add[0]`` + the IPv4 replies before it) lies finished in
    ``out[64 * k : 64 * k + rep_len8[k]]`` with ``rep_src[k]`` its datagram, and accept a (the a-th new connection)
    in ``accept[72 * a :]`` (``ACCEPT_DTYPE``).  ``reply_cap`` (default: one per datagram) bounds what is written;
    0 counts and classifies only.  ``count`` = (replies, IPv4 replies, accepts), int32 on the device: nothing is
    synchronised here.  Returns a ``TcpListen`` of device tensors."""
    dev, log2, n, nf = _pool_batch(pool, buf_idx, blk_first, len16, buf_bytes, 128, ("meta", meta, _U8))
    if meta.numel() != n * META_DTYPE.itemsize:
        raise ValueError("meta must hold one 24-byte record per datagram")
    if pool.data_ptr() & 15:
        raise ValueError("the pool must start 16-byte aligned")
    n_listen = int(n_listen)
    if not 0 <= n_listen <= _lib.RNS_UDP_MAX_SOCKS:
        raise ValueError(f"n_listen must be at most {_lib.RNS_UDP_MAX_SOCKS}")
    if n_listen:
        _require_cuda(listen_tbl, "listen_tbl", _U16)
        if listen_tbl.numel() != 65536 or listen_tbl.device != dev:
            raise ValueError(f"listen_tbl must have 65536 entries on {dev}")
    cap = n if reply_cap is None else int(reply_cap)
    if not 0 <= cap <= _lib.RNS_CHAIN_MAX_PACKETS or not 0 <= int(ip_id_base) <= 0xFFFF:
        raise ValueError("reply_cap must be a datagram count and ip_id_base a u16")
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    if ip_id_add is not None:
        _require_cuda(ip_id_add, "ip_id_add", _I32)
        if ip_id_add.numel() < 1 or ip_id_add.device != dev:
            raise ValueError(f"ip_id_add must be an int32 tensor (at least 1 entry) on {dev}")
    if cap:
        _require_cuda(iss, "iss", _I32)
        if iss.numel() < cap or iss.device != dev:
            raise ValueError(f"iss needs one entry per reply slot ({cap}) on {dev}")
        out = _new(out, "out", REPLY_SLOT * cap, torch.uint8, dev)
        rep_src = _new(rep_src, "rep_src", cap, torch.int32, dev)
        rep_len8 = _new(rep_len8, "rep_len8", cap, torch.uint8, dev)
        accept = _new(accept, "accept", ACCEPT_DTYPE.itemsize * cap, torch.uint8, dev)
    count = _new(count, "count", 3, torch.int32, dev)
    conn = _new(conn, "conn", n, torch.uint8, dev)
    need = listen_work(n)
    work = _workspace(work, need, dev, torch.int64, f"work needs {need} bytes (listen_work) on {dev}")
    ptr = _nonnull(dev)
    opt = lambda t: t.data_ptr() if cap else None  # noqa: E731
    _call("rns_rx_tcp_listen_pool_dev", dev, pool.data_ptr(), pool.numel(), log2, buf_idx.data_ptr(), nf, ptr(blk_first),
          ptr(len16), n, ip4, ip6, ptr(meta), listen_tbl.data_ptr() if n_listen else None, n_listen, opt(iss),
          int(ip_id_base), None if ip_id_add is None else ip_id_add.data_ptr(), opt(out), cap, opt(rep_src), opt(rep_len8),
          opt(accept), count.data_ptr(), ptr(conn), work.data_ptr(), work.numel() * 8)
    return TcpListen(conn, out, rep_src, rep_len8, accept, count)


# ---------------------------------------------------------------------------
# the same on the host
# ---------------------------------------------------------------------------
def _options_host(opts: bytes):
    """parse_options (tcp.rs:856-892): max_segment_size, or None where the reference does not return."""
    mss, at, n = 0, 0, len(opts)
    while at < n:
        t = opts[at]
        if t == 0:
            break
        if t == 1:
            at += 1
            continue
        if at + 1 >= n:
            return None  # header[opt_offset + 1] panics
        ln = opts[at + 1]
        if t == 2:
            if at + 4 > n:
                return None  # header[opt_offset + 2..opt_offset + 4] panics
            mss = (opts[at + 2] << 8) | opts[at + 3]
        if ln == 0:
            return None  # loops for ever
        at += ln
    return mss


def reply_host(v6: bool, local: bytes, remote: bytes, sport: int, dport: int, seq: int, ack: int, syn: bool, ip_id: int) -> bytes:
    """One reply as tcp_output -> ip_output builds it: from the local address and ``sport`` to ``remote``:``dport``."""
    opts = _SYN_OPTIONS if syn else b""
    tcp = bytearray(sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + (seq & _M32).to_bytes(4, "big") +
                    (ack & _M32).to_bytes(4, "big") + bytes([(5 + len(opts) // 4) << 4, 0x12 if syn else 0x14]) +
                    (0xFFFF if syn else 0).to_bytes(2, "big") + bytes(4) + opts)
    tcp[16:18] = (_fold(_be_sum(local) + _be_sum(remote) + 6 + len(tcp) + _be_sum(tcp)) ^ 0xFFFF).to_bytes(2, "big")
    if v6:
        return bytes([0x60, 0, 0, 0]) + len(tcp).to_bytes(2, "big") + bytes([6, 64]) + local + remote + bytes(tcp)
    ip = bytearray(bytes([0x45, 0]) + (20 + len(tcp)).to_bytes(2, "big") + (ip_id & 0xFFFF).to_bytes(2, "big") +
                   bytes([0, 0, 64, 6, 0, 0]) + local + remote)
    ip[10:12] = (_fold(_be_sum(ip)) ^ 0xFFFF).to_bytes(2, "big")
    return bytes(ip) + bytes(tcp)


def listen_host(rx_pool: np.ndarray, buf_idx, blk_first, len16, local_ipv4: bytes, local_ipv6: bytes, meta, listen_tbl,
                n_listen: int, iss, *, buf_bytes: int = 512, reply_cap: int | None = None, ip_id_base: int = 0,
                ip_id_add: int = 0, out: np.ndarray | None = None, rep_src: np.ndarray | None = None,
                rep_len8: np.ndarray | None = None, accept: np.ndarray | None = None) -> TcpListen:
    """``rx_tcp_listen_pool`` in numpy over a host pool (uint8 array) and the placement's records (``META_DTYPE`` or
    their bytes): the same classes, ranks, ids, reply bytes, accept records and counts — the host's path for what
    the device leaves, and what the GPU tests compare with.  ``out`` (uint8), ``rep_src`` (uint32), ``rep_len8``
    (uint8) and ``accept`` (``ACCEPT_DTYPE``) are written in place where given and keep every byte the call does not
    write.  Returns a ``TcpListen`` of numpy arrays."""
    B = int(buf_bytes)
    log2 = _buf_log2(B, 128)
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    meta = _np(meta, np.uint8).view(META_DTYPE)
    buf_idx = np.asarray(buf_idx, dtype=np.uint32).astype(np.int64)
    blk_first = np.asarray(blk_first, dtype=np.uint32).astype(np.int64)
    len16 = np.asarray(len16, dtype=np.uint16).astype(np.int64)
    n, n_listen = len(len16), int(n_listen)
    if len(meta) != n:
        raise ValueError("meta must hold one record per datagram")
    if not 0 <= n_listen <= _lib.RNS_UDP_MAX_SOCKS:
        raise ValueError(f"n_listen must be at most {_lib.RNS_UDP_MAX_SOCKS}")
    tbl = np.asarray(listen_tbl, dtype=np.uint16) if n_listen else None
    cap = n if reply_cap is None else int(reply_cap)
    iss = np.asarray(iss if iss is not None else [], dtype=np.int64) & _M32
    out = np.zeros(REPLY_SLOT * cap, np.uint8) if out is None else out
    rep_src = np.zeros(cap, np.uint32) if rep_src is None else rep_src
    rep_len8 = np.zeros(cap, np.uint8) if rep_len8 is None else rep_len8
    accept = np.zeros(cap, ACCEPT_DTYPE) if accept is None else accept
    conn = np.zeros(n, np.uint8)
    nfr = -(-len16 // B)
    opened = {}  # key -> the index of its first candidate: PORT_MAP's growth within the batch
    R = V = A = 0
    for i in range(n):
        m = meta[i]
        if (int(m["place"]) & (_lib.RNS_PLACE_TCP | _lib.RNS_PLACE_FLOW)) != _lib.RNS_PLACE_TCP:
            continue
        # the record's claims, checked again before a byte of the pool is read
        T, nf = int(len16[i]), int(nfr[i])
        gi = int(blk_first[i // 64]) + int(nfr[64 * (i // 64):i].sum())
        if nf == 0 or gi + nf > len(buf_idx) or T < 16:
            continue
        s0, len0 = int(buf_idx[gi]) << log2, min(T, B)
        if s0 + len0 > rx_pool.size:
            continue
        d = rx_pool[s0:s0 + len0].tobytes()
        ver, ip_hdr, tcp_hdr = d[0] >> 4, int(m["ip_hdr"]), int(m["tcp_hdr"])
        if ver not in (4, 6) or ip_hdr != (40 if ver == 6 else (d[0] & 0xF) * 4) or ip_hdr < 20 or not 20 <= tcp_hdr <= 60 or \
                tcp_hdr & 3 or ip_hdr + tcp_hdr > T:
            continue
        v6 = ver == 6
        remote = d[8:24] if v6 else d[12:16]
        sport, dport, seq = int(m["sport"]), int(m["dport"]), int(m["seq"])
        key = (remote, sport, dport)
        conn[i] = _lib.RNS_CONN_UNMATCHED
        lst = int(tbl[dport]) if n_listen else _lib.RNS_UDP_NO_SOCK
        cand = bool(int(m["flags"]) & 0x02) and lst < n_listen
        if key in opened:
            conn[i] |= _lib.RNS_CONN_LATER  # the socket datagram opened[key] created takes it
            continue
        mss = None
        if cand:
            opened[key] = i
            mss = _options_host(d[ip_hdr + 20:ip_hdr + tcp_hdr])
            if mss is None:
                conn[i] |= _lib.RNS_CONN_HOST
                continue
        conn[i] |= _lib.RNS_CONN_SYN if cand else _lib.RNS_CONN_RST
        k, a = R, A
        R, A = R + 1, A + (1 if cand else 0)
        if not v6:
            V += 1
        if k >= cap:
            conn[i] |= _lib.RNS_CONN_NOBUF
            continue
        conn[i] |= _lib.RNS_CONN_BUILT
        head = reply_host(v6, ip6 if v6 else ip4, remote, dport, sport, int(iss[a]) if cand else 1, seq + 1, cand,
                          int(ip_id_base) + int(ip_id_add) + V - 1)
        out[REPLY_SLOT * k:REPLY_SLOT * k + len(head)] = np.frombuffer(head, dtype=np.uint8)
        rep_src[k], rep_len8[k] = i, len(head)
        if cand:
            r = np.zeros(1, ACCEPT_DTYPE)[0]
            r["key"]["ip"][:len(remote)] = np.frombuffer(remote, dtype=np.uint8)
            r["key"]["sport"], r["key"]["dport"], r["key"]["family"] = sport, dport, 6 if v6 else 4
            f = r["flow"]
            f["rcv_nxt"] = f["rcv_max"] = (seq + 1) & _M32
            f["snd_una"] = f["snd_wl1"] = seq  # send_unacked = seq_num (tcp.rs:917): the peer's number, as the reference has it
            f["snd_nxt"], f["snd_wl2"], f["snd_wnd"] = int(iss[a]), int(m["ack"]), int(m["window"])
            f["state"] = _lib.RNS_TCP_SYN_RECEIVED
            r["src"], r["listener"], r["mss"] = i, lst, mss
            accept[a] = r
    return TcpListen(conn, out, rep_src, rep_len8, accept, np.array([R, V, A], dtype=np.uint32))


# ---------------------------------------------------------------------------
# verify + placement + responder on one stream, and the step to the next batch
# ---------------------------------------------------------------------------
def tcp_listen(pool: torch.Tensor, buf_idx: torch.Tensor, blk_first: torch.Tensor, len16: torch.Tensor, local_ipv4: bytes,
               local_ipv6: bytes, table: torch.Tensor, next_seq: torch.Tensor, win_off: torch.Tensor, win_len: torch.Tensor,
               stream: torch.Tensor, listen_tbl: torch.Tensor | None, n_listen: int, iss: torch.Tensor | None, *,
               buf_bytes: int = 512, reply_cap: int | None = None, ip_id_base: int = 0,
               ip_id_add: torch.Tensor | None = None):
    """``rx_tcp_place_pool`` (the pool verify and the placement) and then ``rx_tcp_listen_pool`` over its records, on
    the current stream with nothing read back in between.  Returns ``(status, meta, TcpListen)``: the reply slots
    ``out[64 * k : 64 * k + rep_len8[k]]`` are ready for ``batch.send_batch`` (rns_io_send_batch), the accept
    records for ``accept_merge``, and ``conn`` says what is left to the host."""
    status, _, meta = rx_tcp_place_pool(pool, buf_idx, blk_first, len16, local_ipv4, local_ipv6, table, next_seq, win_off,
                                        win_len, stream, buf_bytes=buf_bytes)
    r = rx_tcp_listen_pool(pool, buf_idx, blk_first, len16, local_ipv4, local_ipv6, meta.reshape(-1), listen_tbl, n_listen,
                           iss, buf_bytes=buf_bytes, reply_cap=reply_cap, ip_id_base=ip_id_base, ip_id_add=ip_id_add)
    return status, meta, r


def accept_merge(accept, keys=None, flows=None, next_seq=None, win_off=None, win_len=None, *, new_win_off=None,
                 new_win_len: int = 0):
    """The accept records (``ACCEPT_DTYPE`` or their bytes, cut to the records written) appended to the flows the
    host already has: returns ``(keys, flows, next_seq, win_off, win_len)`` — ``KEY_DTYPE``, ``FLOW_DTYPE``, uint32,
    uint64, uint32 — with new flow ``len(keys) + a`` = accept a: its key, its state, next_seq = its rcv_nxt and the
    window ``new_win_off[a]`` (default 0) of ``new_win_len`` bytes.  ``place.rx_flow_table(keys)`` is then the next
    batch's table, in which the new connections' segments match; their state is RNS_TCP_SYN_RECEIVED: the flow
    update stops them with RNS_STOP_STATE, ``conn.rx_tcp_conn_update`` completes their handshake on the device."""
    acc = _np(accept, np.uint8).view(ACCEPT_DTYPE)
    k0 = _keys([] if keys is None else keys)  # (a KEY_DTYPE array or (address, sport, dport) tuples, as rx_flow_table takes them)
    f0 = np.zeros(0, FLOW_DTYPE) if flows is None else _np(flows, np.uint8).view(FLOW_DTYPE)
    old = len(k0)
    cols = []
    for name, a, t in (("next_seq", next_seq, np.uint32), ("win_off", win_off, np.uint64), ("win_len", win_len, np.uint32)):
        a = np.zeros(old, t) if a is None else np.asarray(a).astype(t).reshape(-1)
        if len(a) != old:
            raise ValueError(f"{name} needs one entry per flow")
        cols.append(a)
    if len(f0) != old:
        raise ValueError("flows needs one record per key")
    off = np.zeros(len(acc), np.uint64) if new_win_off is None else np.asarray(new_win_off).astype(np.uint64).reshape(-1)
    if len(off) != len(acc):
        raise ValueError("new_win_off needs one entry per accept record")
    return (np.concatenate([k0, acc["key"]]), np.concatenate([f0, acc["flow"]]),
            np.concatenate([cols[0], acc["flow"]["rcv_nxt"].astype(np.uint32)]), np.concatenate([cols[1], off]),
            np.concatenate([cols[2], np.full(len(acc), int(new_win_len), np.uint32)]))
