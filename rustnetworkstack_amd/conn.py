"""TCP connection update, control-segment build and close step: tcp_input's handshake and close on the device.

``flow.rx_tcp_flow_update`` advances a socket that is Established over plain data and ACK segments.
``rx_tcp_conn_update`` is the same walk with the rest of tcp_input as its step (rns_rx_tcp_conn_update_dev,
tcp.rs:622-835): the RST hack, the data branch of a socket that is not Established, the ACK field and the state
machine, so the accept records of ``listen.rx_tcp_listen_pool`` (SynReceived) go on through the handshake's third
segment, the requests, each FIN, RST and last ACK.  Every datagram leaves a 16-byte control record (``CTL_DTYPE``):
what was done and, where send_packet ran, the segment it built.  ``tx_tcp_ctl_build`` builds and finalizes those
segments in batch order (rns_tx_tcp_ctl_build_dev) and ``tx_tcp_close`` is tcp_close for a batch of sockets
(rns_tx_tcp_close_dev), whose FIN|ACK records go through the same build.  ``conn_update_host``, ``ctl_heads_host``
and ``close_host`` are the same functions on the host, record for record — the host's path for what the device
leaves —, and ``tcp_conn`` is placement -> listen responder -> connection update -> control build on one stream.

The functions are re-exported by ``batch``, whose argument checks they use.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .batch import _I32, _U8, _bytes_of, _call, _ptr as ptr, _require_cuda, _seq_gt, _work_bytes, _workspace
from .flow import FLOW_DTYPE, RES_DTYPE
from .place import META_DTYPE
from .pool import _be_sum, _fold

# rns_tcp_ctl (rns_checksum.h)
CTL_DTYPE = np.dtype([("flow", "<u4"), ("seq", "<u4"), ("ack_num", "<u4"), ("window", "<u2"), ("flags", "u1"), ("act", "u1")])
assert CTL_DTYPE.itemsize == 16
CTL_SLOT = 64  # bytes per slot of tx_tcp_ctl_build's output
_M32 = 0xFFFFFFFF
_FIN, _SYN, _RST, _ACK = 0x01, 0x02, 0x04, 0x10
_FIN_ACKING = (_lib.RNS_TCP_FIN_WAIT1, _lib.RNS_TCP_FIN_WAIT2, _lib.RNS_TCP_CLOSING, _lib.RNS_TCP_CLOSE_WAIT)


def conn_work(n_pkts: int, n_flows: int) -> int:
    """Bytes of workspace ``rx_tcp_conn_update`` (and ``tx_tcp_ctl_build`` over its records) needs
    (rns_rx_tcp_conn_update_work)."""
    return _work_bytes("rns_rx_tcp_conn_update_work", n_pkts, n_flows)


def rx_tcp_conn_update(meta: torch.Tensor, flows: torch.Tensor, pend: torch.Tensor | None, *, pend_cap: int,
                       flows_out: torch.Tensor | None = None, pend_out: torch.Tensor | None = None,
                       ctl: torch.Tensor | None = None, res: torch.Tensor | None = None,
                       work: torch.Tensor | None = None):
    """TCP connection update (rns_rx_tcp_conn_update_dev): ``flow.rx_tcp_flow_update``'s arguments, with ``ctl``
    (uint8 n x 16, ``CTL_DTYPE``) where that has ``seg``.  Returns ``(flows_out, pend_out, ctl, res)``."""
    _require_cuda(meta, "meta", _U8)
    dev = meta.device
    if meta.numel() % META_DTYPE.itemsize:
        raise ValueError("meta must hold whole 24-byte records")
    n = meta.numel() // META_DTYPE.itemsize
    _require_cuda(flows, "flows", _U8)
    nfl = flows.numel() // FLOW_DTYPE.itemsize
    _bytes_of(flows, "flows", nfl, FLOW_DTYPE.itemsize, dev)
    pend_cap = int(pend_cap)
    if pend_cap < 0 or pend_cap >= 2 ** 32 or n > _lib.RNS_CHAIN_MAX_PACKETS or nfl >= 2 ** 31:
        raise ValueError("pend_cap is a u32; at most RNS_CHAIN_MAX_PACKETS datagrams and 2^31-1 flows")
    if pend_cap:
        if pend is None:
            raise ValueError("pend is needed with pend_cap > 0")
        _require_cuda(pend, "pend", _I32)
        if pend.numel() != 2 * pend_cap * nfl or pend.device != dev:
            raise ValueError("pend must hold pend_cap (seq, len) pairs per flow on the meta's device")
        if pend_out is None:
            pend_out = torch.empty_like(pend)
        else:
            _require_cuda(pend_out, "pend_out", _I32)
            if pend_out.numel() != pend.numel() or pend_out.device != dev:
                raise ValueError("pend_out must match pend")
    if flows_out is None:
        flows_out = torch.empty_like(flows)
    else:
        _bytes_of(flows_out, "flows_out", nfl, FLOW_DTYPE.itemsize, dev)
    if ctl is None:
        ctl = torch.empty((n, CTL_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    else:
        _bytes_of(ctl, "ctl", n, CTL_DTYPE.itemsize, dev)
    if res is None:
        res = torch.empty((nfl, RES_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    else:
        _bytes_of(res, "res", nfl, RES_DTYPE.itemsize, dev)
    work = _workspace(work, conn_work(n, nfl), dev)
    _call("rns_rx_tcp_conn_update_dev", dev, ptr(meta), n, nfl, ptr(flows), ptr(pend) if pend_cap else None, pend_cap,
          ptr(flows_out), ptr(pend_out) if pend_cap else None, ptr(ctl), ptr(res), work.data_ptr(), work.numel())
    return flows_out, pend_out, ctl, res


def tx_tcp_ctl_build(ctl: torch.Tensor, n_flows: int, tmpl: torch.Tensor, head_len8: torch.Tensor, ip_id_base: int, *,
                     out_cap: int, ip_id_add: torch.Tensor | None = None, tmpl_stride: int | None = None,
                     out: torch.Tensor | None = None, src: torch.Tensor | None = None, len8: torch.Tensor | None = None,
                     count: torch.Tensor | None = None, work: torch.Tensor | None = None):
    """Control-segment build (rns_tx_tcp_ctl_build_dev): ``ctl`` uint8 n x 16 (``CTL_DTYPE``) from the update, the
    close step or the host; ``tmpl`` / ``head_len8`` as ``flow.tx_ack_build`` takes them, one per flow; ``ip_id_add`` an
    optional int32 device tensor whose first entry is added to ``ip_id_base``.  Returns ``(out, src, len8, count)``:
    ``out`` uint8 ``out_cap`` x 64 (only the heads' bytes are written), ``src`` int32 and ``len8`` uint8 per slot,
    ``count`` int32 [segments, IPv4 ones].  ``out_cap == 0`` counts only."""
    _require_cuda(ctl, "ctl", _U8)
    dev = ctl.device
    if ctl.numel() % CTL_DTYPE.itemsize:
        raise ValueError("ctl must hold whole 16-byte records")
    n, nfl = ctl.numel() // CTL_DTYPE.itemsize, int(n_flows)
    _require_cuda(tmpl, "tmpl", _U8)
    _require_cuda(head_len8, "head_len8", _U8)
    if tmpl_stride is None:
        tmpl_stride = int(tmpl.shape[1]) if tmpl.dim() == 2 else 0
    if head_len8.numel() != nfl or (nfl and (tmpl_stride <= 0 or tmpl.numel() < nfl * tmpl_stride)):
        raise ValueError("head_len8 and tmpl need one entry / tmpl_stride bytes per flow")
    if tmpl.device != dev or head_len8.device != dev:
        raise ValueError("tmpl and head_len8 must be on the records' device")
    out_cap = int(out_cap)
    if not 0 <= out_cap < 2 ** 32 or not 0 <= int(ip_id_base) <= 0xFFFF or n > _lib.RNS_CHAIN_MAX_PACKETS:
        raise ValueError("out_cap is a u32, ip_id_base a u16, and at most RNS_CHAIN_MAX_PACKETS records")
    if ip_id_add is not None:
        _require_cuda(ip_id_add, "ip_id_add", _I32)
        if ip_id_add.numel() < 1 or ip_id_add.device != dev:
            raise ValueError(f"ip_id_add must be an int32 tensor (at least 1 entry) on {dev}")
    if out_cap:
        if out is None:
            out = torch.empty((out_cap, CTL_SLOT), dtype=torch.uint8, device=dev)
        if src is None:
            src = torch.empty(out_cap, dtype=torch.int32, device=dev)
        if len8 is None:
            len8 = torch.empty(out_cap, dtype=torch.uint8, device=dev)
        _bytes_of(out, "out", out_cap, CTL_SLOT, dev)
        _require_cuda(src, "src", _I32)
        _bytes_of(len8, "len8", out_cap, 1, dev)
        if src.numel() != out_cap or src.device != dev:
            raise ValueError("src needs one entry per slot on the records' device")
    if count is None:
        count = torch.empty(2, dtype=torch.int32, device=dev)
    else:
        _require_cuda(count, "count", _I32)
        if count.numel() != 2 or count.device != dev:
            raise ValueError("count holds two int32 entries on the records' device")
    work = _workspace(work, _work_bytes("rns_tx_tcp_ctl_build_work", n), dev)
    _call("rns_tx_tcp_ctl_build_dev", dev, ptr(ctl), n, nfl, ptr(tmpl), tmpl_stride, ptr(head_len8), int(ip_id_base),
          None if ip_id_add is None else ip_id_add.data_ptr(), work.data_ptr(), work.numel(),
          ptr(out) if out_cap else None, out_cap, ptr(src) if out_cap else None, ptr(len8) if out_cap else None,
          count.data_ptr())
    return out, src, len8, count


def tx_tcp_close(flows: torch.Tensor, op: torch.Tensor, *, flows_out: torch.Tensor | None = None,
                 ctl: torch.Tensor | None = None):
    """tcp_close for a batch of sockets (rns_tx_tcp_close_dev): ``flows`` uint8 n_flows x 40, ``op`` uint8 per flow
    (1: close).  ``flows_out`` may be ``flows`` itself (in place); a new tensor by default.  Returns ``(flows_out,
    ctl)``: ``ctl`` uint8 n_flows x 16, a FIN|ACK record for every flow that sends, zero for the others."""
    _require_cuda(flows, "flows", _U8)
    dev = flows.device
    nfl = flows.numel() // FLOW_DTYPE.itemsize
    _bytes_of(flows, "flows", nfl, FLOW_DTYPE.itemsize, dev)
    _bytes_of(op, "op", nfl, 1, dev)
    if nfl >= 2 ** 31:
        raise ValueError("at most 2^31-1 flows")
    if flows_out is None:
        flows_out = torch.empty_like(flows)
    else:
        _bytes_of(flows_out, "flows_out", nfl, FLOW_DTYPE.itemsize, dev)
    if ctl is None:
        ctl = torch.empty((nfl, CTL_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    else:
        _bytes_of(ctl, "ctl", nfl, CTL_DTYPE.itemsize, dev)
    _call("rns_tx_tcp_close_dev", dev, ptr(flows), ptr(flows_out), nfl, ptr(op), ptr(ctl))
    return flows_out, ctl


# ---------------------------------------------------------------------------
# the same on the host
# ---------------------------------------------------------------------------
def _seq_le(a: int, b: int) -> bool:
    return not _seq_gt(a, b)


def _send(s: dict, flags: int):
    """send_packet (tcp.rs:402-447) for an empty packet: (seq, ack_num, window, flags) in the state ``s`` has now."""
    plus = 1 if s["state"] in _FIN_ACKING and s["rcv_max"] == s["rcv_nxt"] else 0
    return s["snd_nxt"], (s["rcv_nxt"] + plus) & _M32, (0xFFFF - (s["rq_len"] & 0xFFFF)) & 0xFFFF, flags


def _stop_of(s: dict, rec, n_pend: int, cap: int) -> int:
    flags, pay, st = int(rec["flags"]), int(rec["pay_len"]), s["state"]
    if st >= _lib.RNS_TCP_SYN_SENT:
        return _lib.RNS_STOP_STATE
    if int(rec["tcp_hdr"]) != 20:
        return _lib.RNS_STOP_OPTIONS
    if flags & _RST:
        return 0
    if flags & _SYN and pay:
        return _lib.RNS_STOP_FLAGS
    if int(rec["place"]) & _lib.RNS_PLACE_OUTSIDE:
        return _lib.RNS_STOP_OUTSIDE
    if pay and int(rec["seq"]) != s["rcv_nxt"] and n_pend >= cap:
        return _lib.RNS_STOP_PEND
    if pay and flags & _FIN:
        acks_fin = bool(flags & _ACK) and int(rec["ack"]) == (s["snd_nxt"] + 1) & _M32
        if st == _lib.RNS_TCP_FIN_WAIT2 or (st == _lib.RNS_TCP_FIN_WAIT1 and not acks_fin):
            return _lib.RNS_STOP_TWICE
    return 0


def conn_update_host(meta_records, flows, pend, pend_cap: int):
    """``rx_tcp_conn_update`` on the host, with the same outputs record for record: ``meta_records`` a META_DTYPE
    array, ``flows`` a FLOW_DTYPE array, ``pend`` a uint32 array of n_flows x pend_cap x 2 (or None with ``pend_cap ==
    0``).  Returns ``(flows_out, pend_out, ctl, res)`` as new numpy arrays (``pend_out``'s entries past n_pend are
    the input's).  It is the host's path for everything the device stops at."""
    m = np.asarray(meta_records).reshape(-1)
    flows = np.asarray(flows).reshape(-1)
    if m.dtype != META_DTYPE or flows.dtype != FLOW_DTYPE:
        raise TypeError("meta_records must be META_DTYPE records and flows FLOW_DTYPE records")
    L = _lib
    n, nfl, cap = m.size, flows.size, int(pend_cap)
    pend_in = (np.zeros((nfl, 0, 2), dtype=np.uint32) if cap == 0 or pend is None
               else np.asarray(pend, dtype=np.uint32).reshape(nfl, cap, 2))
    out, pend_out = flows.copy(), pend_in.copy()
    ctl, res = np.zeros(n, dtype=CTL_DTYPE), np.zeros(nfl, dtype=RES_DTYPE)
    res["stop"] = _M32
    member = ((m["place"] & L.RNS_PLACE_FLOW) != 0) & (m["flow"] < nfl)
    order = np.flatnonzero(member)
    order = order[np.argsort(m["flow"][order], kind="stable")]          # per flow, ascending datagram index
    bounds = np.searchsorted(m["flow"][order], np.arange(nfl + 1))
    for f in range(nfl):
        idx = order[bounds[f]:bounds[f + 1]]
        r = res[f]
        r["n_segs"] = idx.size
        if idx.size == 0:
            continue
        s = {k: int(flows[f][k]) for k in FLOW_DTYPE.names}
        if idx.size > L.RNS_FLOW_MAX_SEGS:
            r["stop"], r["why"] = idx[0], L.RNS_STOP_MANY
            continue
        if s["n_pend"] > cap:
            r["stop"], r["why"] = idx[0], L.RNS_STOP_STATE
            continue
        pl = [(int(a), int(b)) for a, b in pend_in[f, :s["n_pend"]]]
        readable = acked = n_sent = events = consumed = 0
        for i in idx:
            rec = m[i]
            why = _stop_of(s, rec, len(pl), cap)
            if why:
                r["stop"], r["why"] = i, why
                break
            flags, seq, ack, pay = int(rec["flags"]), int(rec["seq"]), int(rec["ack"]), int(rec["pay_len"])
            st, act, sent = s["state"], L.RNS_CTL_CONSUMED, None
            consumed += 1
            if flags & _RST:                                             # A, tcp.rs:635-640
                s["state"] = L.RNS_TCP_CLOSED
                events |= L.RNS_EV_STATE
                ctl[i] = (f, 0, 0, 0, 0, act | L.RNS_CTL_RESET | L.RNS_CTL_STATE)
                continue
            if pay:                                                      # B, tcp.rs:642-696
                end = (seq + pay) & _M32
                if not _seq_gt(s["rcv_max"], end):
                    s["rcv_max"] = end
                got = 0
                if seq == s["rcv_nxt"]:                                  # add_packet, tcp.rs:488-516
                    got = pay
                    s["rcv_nxt"] = (s["rcv_nxt"] + pay) & _M32
                    k = 0
                    while k < len(pl):
                        if _seq_gt(seq, pl[k][0]):
                            del pl[k]
                        elif pl[k][0] == s["rcv_nxt"]:
                            _, ln = pl.pop(k)
                            s["rcv_nxt"] = (s["rcv_nxt"] + ln) & _M32
                            got += ln
                            k = 0
                        else:
                            k += 1
                else:
                    pl.append((seq, pay))
                s["rq_len"] = (s["rq_len"] + got) & _M32
                readable = (readable + got) & _M32
                if st == L.RNS_TCP_ESTABLISHED:
                    s["delayed_acks"] = (s["delayed_acks"] + 1) & 0xFFFF
                    if s["delayed_acks"] >= 5 or flags & _FIN:
                        s["delayed_acks"] = s["ack_timer"] = 0
                        sent = _send(s, _ACK)
                    elif s["ack_timer"] == 0:
                        s["ack_timer"] = 1
                        act |= L.RNS_CTL_ACK_TIMER
                else:
                    s["ack_timer"] = 0
                    sent = _send(s, _ACK)
            if flags & _ACK and st not in (L.RNS_TCP_CLOSED, L.RNS_TCP_TIME_WAIT):   # C, tcp.rs:698-740
                if _seq_gt(ack, s["snd_una"]) and _seq_le(ack, s["snd_nxt"]):
                    acked = (acked + ack - s["snd_una"]) & _M32
                    s["snd_una"] = ack
                if _seq_le(s["snd_una"], ack) and _seq_le(ack, s["snd_nxt"]) and (
                        _seq_gt(seq, s["snd_wl1"]) or (s["snd_wl1"] == seq and _seq_le(s["snd_wl2"], ack))):
                    s["snd_wnd"], s["snd_wl1"], s["snd_wl2"] = int(rec["window"]), seq, ack
                    events |= L.RNS_EV_WND
            has_ack, fin = bool(flags & _ACK), bool(flags & _FIN)        # D, tcp.rs:742-835
            acks_fin = has_ack and ack == (s["snd_nxt"] + 1) & _M32
            new = None
            if st == L.RNS_TCP_SYN_RECEIVED and has_ack:
                new = L.RNS_TCP_ESTABLISHED
                s["snd_nxt"], s["snd_una"] = (s["snd_nxt"] + 1) & _M32, ack
            elif st == L.RNS_TCP_ESTABLISHED and fin:
                new = L.RNS_TCP_CLOSE_WAIT
            elif st == L.RNS_TCP_LAST_ACK and has_ack:
                new = L.RNS_TCP_CLOSED
            elif st == L.RNS_TCP_FIN_WAIT1:
                if acks_fin and fin:
                    new = L.RNS_TCP_TIME_WAIT
                    act |= L.RNS_CTL_TIMEWAIT
                elif fin:
                    new = s["state"] = L.RNS_TCP_CLOSING
                    sent = _send(s, _ACK)
                    act |= L.RNS_CTL_RESP_TIMER
                elif acks_fin:
                    new = L.RNS_TCP_FIN_WAIT2
            elif st == L.RNS_TCP_FIN_WAIT2 and fin:
                sent = _send(s, _ACK)
                new = L.RNS_TCP_TIME_WAIT
                act |= L.RNS_CTL_RESP_TIMER | L.RNS_CTL_TIMEWAIT
            elif st == L.RNS_TCP_CLOSING and has_ack:
                new = L.RNS_TCP_TIME_WAIT
                act |= L.RNS_CTL_TIMEWAIT
            if new is not None:
                s["state"] = new
                act |= L.RNS_CTL_STATE
                events |= L.RNS_EV_STATE
            if sent is not None:
                n_sent += 1
                ctl[i] = (f,) + sent + (act | L.RNS_CTL_SEND,)
            else:
                ctl[i] = (f, 0, 0, 0, 0, act)
        s["n_pend"] = len(pl)
        for k in FLOW_DTYPE.names:
            out[f][k] = s[k]
        if pl:
            pend_out[f, :len(pl)] = np.array(pl, dtype=np.uint32)
        r["consumed"], r["readable"], r["acked"], r["n_acks"], r["events"] = consumed, readable, acked, n_sent, events
    return out, pend_out, ctl, res


def close_host(flows, op):
    """``tx_tcp_close`` on the host: ``(flows_out, ctl)`` as new numpy arrays (FLOW_DTYPE, CTL_DTYPE)."""
    flows = np.asarray(flows).reshape(-1)
    if flows.dtype != FLOW_DTYPE:
        raise TypeError("flows must be FLOW_DTYPE records")
    op = np.asarray(op, dtype=np.uint8).reshape(-1)
    if op.size != flows.size:
        raise ValueError("op needs one entry per flow")
    out, ctl = flows.copy(), np.zeros(flows.size, dtype=CTL_DTYPE)
    nxt = {_lib.RNS_TCP_ESTABLISHED: _lib.RNS_TCP_FIN_WAIT1, _lib.RNS_TCP_CLOSE_WAIT: _lib.RNS_TCP_LAST_ACK}
    for f in np.flatnonzero(op == 1):
        s = {k: int(flows[f][k]) for k in FLOW_DTYPE.names}
        if s["state"] not in nxt:
            continue
        ctl[f] = (f,) + _send(s, _FIN | _ACK) + (_lib.RNS_CTL_SEND | _lib.RNS_CTL_RESP_TIMER | _lib.RNS_CTL_STATE,)
        out[f]["state"] = nxt[s["state"]]                                # after the send, tcp.rs:211-219
    return out, ctl


def _tmpl_ok(t: bytes, hl: int, stride: int) -> bool:
    if hl not in (40, 60) or hl > stride:
        return False
    if hl == 40:
        return t[0] == 0x45 and t[9] == 6 and t[32] >> 4 == 5
    return t[0] >> 4 == 6 and t[6] == 6 and t[52] >> 4 == 5


def ctl_heads_host(ctl, n_flows: int, tmpl, head_len8, ip_id_base: int, *, out_cap: int | None = None, ip_id_add: int = 0,
                   tmpl_stride: int | None = None, out: np.ndarray | None = None, src: np.ndarray | None = None,
                   len8: np.ndarray | None = None):
    """``tx_tcp_ctl_build`` on the host: ``ctl`` CTL_DTYPE records, ``tmpl`` a uint8 array of n_flows x tmpl_stride,
    ``head_len8`` uint8 per flow.  Returns ``(out, src, len8, count)`` numpy arrays: ``out`` uint8 [out_cap * 64]
    (given arrays are written in place and keep every byte the call does not write), ``count`` uint32 [segments,
    IPv4 ones]."""
    ctl = np.asarray(ctl).reshape(-1)
    if ctl.dtype != CTL_DTYPE:
        raise TypeError("ctl must be CTL_DTYPE records")
    nfl = int(n_flows)
    tmpl = np.asarray(tmpl, dtype=np.uint8)
    stride = int(tmpl_stride) if tmpl_stride is not None else (int(tmpl.shape[1]) if tmpl.ndim == 2 else 0)
    tmpl = tmpl.reshape(-1)
    hl8 = np.asarray(head_len8, dtype=np.uint8).reshape(-1)
    send = np.flatnonzero(((ctl["act"] & _lib.RNS_CTL_SEND) != 0) & (ctl["flow"] < nfl))
    cap = len(send) if out_cap is None else int(out_cap)
    out = np.zeros(CTL_SLOT * cap, np.uint8) if out is None else out
    src = np.zeros(cap, np.uint32) if src is None else src
    len8 = np.zeros(cap, np.uint8) if len8 is None else len8
    v4s = 0
    for k, i in enumerate(send):
        c = ctl[i]
        f = int(c["flow"])
        hl = int(hl8[f])
        pid = (int(ip_id_base) + int(ip_id_add) + v4s) & 0xFFFF
        v4s += hl == 40
        if k >= cap:
            continue
        src[k], len8[k] = i, 0
        t = tmpl[f * stride:(f + 1) * stride].tobytes()
        if not _tmpl_ok(t, hl, stride) or int(c["flags"]) & _SYN:
            continue
        h = bytearray(t[:hl])
        ip = hl - 20
        h[ip + 4:ip + 8] = int(c["seq"]).to_bytes(4, "big")
        h[ip + 8:ip + 12] = int(c["ack_num"]).to_bytes(4, "big")
        h[ip + 12], h[ip + 13] = 0x50, int(c["flags"])
        h[ip + 14:ip + 16] = int(c["window"]).to_bytes(2, "big")
        h[ip + 16:ip + 18] = b"\x00\x00"
        if hl == 40:
            h[2:4], h[4:6], h[10:12] = (40).to_bytes(2, "big"), pid.to_bytes(2, "big"), b"\x00\x00"
            h[10:12] = (_fold(_be_sum(h[:20])) ^ 0xFFFF).to_bytes(2, "big")
            addrs = h[12:20]
        else:
            h[4:6] = (20).to_bytes(2, "big")
            addrs = h[8:40]
        h[ip + 16:ip + 18] = (_fold(_be_sum(addrs) + 6 + 20 + _be_sum(h[ip:])) ^ 0xFFFF).to_bytes(2, "big")
        out[CTL_SLOT * k:CTL_SLOT * k + hl] = np.frombuffer(bytes(h), dtype=np.uint8)
        len8[k] = hl
    return out, src, len8, np.array([len(send), v4s], dtype=np.uint32)


# ---------------------------------------------------------------------------
# placement -> listen responder -> connection update -> control build on one stream
# ---------------------------------------------------------------------------
class TcpConn(NamedTuple):
    """What ``tcp_conn`` leaves, all device tensors."""
    status: torch.Tensor     # the verify's status per datagram
    meta: torch.Tensor       # the placement's records
    listen: object           # the listen responder's TcpListen: replies, accept records, conn bits
    flows: torch.Tensor      # uint8 [n_flows, 40]: the sockets after the batch
    pend: torch.Tensor       # the pending lists after the batch (None with pend_cap 0)
    ctl: torch.Tensor        # uint8 [n, 16]: CTL_DTYPE per datagram
    res: torch.Tensor        # uint8 [n_flows, 24]: RES_DTYPE per flow
    out: torch.Tensor        # uint8 [n, 64]: the control segments' slots
    src: torch.Tensor        # int32 [n]: a slot's datagram
    len8: torch.Tensor       # uint8 [n]: a slot's length, 40 / 60 (0: malformed template)
    count: torch.Tensor      # int32 [2]: control segments, IPv4 ones


def tcp_conn(pool: torch.Tensor, buf_idx: torch.Tensor, blk_first: torch.Tensor, len16: torch.Tensor, local_ipv4: bytes,
             local_ipv6: bytes, table: torch.Tensor, next_seq: torch.Tensor, win_off: torch.Tensor, win_len: torch.Tensor,
             stream: torch.Tensor, listen_tbl: torch.Tensor | None, n_listen: int, iss: torch.Tensor | None,
             flows: torch.Tensor, pend: torch.Tensor | None, tmpl: torch.Tensor, head_len8: torch.Tensor, *, pend_cap: int,
             buf_bytes: int = 512, reply_cap: int | None = None, ip_id_base: int = 0,
             ip_id_add: torch.Tensor | None = None) -> TcpConn:
    """``listen.tcp_listen`` (pool verify, placement, listen responder), then ``rx_tcp_conn_update`` over the
    placement's records and ``tx_tcp_ctl_build`` over the update's, on the current stream with nothing read back
    in between.  The IPv4 ids: the responder's replies take ``ip_id_base`` (+ ``ip_id_add[0]``) onwards, the control
    segments follow them (the reply count is added on the device).  The reference would interleave the two in batch
    order; the ids are unique either way.  Returns a ``TcpConn``."""
    from .listen import tcp_listen
    status, meta, lis = tcp_listen(pool, buf_idx, blk_first, len16, local_ipv4, local_ipv6, table, next_seq, win_off,
                                   win_len, stream, listen_tbl, n_listen, iss, buf_bytes=buf_bytes, reply_cap=reply_cap,
                                   ip_id_base=ip_id_base, ip_id_add=ip_id_add)
    flat = meta.reshape(-1)
    n = flat.numel() // META_DTYPE.itemsize
    nfl = flows.numel() // FLOW_DTYPE.itemsize
    flows_out, pend_out, ctl, res = rx_tcp_conn_update(flat, flows, pend, pend_cap=pend_cap)
    add = lis.count[1:2] if ip_id_add is None else lis.count[1:2] + ip_id_add[:1]
    out, src, len8, count = tx_tcp_ctl_build(ctl.reshape(-1), nfl, tmpl, head_len8, ip_id_base, out_cap=max(n, 1),
                                             ip_id_add=add.contiguous())
    return TcpConn(status, meta, lis, flows_out, pend_out, ctl, res, out, src, len8, count)
