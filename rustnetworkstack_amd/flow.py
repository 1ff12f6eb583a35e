"""TCP flow update and ACK build: the rest of tcp_input for an Established socket on the device.

``place.rx_tcp_place_pool`` leaves a 24-byte record per datagram.  ``rx_tcp_flow_update`` walks every
flow's records of the batch in batch order through tcp.rs:642-740 (rns_rx_tcp_flow_update_dev): the
reassembler's and the socket's sequence numbers, the delayed-ACK count and its immediate ACKs, the
ACK-field check, the send window.  The first segment that is not the fast path's (a flag, options,
bytes outside the window, a full pending list, a flow that is not Established, more than
``RNS_FLOW_MAX_SEGS`` segments) stops its flow; ``flow_update_host`` is the same walk in Python, record
for record, and the host's path from there.  ``tx_ack_build`` builds and finalizes the ACKs the update
decided on, in batch order (rns_tx_ack_build_dev).  After the two calls the host reads 40 + 24 bytes
per flow, not 24 per datagram.  The functions are re-exported by ``batch``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .batch import _I32, _U8, _bytes_of, _call, _ptr as ptr, _require_cuda, _seq_gt, _work_bytes, _workspace
from .place import META_DTYPE

# rns_tcp_flow, rns_rx_tcp_seg, rns_tcp_flow_res (rns_checksum.h)
FLOW_DTYPE = np.dtype([("rcv_nxt", "<u4"), ("rcv_max", "<u4"), ("snd_una", "<u4"), ("snd_nxt", "<u4"),
                       ("snd_wnd", "<u4"), ("snd_wl1", "<u4"), ("snd_wl2", "<u4"), ("rq_len", "<u4"), ("n_pend", "<u4"),
                       ("delayed_acks", "<u2"), ("state", "u1"), ("ack_timer", "u1")])
SEG_DTYPE = np.dtype([("ack_num", "<u4"), ("window", "<u2"), ("act", "u1"), ("pad", "u1")])
RES_DTYPE = np.dtype([("n_segs", "<u4"), ("consumed", "<u4"), ("stop", "<u4"), ("readable", "<u4"), ("acked", "<u4"),
                      ("n_acks", "<u2"), ("events", "u1"), ("why", "u1")])
assert (FLOW_DTYPE.itemsize, SEG_DTYPE.itemsize, RES_DTYPE.itemsize) == (40, 8, 24)
ACK_SLOT = 64  # bytes per ACK slot of tx_ack_build's output
_M32 = 0xFFFFFFFF


def flow_update_work(n_pkts: int, n_flows: int) -> int:
    """Bytes of workspace ``rx_tcp_flow_update`` (and ``tx_ack_build``) need (rns_rx_tcp_flow_update_work)."""
    return _work_bytes("rns_rx_tcp_flow_update_work", n_pkts, n_flows)


def rx_tcp_flow_update(meta: torch.Tensor, flows: torch.Tensor, pend: torch.Tensor | None, *, pend_cap: int,
                       flows_out: torch.Tensor | None = None, pend_out: torch.Tensor | None = None,
                       seg: torch.Tensor | None = None, res: torch.Tensor | None = None,
                       work: torch.Tensor | None = None):
    """TCP flow update (rns_rx_tcp_flow_update_dev).  ``meta``: the placement's records (uint8, n x 24);
    ``flows``: uint8, n_flows x 40 (FLOW_DTYPE); ``pend``: int32, n_flows x pend_cap x 2 (seq, len)
    pairs, the reassembler's pending list in its order (None with ``pend_cap == 0``).  Returns
    ``(flows_out, pend_out, seg, res)``: new tensors unless given (uint8 n_flows x 40, int32 like
    ``pend``, uint8 n x 8 SEG_DTYPE, uint8 n_flows x 24 RES_DTYPE); in and out must not overlap.
    ``work``: a uint8 workspace of ``flow_update_work(n, n_flows)`` bytes (allocated when None)."""
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
    if seg is None:
        seg = torch.empty((n, SEG_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    else:
        _bytes_of(seg, "seg", n, SEG_DTYPE.itemsize, dev)
    if res is None:
        res = torch.empty((nfl, RES_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    else:
        _bytes_of(res, "res", nfl, RES_DTYPE.itemsize, dev)
    work = _workspace(work, flow_update_work(n, nfl), dev)
    _call("rns_rx_tcp_flow_update_dev", dev, ptr(meta), n, nfl, ptr(flows), ptr(pend) if pend_cap else None, pend_cap,
          ptr(flows_out), ptr(pend_out) if pend_cap else None, ptr(seg), ptr(res), work.data_ptr(), work.numel())
    return flows_out, pend_out, seg, res


def tx_ack_build(meta: torch.Tensor, seg: torch.Tensor, flows: torch.Tensor, tmpl: torch.Tensor, head_len8: torch.Tensor,
                 ip_id_base: int, *, ack_cap: int, tmpl_stride: int | None = None, out: torch.Tensor | None = None,
                 ack_src: torch.Tensor | None = None, ack_len8: torch.Tensor | None = None,
                 n_acks: torch.Tensor | None = None, work: torch.Tensor | None = None):
    """ACK build (rns_tx_ack_build_dev): ``meta`` / ``seg`` as the update took and gave them, ``flows`` its
    out state, ``tmpl`` the flows' template heads (uint8, ``tmpl_stride`` bytes each: the second
    dimension of a 2-D tensor by default), ``head_len8`` uint8 per flow (40: IPv4, 60: IPv6).  Returns
    ``(out, ack_src, ack_len8, n_acks)``: ``out`` uint8 ``ack_cap`` x 64 (only the heads' bytes are
    written), ``ack_src`` int32 and ``ack_len8`` uint8 per slot, ``n_acks`` int32 [total, IPv4 ones].
    ``ack_cap == 0`` counts only (the first three are then None unless given)."""
    _require_cuda(meta, "meta", _U8)
    dev = meta.device
    n = meta.numel() // META_DTYPE.itemsize
    _bytes_of(seg, "seg", n, SEG_DTYPE.itemsize, dev)
    _require_cuda(flows, "flows", _U8)
    nfl = flows.numel() // FLOW_DTYPE.itemsize
    _bytes_of(flows, "flows", nfl, FLOW_DTYPE.itemsize, dev)
    _require_cuda(tmpl, "tmpl", _U8)
    _require_cuda(head_len8, "head_len8", _U8)
    if tmpl_stride is None:
        tmpl_stride = int(tmpl.shape[1]) if tmpl.dim() == 2 else 0
    if head_len8.numel() != nfl or (nfl and (tmpl_stride <= 0 or tmpl.numel() < nfl * tmpl_stride)):
        raise ValueError("head_len8 and tmpl need one entry / tmpl_stride bytes per flow")
    if tmpl.device != dev or head_len8.device != dev:
        raise ValueError("tmpl and head_len8 must be on the meta's device")
    ack_cap = int(ack_cap)
    if not 0 <= ack_cap < 2 ** 32 or not 0 <= int(ip_id_base) <= 0xFFFF:
        raise ValueError("ack_cap is a u32 and ip_id_base a u16")
    if ack_cap:
        if out is None:
            out = torch.empty((ack_cap, ACK_SLOT), dtype=torch.uint8, device=dev)
        if ack_src is None:
            ack_src = torch.empty(ack_cap, dtype=torch.int32, device=dev)
        if ack_len8 is None:
            ack_len8 = torch.empty(ack_cap, dtype=torch.uint8, device=dev)
        _bytes_of(out, "out", ack_cap, ACK_SLOT, dev)
        _require_cuda(ack_src, "ack_src", _I32)
        _bytes_of(ack_len8, "ack_len8", ack_cap, 1, dev)
        if ack_src.numel() != ack_cap or ack_src.device != dev:
            raise ValueError("ack_src needs one entry per slot on the meta's device")
    if n_acks is None:
        n_acks = torch.empty(2, dtype=torch.int32, device=dev)
    else:
        _require_cuda(n_acks, "n_acks", _I32)
        if n_acks.numel() != 2 or n_acks.device != dev:
            raise ValueError("n_acks holds two int32 entries on the meta's device")
    work = _workspace(work, flow_update_work(n, 0), dev)
    _call("rns_tx_ack_build_dev", dev, ptr(meta), ptr(seg), n, ptr(flows), nfl, ptr(tmpl), tmpl_stride, ptr(head_len8),
          int(ip_id_base), work.data_ptr(), work.numel(), ptr(out) if ack_cap else None, ack_cap,
          ptr(ack_src) if ack_cap else None, ptr(ack_len8) if ack_cap else None, n_acks.data_ptr())
    return out, ack_src, ack_len8, n_acks


# ---------------------------------------------------------------------------
# the same walk on the host
# ---------------------------------------------------------------------------
def _seq_le(a: int, b: int) -> bool:
    return not _seq_gt(a, b)


def flow_update_host(meta_records, flows, pend, pend_cap: int):
    """``rx_tcp_flow_update`` on the host, with the same outputs record for record: ``meta_records`` a
    META_DTYPE array, ``flows`` a FLOW_DTYPE array, ``pend`` a uint32 array of n_flows x pend_cap x 2 (or
    None with ``pend_cap == 0``).  Returns ``(flows_out, pend_out, seg, res)`` as new numpy arrays
    (``pend_out``'s entries past n_pend are the input's).  It is the host's path for everything the
    device stops at: feed it the records from ``res['stop']`` on, after the slow path has dealt with
    the stopping segment."""
    m = np.asarray(meta_records).reshape(-1)
    flows = np.asarray(flows).reshape(-1)
    if m.dtype != META_DTYPE or flows.dtype != FLOW_DTYPE:
        raise TypeError("meta_records must be META_DTYPE records and flows FLOW_DTYPE records")
    n, nfl, cap = m.size, flows.size, int(pend_cap)
    pend_in = (np.zeros((nfl, 0, 2), dtype=np.uint32) if cap == 0 or pend is None
               else np.asarray(pend, dtype=np.uint32).reshape(nfl, cap, 2))
    out, pend_out = flows.copy(), pend_in.copy()
    seg, res = np.zeros(n, dtype=SEG_DTYPE), np.zeros(nfl, dtype=RES_DTYPE)
    res["stop"] = _M32
    member = ((m["place"] & _lib.RNS_PLACE_FLOW) != 0) & (m["flow"] < nfl)
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
        if idx.size > _lib.RNS_FLOW_MAX_SEGS:
            r["stop"], r["why"] = idx[0], _lib.RNS_STOP_MANY
            continue
        if s["state"] != _lib.RNS_TCP_ESTABLISHED or s["n_pend"] > cap:
            r["stop"], r["why"] = idx[0], _lib.RNS_STOP_STATE
            continue
        pl = [(int(a), int(b)) for a, b in pend_in[f, :s["n_pend"]]]
        readable = acked = n_acks = events = consumed = 0
        for i in idx:
            rec = m[i]
            flags, seq, ack, pay = int(rec["flags"]), int(rec["seq"]), int(rec["ack"]), int(rec["pay_len"])
            why = (_lib.RNS_STOP_FLAGS if flags & 0x07 else
                   _lib.RNS_STOP_OPTIONS if int(rec["tcp_hdr"]) != 20 else
                   _lib.RNS_STOP_OUTSIDE if int(rec["place"]) & _lib.RNS_PLACE_OUTSIDE else
                   _lib.RNS_STOP_PEND if pay and seq != s["rcv_nxt"] and len(pl) >= cap else 0)
            if why:
                r["stop"], r["why"] = i, why
                break
            act = _lib.RNS_SEG_CONSUMED
            if pay:                                                      # tcp.rs:642-687
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
                s["delayed_acks"] = (s["delayed_acks"] + 1) & 0xFFFF
                if s["delayed_acks"] >= 5:
                    s["delayed_acks"] = s["ack_timer"] = 0
                    act |= _lib.RNS_SEG_ACK
                    seg[i]["ack_num"] = s["rcv_nxt"]
                    seg[i]["window"] = (0xFFFF - (s["rq_len"] & 0xFFFF)) & 0xFFFF
                    n_acks += 1
                elif s["ack_timer"] == 0:
                    s["ack_timer"] = 1
                    act |= _lib.RNS_SEG_TIMER
            if flags & 0x10:                                             # tcp.rs:698-740
                if _seq_gt(ack, s["snd_una"]) and _seq_le(ack, s["snd_nxt"]):
                    acked = (acked + ack - s["snd_una"]) & _M32
                    s["snd_una"] = ack
                if _seq_le(s["snd_una"], ack) and _seq_le(ack, s["snd_nxt"]) and (
                        _seq_gt(seq, s["snd_wl1"]) or (s["snd_wl1"] == seq and _seq_le(s["snd_wl2"], ack))):
                    s["snd_wnd"], s["snd_wl1"], s["snd_wl2"] = int(rec["window"]), seq, ack
                    events |= _lib.RNS_EV_WND
            seg[i]["act"] = act
            consumed += 1
        s["n_pend"] = len(pl)
        for k in FLOW_DTYPE.names:
            out[f][k] = s[k]
        if pl:
            pend_out[f, :len(pl)] = np.array(pl, dtype=np.uint32)
        r["consumed"], r["readable"], r["acked"], r["n_acks"], r["events"] = consumed, readable, acked, n_acks, events
    return out, pend_out, seg, res
