"""TCP send planning: tcp_write's window gate and retransmit on the device.

After ``flow.rx_tcp_flow_update`` every flow's ``snd_una``, ``snd_nxt`` and ``snd_wnd`` lie on the device.
``tx_tcp_plan`` (rns_tx_tcp_plan_dev) reads them there, decides per flow what tcp_write (tcp.rs:256-292)
and retransmit (tcp.rs:329-348) would send now, and writes exactly the descriptors
``segment.tx_segment`` takes — two entries per flow, the retransmit and the new data — with the
template rows patched as send_packet (tcp.rs:402-447) fills them.  ``tx_tcp_send`` is the plan and the
segmentation in one stream of launches, nothing read back in between; ``plan_host`` is the same plan
on numpy arrays, the host's continuation for what the device stops at.  The functions are re-exported
by ``batch``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .batch import _I32, _I64, _U8, _U16, _bytes_of, _call, _ptr as ptr, _require_cuda, _work_bytes, _workspace
from .flow import FLOW_DTYPE

# rns_tx_plan_res (rns_checksum.h)
RES_DTYPE = np.dtype([("new_bytes", "<u4"), ("new_segs", "<u4"), ("rexmit_bytes", "<u4"), ("why", "u1"), ("pad", "u1", (3,))])
PLAN_RES_DTYPE = RES_DTYPE  # its name in ``batch``, where RES_DTYPE is the flow update's
assert RES_DTYPE.itemsize == 16
_M32 = 0xFFFFFFFF


def tx_plan_work(n_flows: int) -> int:
    """Bytes of workspace ``tx_tcp_plan`` needs (rns_tx_tcp_plan_work)."""
    return _work_bytes("rns_tx_tcp_plan_work", n_flows)


def _per_flow(t: torch.Tensor, name: str, n: int, dtypes, dev) -> None:
    _require_cuda(t, name, dtypes)
    if t.numel() != n or t.device != dev:
        raise ValueError(f"{name} needs one entry per flow ({n}) on the flows' device")


def tx_tcp_plan(flows: torch.Tensor, sq_off: torch.Tensor, sq_seq: torch.Tensor, sq_len: torch.Tensor, mss: torch.Tensor,
                tmpl: torch.Tensor, head_len8: torch.Tensor, *, rexmit: torch.Tensor | None = None, ip_id_base: int = 0,
                ip_id_add: torch.Tensor | None = None, head_first_off: int, seg_cap: int,
                work: torch.Tensor | None = None, flows_out: torch.Tensor | None = None) -> dict:
    """TCP send planning (rns_tx_tcp_plan_dev).  ``flows``: uint8, n_flows x 40 (FLOW_DTYPE), as the flow
    update left them; ``sq_off`` int64, ``sq_seq`` / ``sq_len`` int32: the flows' send buffers in the
    arena (the byte of sequence ``sq_seq[f]`` at ``sq_off[f]``, ``sq_len[f]`` bytes); ``mss`` uint16;
    ``tmpl`` uint8, one row (the template head) per flow; ``head_len8`` uint8 (40: IPv4, 60: IPv6);
    ``rexmit`` uint8 per flow, non-zero where the retransmit timer fired; ``ip_id_add`` an int32 tensor
    whose first entry is added to ``ip_id_base`` on the device (``tx_ack_build``'s ``n_acks[1:]``, say).
    Returns a dict over the E = 2 n_flows entries: ``tmpl`` (E x stride), ``head_len8``, ``pay_off``,
    ``pay_len``, ``mss``, ``head_off``, ``seg_first`` (E + 1), ``blk_flow`` (ceil(seg_cap / 64)) — the
    arguments of ``tx_segment`` — and ``n`` (int32: kept segments, IPv4 ones), ``res`` (uint8, n_flows x
    16, RES_DTYPE), ``flows_out`` (like ``flows``, ``snd_nxt`` advanced; must not overlap it)."""
    _require_cuda(flows, "flows", _U8)
    dev = flows.device
    nfl = flows.numel() // FLOW_DTYPE.itemsize
    _bytes_of(flows, "flows", nfl, FLOW_DTYPE.itemsize, dev)
    _per_flow(sq_off, "sq_off", nfl, _I64, dev)
    _per_flow(sq_seq, "sq_seq", nfl, _I32, dev)
    _per_flow(sq_len, "sq_len", nfl, _I32, dev)
    _per_flow(mss, "mss", nfl, _U16, dev)
    _per_flow(head_len8, "head_len8", nfl, _U8, dev)
    if rexmit is not None:
        _per_flow(rexmit, "rexmit", nfl, _U8, dev)
    _require_cuda(tmpl, "tmpl", _U8)
    if tmpl.dim() == 1 and nfl == 1:
        tmpl = tmpl.view(1, -1)
    if tmpl.dim() != 2 or tmpl.shape[0] != nfl or tmpl.shape[1] == 0 or tmpl.device != dev:
        raise ValueError("tmpl must hold one row (the template head) per flow on the flows' device")
    stride = int(tmpl.shape[1])
    if ip_id_add is not None:
        _require_cuda(ip_id_add, "ip_id_add", _I32)
        if ip_id_add.numel() < 1 or ip_id_add.device != dev:
            raise ValueError("ip_id_add holds one int32 entry on the flows' device")
    seg_cap, head_first_off = int(seg_cap), int(head_first_off)
    if nfl > 2 ** 30 or not 0 <= seg_cap <= _lib.RNS_CHAIN_MAX_PACKETS or not 0 <= int(ip_id_base) <= 0xFFFF or \
            not 0 <= head_first_off < 2 ** 64:
        raise ValueError("at most 2^30 flows and RNS_CHAIN_MAX_PACKETS segments; ip_id_base is a u16, head_first_off a u64")
    if flows_out is None:
        flows_out = torch.empty_like(flows)
    else:
        _bytes_of(flows_out, "flows_out", nfl, FLOW_DTYPE.itemsize, dev)
    work = _workspace(work, tx_plan_work(nfl), dev)
    E = 2 * nfl
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    p = {"tmpl": new((E, stride), torch.uint8), "head_len8": new(E, torch.uint8), "pay_off": new(E, torch.int64),
         "pay_len": new(E, torch.int32), "mss": new(E, torch.uint16), "head_off": new(E, torch.int64),
         "seg_first": new(E + 1, torch.int32), "blk_flow": new((seg_cap + 63) // 64, torch.int32),
         "n": new(2, torch.int32), "res": new((nfl, RES_DTYPE.itemsize), torch.uint8), "flows_out": flows_out}
    _call("rns_tx_tcp_plan_dev", dev, ptr(flows), ptr(flows_out), nfl, ptr(sq_off), ptr(sq_seq), ptr(sq_len), ptr(mss),
          ptr(rexmit), ptr(tmpl), stride, ptr(head_len8), int(ip_id_base), ptr(ip_id_add), head_first_off & (2 ** 64 - 1),
          seg_cap, ptr(p["tmpl"]), ptr(p["head_len8"]), ptr(p["pay_off"]), ptr(p["pay_len"]), ptr(p["mss"]),
          ptr(p["head_off"]), p["seg_first"].data_ptr(), ptr(p["blk_flow"]), p["n"].data_ptr(), ptr(p["res"]),
          work.data_ptr(), work.numel())
    return p


def tx_tcp_send(arena: torch.Tensor, flows: torch.Tensor, sq_off: torch.Tensor, sq_seq: torch.Tensor, sq_len: torch.Tensor,
                mss: torch.Tensor, tmpl: torch.Tensor, head_len8: torch.Tensor, *, seg_cap: int, head_first_off: int,
                status: torch.Tensor | None = None, **plan_args):
    """The plan, then ``tx_segment`` on the planned descriptors with ``n_seg = seg_cap``: one stream of
    launches, no synchronisation and nothing read back in between.  Returns ``(plan, status)``: the dict
    of ``tx_tcp_plan`` and the uint8 status per segment, ``seg_cap`` entries — those at and past
    ``plan['n'][0]`` are RNS_TX_MALFORMED (no entry covers them) and nothing is written for them."""
    from .segment import tx_segment
    _require_cuda(arena, "arena", _U8)
    if arena.device != flows.device:
        raise ValueError("the arena must be on the flows' device")
    p = tx_tcp_plan(flows, sq_off, sq_seq, sq_len, mss, tmpl, head_len8, seg_cap=seg_cap, head_first_off=head_first_off,
                    **plan_args)
    if p["head_len8"].numel() == 0 or int(seg_cap) == 0:  # no flow or no room: no segment is covered
        return p, torch.full((int(seg_cap),), _lib.RNS_TX_MALFORMED, dtype=torch.uint8, device=arena.device)
    status = tx_segment(arena, p["tmpl"], p["head_len8"], p["pay_off"], p["pay_len"], p["mss"], p["head_off"],
                        p["seg_first"], p["blk_flow"], int(seg_cap), status=status)
    return p, status


# ---------------------------------------------------------------------------
# the same plan on the host
# ---------------------------------------------------------------------------
def _tmpl_ok(t: np.ndarray, hl: int, stride: int) -> bool:
    """The template rule of the ACK build and the planning (tcp_tmpl_ok, rns_k_tcp_head.hpp)."""
    if hl not in (40, 60) or hl > stride:
        return False
    if hl == 40:
        return bool(t[0] == 0x45 and t[9] == 6 and (t[32] >> 4) == 5)
    return bool((t[0] >> 4) == 6 and t[6] == 6 and (t[52] >> 4) == 5)


def plan_host(flows, sq_off, sq_seq, sq_len, mss, tmpl, head_len8, *, rexmit=None, ip_id_base: int = 0, ip_id_add: int = 0,
              head_first_off: int, seg_cap: int, tmpl_out_fill: int = 0) -> dict:
    """``tx_tcp_plan`` on the host, in closed form, with the same outputs array for array (numpy; the
    rows of ``tmpl`` that the device leaves unwritten hold ``tmpl_out_fill``).  ``flows`` a FLOW_DTYPE
    array, ``tmpl`` uint8 n_flows x stride, ``ip_id_add`` the value of the device dword."""
    flows = np.asarray(flows).reshape(-1)
    if flows.dtype != FLOW_DTYPE:
        raise TypeError("flows must be FLOW_DTYPE records")
    nfl = flows.size
    tmpl = np.asarray(tmpl, dtype=np.uint8).reshape(nfl, -1) if nfl else np.zeros((0, 1), dtype=np.uint8)
    stride, E, cap, M = tmpl.shape[1], 2 * nfl, int(seg_cap), _lib.RNS_PLAN_MAX
    sq_off, sq_seq, sq_len = (np.asarray(x).reshape(-1) for x in (sq_off, sq_seq, sq_len))
    mss, head_len8 = np.asarray(mss).reshape(-1), np.asarray(head_len8).reshape(-1)
    if any(x.size != nfl for x in (sq_off, sq_seq, sq_len, mss, head_len8)) or stride == 0:
        raise ValueError("one entry per flow, and a template row of at least one byte")
    if nfl > 2 ** 30 or not 0 <= cap <= _lib.RNS_CHAIN_MAX_PACKETS:
        raise ValueError("at most 2^30 flows and RNS_CHAIN_MAX_PACKETS segments")
    p = {"tmpl": np.full((E, stride), tmpl_out_fill, dtype=np.uint8), "head_len8": np.repeat(head_len8.astype(np.uint8), 2),
         "pay_off": np.zeros(E, dtype=np.uint64), "pay_len": np.zeros(E, dtype=np.uint32),
         "mss": np.repeat(mss.astype(np.uint16), 2), "head_off": np.zeros(E, dtype=np.uint64),
         "seg_first": np.zeros(E + 1, dtype=np.uint32), "blk_flow": np.full((cap + 63) // 64, E, dtype=np.uint32),
         "n": np.zeros(2, dtype=np.uint32), "res": np.zeros(nfl, dtype=RES_DTYPE), "flows_out": flows.copy()}
    at = v4_at = 0                     # kept segments, kept IPv4 segments
    head = int(head_first_off)
    full = False                       # an entry was dropped: so is every later one
    id0 = int(ip_id_base) + int(ip_id_add)
    for f in range(nfl):
        fl = flows[f]
        una, nxt, wnd = int(fl["snd_una"]), int(fl["snd_nxt"]), int(fl["snd_wnd"])
        ms, hl, ql = int(mss[f]), int(head_len8[f]), int(sq_len[f]) & _M32
        inflight, a = (nxt - una) & _M32, (una - int(sq_seq[f])) & _M32
        res = p["res"][f]
        rex = new = segs = 0
        if int(fl["state"]) != _lib.RNS_TCP_ESTABLISHED:
            res["why"] = _lib.RNS_PLAN_STATE
        elif ms == 0 or ql > M or wnd > M or inflight > M or a > ql or a + inflight > ql:
            res["why"] = _lib.RNS_PLAN_BAD
        elif not _tmpl_ok(tmpl[f], hl, stride):
            res["why"] = _lib.RNS_PLAN_TMPL
        else:
            if rexmit is not None and int(np.asarray(rexmit).reshape(-1)[f]) and inflight:
                rex = min(ms, inflight)
            unsent, room = ql - a - inflight, max(wnd - inflight, 0)
            nfull = unsent // ms
            kf = min(nfull, room // ms)
            new, segs = kf * ms, kf
            if kf < nfull:
                res["why"] = _lib.RNS_PLAN_WINDOW
            elif unsent > new:
                if unsent - new <= room - new:
                    new, segs = unsent, segs + 1
                else:
                    res["why"] = _lib.RNS_PLAN_WINDOW
        q0 = (int(sq_off[f]) + a) & (2 ** 64 - 1)
        for k, (nbytes, nseg, off) in enumerate(((rex, 1 if rex else 0, q0), (new, segs, (q0 + inflight) & (2 ** 64 - 1)))):
            e = 2 * f + k
            p["seg_first"][e], p["head_off"][e] = at, head & (2 ** 64 - 1)
            if nseg == 0:
                continue
            if full or at + nseg > cap:
                full = True
                if k == 1:
                    res["why"] = _lib.RNS_PLAN_CAP
                continue
            p["pay_off"][e], p["pay_len"][e] = off, nbytes
            row = tmpl[f, :hl].copy()
            ip = 20 if hl == 40 else 40
            row[ip + 4:ip + 12] = np.frombuffer(nxt.to_bytes(4, "big") + int(fl["rcv_nxt"]).to_bytes(4, "big"), dtype=np.uint8)
            row[ip + 12], row[ip + 13] = 0x50, 0x18
            row[ip + 14:ip + 16] = np.frombuffer(((0xFFFF - (int(fl["rq_len"]) & 0xFFFF)) & 0xFFFF).to_bytes(2, "big"), np.uint8)
            if hl == 40:
                row[4:6] = np.frombuffer(((id0 + v4_at) & 0xFFFF).to_bytes(2, "big"), dtype=np.uint8)
                v4_at += nseg
            p["tmpl"][e, :hl] = row
            p["blk_flow"][(at + 63) // 64:(at + nseg + 63) // 64] = e  # the 64-segment blocks that start in this entry
            at += nseg
            head += nseg * hl
            if k == 0:
                res["rexmit_bytes"] = nbytes
            else:
                res["new_bytes"], res["new_segs"] = nbytes, nseg
                p["flows_out"][f]["snd_nxt"] = (nxt + nbytes) & _M32
    p["seg_first"][E] = at
    p["n"][:] = (at, v4_at)
    return p
