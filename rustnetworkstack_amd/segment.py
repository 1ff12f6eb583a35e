"""TCP segmentation offload: tcp_write's segment loop (tcp.rs:256-285) on the device.

tcp_write cuts one send into ``send_mss`` pieces and sends each with the same ports, ack, window,
flags and addresses: the heads of one send differ in the sequence number, the IPv4 id and the two
length fields only.  A *flow* — one tcp_write call — is therefore a template head, the send's data
where it lies in the arena, its mss and the place its heads go.  ``tx_segment_layout`` computes the
segment index and the head offsets for given flows, ``tx_segment`` builds and finalizes every head
on the device (rns_tx_segment_dev) and ``tx_segment_chains`` gives the [head, data slice] chains
the form expands to, which ``send_batch_chain`` sends.  The functions are re-exported by ``batch``,
whose argument checks they use.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .batch import _I32, _I64, _U8, _U16, _call, _descriptors, _status


def _flows(pay_len, mss, head_len):
    pl, ms, hl = np.asarray(pay_len), np.asarray(mss), np.asarray(head_len)
    if pl.ndim != 1 or ms.shape != pl.shape or hl.shape != pl.shape:
        raise ValueError("pay_len, mss and head_len must be 1-D and of the same size")
    if pl.size and (int(pl.min()) < 0 or int(pl.max()) > 0xFFFFFFFF):
        raise ValueError("the segmentation form holds u32 data lengths")
    if ms.size and (int(ms.min()) < 0 or int(ms.max()) > 0xFFFF):
        raise ValueError("the segmentation form holds u16 mss values (<= 65535)")
    if hl.size and (int(hl.min()) < 0 or int(hl.max()) > 0xFF):
        raise ValueError("the segmentation form holds u8 head lengths (<= 255)")
    return (np.ascontiguousarray(pl, dtype=np.uint32), np.ascontiguousarray(ms, dtype=np.uint16),
            np.ascontiguousarray(hl, dtype=np.uint8))


def tx_segment_layout(pay_len, mss, head_len, head_first_off: int = 0):
    """The segmentation form's index for flows with the given data lengths, mss and head lengths
    (rns_tx_segment_layout): flow f has ``ceil(pay_len[f] / mss[f])`` segments from ``seg_first[f]``
    on and its heads lie back to back from ``head_off[f]``, the flows' head ranges back to back from
    ``head_first_off``.  Returns (seg_first uint32 [n_flows+1], head_off uint64 [n_flows], blk_flow
    uint32 [ceil(n_seg/64)], n_seg, head_end)."""
    pl, ms, hl = _flows(pay_len, mss, head_len)
    nfl = int(pl.size)
    seg_first, head_off = np.zeros(nfl + 1, dtype=np.uint32), np.zeros(max(nfl, 1), dtype=np.uint64)
    nseg, hend = ctypes.c_uint64(0), ctypes.c_uint64(0)
    lib = _lib.load()
    st = lib.rns_tx_segment_layout(pl.ctypes.data, ms.ctypes.data, hl.ctypes.data, nfl, int(head_first_off),
                                   seg_first.ctypes.data, head_off.ctypes.data, None, ctypes.byref(nseg),
                                   ctypes.byref(hend))
    _lib.check(st, "rns_tx_segment_layout")
    nb = (int(nseg.value) + 63) // 64
    blk_flow = np.zeros(max(nb, 1), dtype=np.uint32)
    st = lib.rns_tx_segment_layout(pl.ctypes.data, ms.ctypes.data, hl.ctypes.data, nfl, int(head_first_off),
                                   seg_first.ctypes.data, head_off.ctypes.data, blk_flow.ctypes.data,
                                   ctypes.byref(nseg), ctypes.byref(hend))
    _lib.check(st, "rns_tx_segment_layout")
    return seg_first, head_off[:nfl], blk_flow[:nb], int(nseg.value), int(hend.value)


def tx_segment_chains(pay_off, pay_len, mss, head_len, head_off):
    """The CSR chains the segmentation form expands to (rns_tx_segment_chains): segment j of flow f
    = [(head_off[f] + j * head_len[f], head_len[f]), (pay_off[f] + j * mss[f], its data bytes)].
    Returns (frag_off uint64 [2 n_seg], frag_len uint32 [2 n_seg], first uint32 [n_seg+1])."""
    pl, ms, hl = _flows(pay_len, mss, head_len)
    po = np.ascontiguousarray(pay_off, dtype=np.uint64)
    ho = np.ascontiguousarray(head_off, dtype=np.uint64)
    nfl = int(pl.size)
    if po.shape != pl.shape or ho.shape != pl.shape:
        raise ValueError("pay_off and head_off need one entry per flow")
    if np.any((pl > 0) & (ms == 0)):
        raise ValueError("a flow with data needs mss >= 1")
    nseg = int(((pl.astype(np.uint64) + np.maximum(ms, 1) - 1) // np.maximum(ms, 1)).sum())
    frag_off, frag_len = np.zeros(max(2 * nseg, 1), dtype=np.uint64), np.zeros(max(2 * nseg, 1), dtype=np.uint32)
    first = np.zeros(nseg + 1, dtype=np.uint32)
    st = _lib.load().rns_tx_segment_chains(po.ctypes.data, pl.ctypes.data, ms.ctypes.data, hl.ctypes.data,
                                           ho.ctypes.data, nfl, nseg, frag_off.ctypes.data, frag_len.ctypes.data,
                                           first.ctypes.data)
    _lib.check(st, "rns_tx_segment_chains")
    return frag_off[:2 * nseg], frag_len[:2 * nseg], first


def tx_segment(arena: torch.Tensor, tmpl: torch.Tensor, head_len8: torch.Tensor, pay_off: torch.Tensor,
               pay_len: torch.Tensor, mss: torch.Tensor, head_off: torch.Tensor, seg_first: torch.Tensor,
               blk_flow: torch.Tensor, n_seg: int, *, status: torch.Tensor | None = None) -> torch.Tensor:
    """TCP segmentation offload (rns_tx_segment_dev): for flow f, template head ``tmpl[f]`` (a 2-D
    uint8 tensor, one row per flow, or 1-D for one flow), data ``arena[pay_off[f] : + pay_len[f]]``
    cut into ``mss[f]`` pieces, the head of piece j written to ``head_off[f] + j * head_len8[f]``
    with its lengths, IPv4 id + j, seq + j * mss and both checksums filled — exactly the bytes and
    the uint8 status per segment of ``tx_fill_chain`` on the [head, data slice] chains with heads
    built from the template.  ``seg_first`` / ``blk_flow`` / ``n_seg``: see ``tx_segment_layout``."""
    dev = _descriptors(arena, ("tmpl", tmpl, _U8), ("head_len8", head_len8, _U8), ("pay_off", pay_off, _I64),
                       ("pay_len", pay_len, _I32), ("mss", mss, _U16), ("head_off", head_off, _I64),
                       ("seg_first", seg_first, _I32), ("blk_flow", blk_flow, _I32))
    nfl = head_len8.numel()
    if tmpl.dim() == 1:
        tmpl = tmpl.view(1, -1)
    if tmpl.dim() != 2 or tmpl.shape[0] != nfl or tmpl.shape[1] == 0:
        raise ValueError("tmpl must hold one row (the template head) per flow")
    if any(t.numel() != nfl for t in (pay_off, pay_len, mss, head_off)) or seg_first.numel() != nfl + 1:
        raise ValueError("head_len8, pay_off, pay_len, mss and head_off need one entry per flow, seg_first one more")
    n_seg = int(n_seg)
    if n_seg < 0 or n_seg > _lib.RNS_CHAIN_MAX_PACKETS:
        raise ValueError(f"at most {_lib.RNS_CHAIN_MAX_PACKETS} segments per call")
    if blk_flow.numel() < (n_seg + 63) // 64:
        raise ValueError("blk_flow needs one entry per 64 segments")
    status = _status(status, n_seg, dev)
    _call("rns_tx_segment_dev", dev, arena.data_ptr(), arena.numel(), tmpl.data_ptr(), int(tmpl.shape[1]),
          head_len8.data_ptr(), pay_off.data_ptr(), pay_len.data_ptr(), mss.data_ptr(), head_off.data_ptr(),
          seg_first.data_ptr(), blk_flow.data_ptr(), nfl, n_seg, status.data_ptr())
    return status
