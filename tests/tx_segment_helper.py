"""Helpers of the TCP segmentation tests (rns_tx_segment_dev): template heads, the head of segment j
built field by field from its template — tcp.rs:938-976 (tcp_output) and ip.rs:140-177 (ip_output)
restated in Python — flows laid into an arena of random bytes, and the numpy expansion of the form:
the segment index, the head offsets and the [head, data slice] chains.  Nothing here calls the code
under test; the checksums come from Oracle.tx_chain_fill on the expanded chains."""
import struct
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O

SRC4, DST4 = bytes([10, 0, 0, 2]), bytes([10, 0, 0, 1])
SRC6 = bytes.fromhex("fd000000000000000000000000000002")
DST6 = bytes.fromhex("fd000000000000000000000000000001")
FLAG_ACK, FLAG_PSH = 0x10, 0x08


def template(v6=False, opts=0, seq=0x1000, ident=7, ack=0x55AA1234, window=0x7210, junk=0xBEEF):
    """A template head as tcp_write's first piece would carry it: every field final but the lengths
    and the two checksums, which hold ``junk`` (the kernel must ignore them).  ``opts`` = bytes of
    TCP options (a multiple of 4, <= 40)."""
    assert opts % 4 == 0 and 0 <= opts <= 40
    doff = 5 + opts // 4
    tcp = struct.pack(">HHIIBBHHH", 0xC001, 80, seq & 0xFFFFFFFF, ack, doff << 4, FLAG_ACK | FLAG_PSH, window, junk, 0)
    tcp += bytes((0x01 + 7 * k) & 0xFF for k in range(opts))
    if v6:
        ip = struct.pack(">IHBB", 0x60000000, junk, 6, 64) + SRC6 + DST6
    else:
        ip = struct.pack(">BBHHHBBH", 0x45, 0, junk, ident & 0xFFFF, 0x4000, 64, 6, junk) + SRC4 + DST4
    return ip + tcp


def head(tmpl: bytes, j: int, mss: int, seglen: int) -> bytes:
    """The head of segment j of a flow, both checksum fields zero."""
    h = bytearray(tmpl)
    hl = len(h)
    if h[0] >> 4 == 4:
        iphdr = 20
        h[2:4] = struct.pack(">H", hl + seglen)                                  # ip.rs:146 total length
        h[4:6] = struct.pack(">H", (struct.unpack(">H", tmpl[4:6])[0] + j) & 0xFFFF)  # NEXT_PACKET_ID.fetch_add(1)
        h[10:12] = b"\0\0"
    else:
        iphdr = 40
        h[4:6] = struct.pack(">H", hl - 40 + seglen)                             # ip.rs:168 payload length
    seq = struct.unpack(">I", tmpl[iphdr + 4:iphdr + 8])[0]
    h[iphdr + 4:iphdr + 8] = struct.pack(">I", (seq + j * mss) & 0xFFFFFFFF)       # tcp.rs:945, advanced per piece
    h[iphdr + 16:iphdr + 18] = b"\0\0"
    return bytes(h)


class Flow:
    """One tcp_write call.  ``align``: the data's start modulo 16.  ``nseg``: the segment count the
    descriptors claim (default: the true one).  ``bad``: the test expects the flow rejected."""

    def __init__(self, tmpl, data, mss, align=0, nseg=None, bad=False, hl=None):
        self.tmpl, self.data, self.mss, self.align, self.bad = bytes(tmpl), bytes(data), int(mss), int(align), bad
        self.hl = len(self.tmpl) if hl is None else hl
        true = -(-len(self.data) // self.mss) if self.mss else 0
        self.nseg = true if nseg is None else nseg


def data_bytes(seed, n):
    return O.splitmix64_bytes(seed, n).tobytes() if n else b""


def lay(flows, head_align=0, seed=1, stride=None, tail=48):
    """The flows in an arena of random bytes: each send's data at its alignment, then the head
    region (its start modulo 16 = head_align), the flows' head ranges back to back.  Returns the
    arena and every descriptor array of the form, from numpy alone."""
    nfl = len(flows)
    stride = stride or max([len(f.tmpl) for f in flows] + [1])
    at, po = 64, []
    for f in flows:
        at = (at + 15) // 16 * 16 + f.align
        po.append(at)
        at += len(f.data) + 3
    hfirst = (at + 15) // 16 * 16 + head_align
    nseg = np.array([f.nseg for f in flows], dtype=np.int64)
    hl = np.array([f.hl for f in flows], dtype=np.int64)
    seg_first = np.zeros(nfl + 1, dtype=np.int64)
    np.cumsum(nseg, out=seg_first[1:])
    ho = hfirst + np.concatenate(([0], np.cumsum(nseg * hl)[:-1])) if nfl else np.zeros(0, dtype=np.int64)
    size = int(hfirst + (nseg * hl).sum()) + tail
    arena = np.frombuffer(O.splitmix64_bytes(seed ^ 0x5E6, size).tobytes(), dtype=np.uint8).copy()
    tm = np.frombuffer(O.splitmix64_bytes(seed ^ 0x7E3, max(nfl, 1) * stride).tobytes(), dtype=np.uint8).copy()
    tm = tm.reshape(max(nfl, 1), stride)
    for i, f in enumerate(flows):
        arena[po[i]:po[i] + len(f.data)] = np.frombuffer(f.data, dtype=np.uint8)
        k = min(len(f.tmpl), stride)
        tm[i, :k] = np.frombuffer(f.tmpl[:k], dtype=np.uint8)
    n_seg = int(seg_first[-1])
    owner = np.repeat(np.arange(nfl), nseg)                       # the flow of every segment
    blk_flow = owner[::64].astype(np.uint32) if n_seg else np.zeros(0, dtype=np.uint32)
    return SimpleNamespace(flows=flows, arena=arena, tmpl=tm[:nfl], stride=stride, hl=hl.astype(np.uint8),
                           po=np.array(po, dtype=np.uint64), pl=np.array([len(f.data) for f in flows], dtype=np.uint32),
                           mss=np.array([f.mss for f in flows], dtype=np.uint16), ho=ho.astype(np.uint64),
                           seg_first=seg_first.astype(np.uint32), blk_flow=blk_flow, n_seg=n_seg, owner=owner,
                           head_end=int(hfirst + (nseg * hl).sum()))


def chains(L, good_only=True):
    """The [head, data slice] chains of the flows' segments (of the flows not marked bad) and the
    index of each chain's segment: (frag_off, frag_len, first, seg)."""
    off, ln, seg = [], [], []
    for i, f in enumerate(L.flows):
        if good_only and f.bad:
            continue
        for j in range(f.nseg):
            off += [int(L.ho[i]) + j * f.hl, int(L.po[i]) + j * f.mss]
            ln += [f.hl, min(f.mss, len(f.data) - j * f.mss)]
            seg.append(int(L.seg_first[i]) + j)
    first = 2 * np.arange(len(seg) + 1)
    return (np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint32), first.astype(np.uint32),
            np.array(seg, dtype=np.int64))


def with_heads(L):
    """A copy of the arena with the head of every segment of the flows not marked bad written,
    both checksum fields zero."""
    a = L.arena.copy()
    for i, f in enumerate(L.flows):
        if f.bad:
            continue
        for j in range(f.nseg):
            h = head(f.tmpl, j, f.mss, min(f.mss, len(f.data) - j * f.mss))
            o = int(L.ho[i]) + j * f.hl
            a[o:o + f.hl] = np.frombuffer(h, dtype=np.uint8)
    return a


def expected(oracle, L):
    """(arena, status per segment, the chains): the heads finalized by the oracle; the segments of
    flows marked bad RNS_TX_MALFORMED, their head ranges as they were."""
    a = with_heads(L)
    off, ln, first, seg = chains(L)
    st = np.full(L.n_seg, 0x80, dtype=np.uint8)
    st[seg] = oracle.tx_chain_fill(a, off, ln, first)
    return a, st, (off, ln, first, seg)


def datagrams(arena, ch):
    """The datagrams of the chains, gathered from a finalized arena."""
    off, ln, first, _ = ch
    return [b"".join(arena[int(off[k]):int(off[k]) + int(ln[k])].tobytes() for k in range(first[i], first[i + 1]))
            for i in range(first.size - 1)]
