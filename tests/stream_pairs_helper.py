"""Batch pairs (X, Y) for the stream and graph-replay tests, with their references.  Nothing here touches a device.

A captured call is fixed in its by-value arguments and its pointers; everything else may change between replays.
So every family gets two batches that agree in every count, cap and array size and differ in every array: the
same number of datagrams in the same number of pool buffers (a few filler datagrams at the end of each batch even
the buffer counts out), other addresses, ports, flags, sequence numbers, payload bytes, socket states and free
lists.  The datagrams come from the families' own builders (rx_place_helper, tcp_listen_helper, udp_demux_helper,
icmp_echo_helper, tx_plan_helper, rx_flow_helper), the references from the host twins in the package and from
those helpers, computed once per process and shared by tests/test_stream_pairs_ref.py (which asserts what the
pairs are built to have) and tests/test_gpu_streams.py.

A ``Batch`` names its arrays by role: ``ins`` the call only reads, ``io`` it updates in place (their contents
before the call), ``want`` holds the bytes every ``io`` and output array must hold after it — POISON wherever the
call writes nothing, because that is what the harness fills outputs with — and ``slack`` marks the bytes of an
array the entry's contract leaves unspecified (the families' own mask_slack rules).
"""
from functools import lru_cache
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np

import icmp_echo_helper as EH
import rx_flow_helper as FH
import rx_place_helper as P
import tcp_listen_helper as LH
import tx_plan_helper as PH
import udp_demux_helper as DH
from oracle.oracle import get_oracle
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.conn import close_host, conn_update_host, ctl_heads_host
from rustnetworkstack_amd.flow import FLOW_DTYPE, flow_update_host
from rustnetworkstack_amd.icmp import echo_host
from rustnetworkstack_amd.listen import ACCEPT_DTYPE, listen_host
from rustnetworkstack_amd.place import META_DTYPE, rx_flow_table
from rustnetworkstack_amd.send import plan_host
from rustnetworkstack_amd.udp import REC, demux_host, port_table, send_host
from test_gpu_tx import outgoing
from test_gpu_tx_chain_packed import cut
from test_gpu_udp_demux import mask_slack as demux_mask_slack
from tx_pool_helper import expand, lay_pool as lay_tx_pool, mask_slack as tx_mask_slack

POISON = 0xEE          # what the harness fills every output with before a run (gpu_guard.FILL)
B = 256                # bytes per pool buffer, receive and transmit
N = 650                # datagrams: two scan blocks of 256, two 64-item blocks and a partial one; a second demux tile
FILLERS = 12           # the datagrams at the end of a batch that even the buffer counts out
NFL, PEND_CAP = 84, 4  # flows (one-segment ones: the lane path; longer lists: the wave path) and pending entries each
STREAM_BYTES = 1 << 17
ECHO_CAP, SEND_CAP = 480, 500      # between the two batches' request / send counts: NOBUF in Y alone
SEG_CAP, HEAD0 = 1536, 1 << 21     # the plan's segment cap and where its heads go in the arena
ARENA_BYTES = HEAD0 + 60 * SEG_CAP + 64
M32 = 0xFFFFFFFF
L4, L6 = P.L4, P.L6


class Batch(NamedTuple):
    args: dict   # the by-value arguments of the calls: equal in X and Y
    ins: dict    # name -> array the calls only read
    io: dict     # name -> array the calls update in place, as it is before them
    want: dict   # name -> the bytes of every io and output array after the calls
    slack: dict  # name -> bool per byte: True where the contract leaves the byte unspecified
    info: dict   # what the conditions in test_stream_pairs_ref.py are asserted on


def poison(nbytes, dtype=np.uint8):
    return np.full(nbytes, POISON, np.uint8).view(dtype)


def padded(a, n, dtype):
    """``a`` as the first entries of an n-entry array that holds POISON in the rest."""
    out = poison(n * np.dtype(dtype).itemsize, dtype)
    out[:len(a)] = a
    return out


def _bufs(pkts):
    return sum(-(-len(p) // B) for p in pkts)


def _even_out(x, y, filler):
    """FILLERS datagrams appended to each list so that both take the same number of B-byte buffers:
    ``filler(j, nbytes)`` is a datagram of exactly nbytes bytes that the family under test passes by."""
    assert len(x) == len(y) == N - FILLERS
    target = max(_bufs(x), _bufs(y)) + FILLERS
    out = []
    for pk in (x, y):
        extra = target - _bufs(pk) - FILLERS
        more = [1 + extra // FILLERS + (1 if j < extra % FILLERS else 0) for j in range(FILLERS)]
        out.append(pk + [filler(j, (b - 1) * B + 60 + j) for j, b in enumerate(more)])
        assert _bufs(out[-1]) == target and len(out[-1]) == N
    return out


def _interleave(streams, rng):
    """Lists of datagrams merged by a seeded shuffle, each list's own order kept."""
    slots = np.repeat(np.arange(len(streams)), [len(s) for s in streams])
    rng.shuffle(slots)
    it = [iter(s) for s in streams]
    return [next(it[k]) for k in slots]


def _size(rng):
    """A payload length: mostly inside one buffer, one in ten in two or three."""
    return int(rng.integers(229, 520)) if rng.random() < 0.1 else int(rng.integers(0, 200))


def _slack_of(mask_fn, nbytes, *args):
    """A family's mask_slack rule as a bool mask: it copies ref into got over the unspecified bytes."""
    got, ref = np.zeros(nbytes, np.uint8), np.ones(nbytes, np.uint8)
    mask_fn(got, ref, *args)
    return got.astype(bool)


# ---------------------------------------------------------------------------
# TCP: placement, flow update, ACK build, connection update, control build, close step, listen responder
# ---------------------------------------------------------------------------
STATES = (1, 1, 1, 2, 1, 3, 1, 5, 1, 1, 6, 1)  # Established, SynReceived, CloseWait, FinWait1, FinWait2


def _tcp_raw(v):
    """Batch v's datagrams (without the fillers) and its flows: 84 known flows of 1..14 segments (other lengths per
    flow in Y: the counts rotate), in order and out of order, pure ACKs, FINs and an RST; 16 new keys as strays, SYNs,
    duplicate SYNs and third ACKs (Y: other keys, a quarter of them to a closed port); strays; UDP and ICMP."""
    rng = np.random.default_rng(4100 + v)
    counts = np.roll(np.array([1 if f % 3 == 0 else 2 + (f * 7) % 13 for f in range(NFL)]), 5 * v)
    dport = (80, 8080)[v]
    keys, flows, streams = [], np.zeros(NFL, FLOW_DTYPE), []
    next_seq, win_off, win_len = [], [], []
    tmpl, hl8 = np.zeros((NFL, 64), np.uint8), np.zeros(NFL, np.uint8)
    at = 16
    for f in range(NFL):
        src = (LH.v6 if f % 4 == 3 else LH.v4)(f + 1000 * v)
        sport = 40000 + 2000 * v + f
        keys.append(P.key_of(src, sport, dport))
        base = (0xFFFFF000 + 0x10000 * f + 0x333 * v) & M32                 # the first flows' numbers wrap
        una = 5000 + f + 77 * v
        flows[f] = FH.flow_rec(rcv_nxt=base, rcv_max=base, snd_una=una, snd_nxt=una + 400, snd_wnd=1000, snd_wl1=(base - 1) & M32,
                               snd_wl2=una, rq_len=10 * f, delayed_acks=(f + v) % 5, state=STATES[(f + 2 * v) % len(STATES)],
                               ack_timer=f & 1).item()
        c = int(counts[f])
        lens = [0 if rng.random() < 0.2 else _size(rng) % 500 for _ in range(c)]
        q = list(range(c))
        if c >= 3 and f % 4 == 1:
            q[1], q[2] = q[2], q[1]                                         # the second arrival is the third in sequence
        seq, pos = [0] * c, 0
        for j in q:
            seq[j] = (base + pos) & M32
            pos += lens[j]
        if c >= 4 and f % 8 == 5:                                           # a hole before the last segment: it stays pending
            lens[c - 1] = max(lens[c - 1], 7)
            seq[c - 1] = (seq[c - 1] + 1000) & M32
            pos += 1000 + 7
        segs = []
        for k in range(c):
            flags = P.ACK | P.PSH if lens[k] else P.ACK
            if k == c - 1 and (f + v) % 5 == 0:
                flags |= P.FIN
            if k == 1 and (f + v) % 17 == 3:
                flags = P.RST
            segs.append(LH.seg(src, sport, dport, seq[k], flags, body=P.body_bytes(97 * f + k + 5000 * v, lens[k]),
                               ack=una + 10 * (k + 1), window=0x1000 + k))
        streams.append(segs)
        next_seq.append(base)
        win_off.append(at)
        win_len.append(pos + 32)
        at += (pos + 32 + 15) // 16 * 16
        t = FH.template(L6 if len(src) == 16 else L4, src, dport, sport)
        tmpl[f, :len(t)], hl8[f] = np.frombuffer(t, dtype=np.uint8), len(t)
    busy = [f for f in range(5 + 10 * v, NFL) if flows[f]["state"] == 1 and counts[f] >= 10 and f % 4 != 3]
    hl8[busy[-v]] = 44                                                      # one malformed template, on a flow that ACKs
    pend = np.zeros((NFL, PEND_CAP, 2), np.uint32)
    for f in range(2, NFL, 8):                                              # a segment pending from an earlier batch
        flows[f]["n_pend"], pend[f, 0] = 1, ((int(flows[f]["rcv_nxt"]) + 5000) & M32, 10 + f)
    assert at <= STREAM_BYTES
    ports, closed = ([80, 443], [8080, 25])[v], (81, 26)[v]
    for k in range(16):
        src = (LH.v6 if k % 4 == 3 else LH.v4)(200 + k + 1000 * v)
        sp = 5000 + 1000 * v + k
        if v == 0:
            dp = ports[k & 1]
            s = [LH.seg(src, sp, dp, 100 + k, P.ACK), LH.seg(src, sp, dp, 200 + k, P.SYN, LH.MSS),
                 LH.seg(src, sp, dp, 200 + k, P.SYN, LH.MSS), LH.seg(src, sp, dp, 201 + k, P.ACK, ack=777)]
        else:
            dp = closed if k >= 12 else ports[k & 1]
            s = [LH.seg(src, sp, dp, 300 + k, P.SYN, LH.MSS if k & 2 else b""), LH.seg(src, sp, dp, 301 + k, P.ACK, ack=778),
                 LH.seg(src, sp, dp, 300 + k, P.SYN), LH.seg(src, sp, dp, 301 + k, P.ACK | P.PSH, body=b"hello")]
        streams.append(s)
    streams += [[LH.seg(LH.v4(300 + j + 1000 * v), 7000 + j, closed, j, P.ACK)] for j in range(6)]
    have = sum(len(s) for s in streams)
    for j in range(N - FILLERS - have):
        streams.append([P.udp4(P.R4, bytes(j % 40)) if j & 1 else P.icmp4(P.R4, bytes(8 + j % 30))])
        if j % 9 == 2 + v:                                                  # a known flow's segment whose TCP checksum fails
            bad = bytearray(LH.seg(LH.v4(1000 * v), 40000 + 2000 * v, dport, 77, P.ACK | P.PSH, body=bytes([j]) * 9))
            bad[-1] ^= 0x40
            streams[-1] = [bytes(bad)]
    return SimpleNamespace(pkts=_interleave(streams, rng), keys=keys, flows=flows, next_seq=np.array(next_seq, np.uint32),
                           win_off=np.array(win_off, np.uint64), win_len=np.array(win_len, np.uint32), tmpl=tmpl, hl8=hl8,
                           ports=ports, add=np.array([(5, 0x10040)[v]], np.uint32),
                           iss=np.array(LH.iss_of(N), np.uint32) + np.uint32(v), pend=pend)


@lru_cache(maxsize=None)
def tcp_base():
    """Both TCP batches laid into pools, with the placement's reference (rx_place_helper.expected): every other TCP
    family starts from its records."""
    raw = [_tcp_raw(0), _tcp_raw(1)]
    pk = _even_out(raw[0].pkts, raw[1].pkts, lambda j, nbytes: P.udp4(P.R4, bytes(nbytes - 28)))
    for v, t in enumerate(raw):
        t.pkts = pk[v]
        t.pool, idx, blk, t.len16 = P.lay_pool(t.pkts, B, shuffled=True, seed=11 + v)
        t.idx, t.blk = idx.astype(np.uint32), blk.astype(np.uint32)
        t.table = rx_flow_table(t.keys)
        t.status, t.l4, meta, t.stream = P.expected(t.pkts, B, t.keys, t.next_seq, t.win_off, t.win_len, poison(STREAM_BYTES),
                                                    ones_comp=get_oracle().compute_ones_comp)
        t.meta = meta.view(META_DTYPE)
        t.listen_tbl = port_table(t.ports)
        t.args = dict(n_pkts=N, n_frags=int(t.idx.size), pool_bytes=int(t.pool.size), buf_bytes=B, n_flows=NFL,
                      tbl_bytes=int(t.table.size), stream_bytes=STREAM_BYTES, local=(L4, L6))
        t.pool_ins = dict(pool=t.pool, idx=t.idx, blk=t.blk, len16=t.len16)
        t.place_ins = dict(t.pool_ins, table=t.table, next_seq=t.next_seq, win_off=t.win_off, win_len=t.win_len)
    return raw


def _pend_slack(flows_out):
    """The pending lists' entries past n_pend (same_update / same_conn compare the valid ones)."""
    m = np.ones((NFL, PEND_CAP, 8), bool)
    for f in range(NFL):
        if flows_out[f]["n_pend"] <= PEND_CAP:
            m[f, :int(flows_out[f]["n_pend"])] = False
    return m.reshape(-1)


def _pair(make):
    return tuple(make(t, v) for v, t in enumerate(tcp_base()))


@lru_cache(maxsize=None)
def verify_pair():
    return _pair(lambda t, v: Batch(t.args, t.pool_ins, {}, dict(status=t.status, l4=t.l4), {}, {}))


@lru_cache(maxsize=None)
def place_pair():
    return _pair(lambda t, v: Batch(t.args, t.place_ins, dict(stream=poison(STREAM_BYTES)),
                                    dict(status=t.status, l4=t.l4, meta=t.meta, stream=t.stream), {}, {}))


def _flow_ref(t):
    if not hasattr(t, "flow"):
        t.flow = flow_update_host(t.meta, t.flows, t.pend, PEND_CAP)
    return t.flow


def _conn_ref(t):
    if not hasattr(t, "conn"):
        t.conn = conn_update_host(t.meta, t.flows, t.pend, PEND_CAP)
    return t.conn


def _update_batch(t, ref, third):
    fo, po, rec, res = ref
    args = dict(n_pkts=N, n_flows=NFL, pend_cap=PEND_CAP)
    return Batch(args, dict(meta=t.meta, flows=t.flows, pend=t.pend), {}, {"flows_out": fo, "pend_out": po, third: rec, "res": res},
                 dict(pend_out=_pend_slack(fo)), dict(n_segs=res["n_segs"].copy(), res=res))


@lru_cache(maxsize=None)
def flow_pair():
    return _pair(lambda t, v: _update_batch(t, _flow_ref(t), "seg"))


@lru_cache(maxsize=None)
def conn_pair():
    return _pair(lambda t, v: _update_batch(t, _conn_ref(t), "ctl"))


ACK_ID, CTL_ID, LISTEN_ID = 0xFFF0, 0xFFC0, 0xFFE0  # the ids wrap inside every batch


def _ack_want(t):
    """tx_ack_build's outputs from rx_flow_helper.ack_heads_ref over the flow update's reference."""
    fo, _, seg, _ = _flow_ref(t)
    heads, v4s = FH.ack_heads_ref(t.meta, seg, fo, [bytes(r) for r in t.tmpl], t.hl8, ACK_ID)
    out, src, len8 = poison(64 * N), poison(4 * N, np.uint32), poison(N)
    for k, (i, h) in enumerate(heads):
        src[k], len8[k] = i, 0 if h is None else len(h)
        if h is not None:
            out[64 * k:64 * k + len(h)] = np.frombuffer(h, dtype=np.uint8)
    return dict(out=out, ack_src=src, ack_len8=len8, n_acks=np.array([len(heads), v4s], np.uint32))


@lru_cache(maxsize=None)
def ack_pair():
    def make(t, v):
        fo, _, seg, _ = _flow_ref(t)
        return Batch(dict(n_pkts=N, n_flows=NFL, ip_id_base=ACK_ID, ack_cap=N, tmpl_stride=64),
                     dict(meta=t.meta, seg=seg, flows=fo, tmpl=t.tmpl, head_len8=t.hl8), {}, _ack_want(t), {}, {})
    return _pair(make)


def _ctl_want(ctl, t, add):
    out, src, len8, count = ctl_heads_host(ctl, NFL, t.tmpl, t.hl8, CTL_ID, out_cap=N, ip_id_add=add, tmpl_stride=64,
                                           out=poison(64 * N), src=poison(4 * N, np.uint32), len8=poison(N))
    return dict(out=out, src=src, len8=len8, count=count)


@lru_cache(maxsize=None)
def ctl_pair():
    def make(t, v):
        ctl = _conn_ref(t)[2]
        return Batch(dict(n_pkts=N, n_flows=NFL, ip_id_base=CTL_ID, out_cap=N, tmpl_stride=64),
                     dict(ctl=ctl, tmpl=t.tmpl, head_len8=t.hl8, ip_id_add=t.add), {}, _ctl_want(ctl, t, int(t.add[0])), {}, {})
    return _pair(make)


@lru_cache(maxsize=None)
def close_pair():
    def make(t, v):
        flows = _conn_ref(t)[0]
        op = np.array([1 if (f + v) % 3 else (f + v) % 4 for f in range(NFL)], np.uint8)
        fo, ctl = close_host(flows, op)
        return Batch(dict(n_flows=NFL), dict(flows=flows, op=op), {}, dict(flows_out=fo, ctl=ctl), {}, {})
    return _pair(make)


def _listen_ref(t):
    if not hasattr(t, "listen"):
        t.listen = listen_host(t.pool, t.idx, t.blk, t.len16, L4, L6, t.meta, t.listen_tbl, len(t.ports), t.iss, buf_bytes=B,
                               reply_cap=N, ip_id_base=LISTEN_ID, ip_id_add=int(t.add[0]), out=poison(64 * N),
                               rep_src=poison(4 * N, np.uint32), rep_len8=poison(N), accept=poison(72 * N, ACCEPT_DTYPE))
    return t.listen


def _listen_want(t, prefix=""):
    e = _listen_ref(t)
    return {prefix + k: getattr(e, k) for k in ("conn", "out", "rep_src", "rep_len8", "accept", "count")}


def _listen_info(t):
    e = _listen_ref(t)
    acc = e.accept[:int(e.count[2])]["key"]
    return dict(count=e.count, later=int(((e.conn & _lib.RNS_CONN_LATER) != 0).sum()), port_map={k.tobytes() for k in acc})


@lru_cache(maxsize=None)
def listen_pair():
    def make(t, v):
        args = dict(t.args, n_listen=len(t.ports), reply_cap=N, ip_id_base=LISTEN_ID)
        return Batch(args, dict(t.pool_ins, meta=t.meta, listen_tbl=t.listen_tbl, iss=t.iss, ip_id_add=t.add), {},
                     _listen_want(t), {}, _listen_info(t))
    return _pair(make)


@lru_cache(maxsize=None)
def tcp_conn_chain_pair():
    """conn.tcp_conn: verify + placement, listen responder, connection update, control build (its ids after the
    replies': the reply count is added on the device)."""
    def make(t, v):
        fo, po, ctl, res = _conn_ref(t)
        want = dict(status=t.status, meta=t.meta, stream=t.stream, flows_out=fo, pend_out=po, ctl=ctl, res=res)
        want.update(_listen_want(t, "l_"))
        heads = ctl_heads_host(ctl, NFL, t.tmpl, t.hl8, LISTEN_ID, out_cap=N, ip_id_add=int(t.add[0]) + int(_listen_ref(t).count[1]),
                               tmpl_stride=64, out=poison(64 * N), src=poison(4 * N, np.uint32), len8=poison(N))
        want.update(zip(("out", "src", "len8", "count"), heads))
        ins = dict(t.place_ins, listen_tbl=t.listen_tbl, iss=t.iss, flows=t.flows, pend=t.pend, tmpl=t.tmpl, head_len8=t.hl8,
                   ip_id_add=t.add)
        args = dict(t.args, n_listen=len(t.ports), pend_cap=PEND_CAP, ip_id_base=LISTEN_ID)
        return Batch(args, ins, dict(stream=poison(STREAM_BYTES)), want, dict(pend_out=_pend_slack(fo)), _listen_info(t))
    return _pair(make)


@lru_cache(maxsize=None)
def place_flow_ack_chain_pair():
    def make(t, v):
        fo, po, seg, res = _flow_ref(t)
        want = dict(status=t.status, l4=t.l4, meta=t.meta, stream=t.stream, flows_out=fo, pend_out=po, seg=seg, res=res)
        want.update(_ack_want(t))
        args = dict(t.args, pend_cap=PEND_CAP, ip_id_base=ACK_ID, ack_cap=N, tmpl_stride=64)
        return Batch(args, dict(t.place_ins, flows=t.flows, pend=t.pend, tmpl=t.tmpl, head_len8=t.hl8),
                     dict(stream=poison(STREAM_BYTES)), want, dict(pend_out=_pend_slack(fo)), {})
    return _pair(make)


# ---------------------------------------------------------------------------
# UDP: demux, send build, demux -> send
# ---------------------------------------------------------------------------
UDP_PORTS = ([53, 5353, 4000, 700, 9999], [5353, 700, 53, 8080, 4000])
UDP_WEIGHTS = ([0.25, 0.05, 0.15, 0.10, 0.05, 0.40], [0.10, 0.30, 0.20, 0.15, 0.20, 0.05])  # the last: an unbound port
NTX = 3 * N            # transmit buffers (and free-list entries): enough for every datagram of either batch
UDP_ID = 0xFFF8


def _udp_raw(v):
    rng = np.random.default_rng(5200 + v)
    ports = UDP_PORTS[v]
    pkts = []
    for k in range(N - FILLERS):
        r = (k + 5 * v) % 23
        if r == 7:
            pkts.append(P.segment(P.R4, 1234, ports[0], 1000 + k, P.body_bytes(k, 20 + k % 50)))
            if k % 3 == v:                                                  # its TCP checksum fails: an L4 sum that is not 0
                pkts[-1] = pkts[-1][:-1] + bytes([pkts[-1][-1] ^ 0x40])
        elif r == 15:
            pkts.append(P.icmp4(P.R4, bytes(8 + k % 30)))
        else:
            pkts.append(DH.any_udp(k + 3000 * v, int(rng.choice(ports + [9], p=UDP_WEIGHTS[v])), _size(rng)))
        if r == 20 and k % 4 == v:                                          # an IP header checksum that fails: not accepted
            bad = bytearray(pkts[-1])
            if bad[0] >> 4 == 4:
                bad[10] ^= 0x40
                pkts[-1] = bytes(bad)
    return pkts


def _tx_pool0(seed):
    tx0 = np.full(NTX * B, 0xA5, np.uint8)
    tx0[::7] = np.arange(tx0[::7].size, dtype=np.uint8) + np.uint8(seed)   # a buffer written to the wrong place shows
    return tx0


def _tx_want(r, cap, tx, free):
    """The transmit form's outputs (tx_blk_first, tx_head_len8, tx_pay_len16, tx_src, count) padded to the cap's
    sizes, the pool after the build and its slack."""
    bf, hl, pl, src, count = r
    want = dict(tx_blk_first=padded(bf, (cap + 63) // 64, np.uint32), tx_head_len8=padded(hl, cap, np.uint8),
                tx_pay_len16=padded(pl, cap, np.uint16), tx_src=padded(src, cap, np.uint32), count=count, tx_pool=tx)
    return want, dict(tx_pool=_slack_of(tx_mask_slack, tx.size, free, bf, hl, pl, B))


@lru_cache(maxsize=None)
def udp_base():
    pk = _even_out(_udp_raw(0), _udp_raw(1), lambda j, nbytes: P.icmp4(P.R4, bytes(nbytes - 28)))
    out = []
    for v in (0, 1):
        u = SimpleNamespace(pkts=pk[v], ports=np.array(UDP_PORTS[v], np.uint16), tbl=port_table(UDP_PORTS[v]))
        u.pool, idx, blk, u.len16 = P.lay_pool(u.pkts, B, shuffled=True, seed=21 + v)
        u.idx, u.blk = idx.astype(np.uint32), blk.astype(np.uint32)
        u.data_bytes = int(u.idx.size) * B
        data, rec = poison(u.data_bytes), poison(32 * N, REC)
        u.demux = demux_host(u.pool, u.idx, u.blk, u.len16, L4, L6, u.tbl, len(u.ports), buf_bytes=B, rec_cap=N, data=data, rec=rec)
        e = u.demux
        u.demux_want = dict(status=e.status, l4=e.l4_sum, udp=e.udp, pos=e.pos, rec=e.rec, q_first=e.q_first, count=e.count,
                            data=e.data)
        u.demux_slack = dict(data=_slack_of(demux_mask_slack, u.data_bytes, e))
        u.demux_ins = dict(pool=u.pool, idx=u.idx, blk=u.blk, len16=u.len16, port_tbl=u.tbl)
        u.demux_args = dict(n_pkts=N, n_frags=int(u.idx.size), pool_bytes=int(u.pool.size), buf_bytes=B, n_socks=len(u.ports),
                            rec_cap=N, data_bytes=u.data_bytes, local=(L4, L6))
        u.free = np.random.default_rng(40 + v).permutation(NTX).astype(np.uint32)
        u.add = np.array([(3, 0x2FFF0)[v]], np.uint32)
        u.tx0 = _tx_pool0(v)
        tx = u.tx0.copy()
        u.send = send_host(e.data, e.rec, e.q_first, u.ports, L4, L6, tx, u.free, buf_bytes=B, n_recs=N, send_cap=SEND_CAP,
                           ip_id_base=UDP_ID, ip_id_add=int(u.add[0]))
        u.send_want, u.send_slack = _tx_want(tuple(u.send)[1:], SEND_CAP, tx, u.free)
        u.send_want["send"] = u.send.send
        u.send_args = dict(n_recs=N, n_socks=len(u.ports), send_cap=SEND_CAP, n_free=NTX, tx_bytes=NTX * B, buf_bytes=B,
                           ip_id_base=UDP_ID, local=(L4, L6))
        u.info = dict(queues=np.diff(e.q_first.astype(np.int64)), count=e.count, send=u.send.send, send_count=u.send.count)
        out.append(u)
    return out


@lru_cache(maxsize=None)
def demux_pair():
    return tuple(Batch(u.demux_args, u.demux_ins, {}, u.demux_want, u.demux_slack, u.info) for u in udp_base())


@lru_cache(maxsize=None)
def udp_send_pair():
    return tuple(Batch(u.send_args, dict(data=u.demux.data, rec=u.demux.rec, q_first=u.demux.q_first, sock_port=u.ports,
                                         free=u.free, ip_id_add=u.add), dict(tx_pool=u.tx0), u.send_want, u.send_slack, u.info)
                 for u in udp_base())


@lru_cache(maxsize=None)
def demux_send_chain_pair():
    return tuple(Batch(dict(u.demux_args, **u.send_args), dict(u.demux_ins, sock_port=u.ports, free=u.free, ip_id_add=u.add),
                       dict(tx_pool=u.tx0), dict({"d_count" if k == "count" else k: w for k, w in u.demux_want.items()}, **u.send_want),
                       dict(u.demux_slack, **u.send_slack), u.info)
                 for u in udp_base())


# ---------------------------------------------------------------------------
# ICMP echo
# ---------------------------------------------------------------------------
ECHO_ID = 0xFFD0


def _icmp_raw(v):
    """Six datagrams in ten are echo requests in X, nine in ten in Y (more than ECHO_CAP); the others are echo
    replies, TCP and UDP."""
    rng = np.random.default_rng(6300 + v)
    pkts = []
    for k in range(N - FILLERS):
        n, r = _size(rng), (k * 7 + 3 * v) % 10
        body = EH.body(k + 2000 * v, n)
        if r < (6, 9)[v]:
            pkts.append(EH.ping6(body, src=EH.R6B if k & 8 else EH.R6) if k % 3 == 1 else
                        EH.ping4(body, src=EH.R4B if k & 8 else EH.R4, ihl=5 + k % 3))
        elif r == 9:
            pkts.append(EH.udp4(n) if k & 1 else EH.tcp4(n))
        else:
            pkts.append(EH.ping4(body, typ=0, corrupt=k % 4 == v))          # some with a checksum that fails
    return pkts


@lru_cache(maxsize=None)
def echo_pair():
    pk = _even_out(_icmp_raw(0), _icmp_raw(1), lambda j, nbytes: P.udp4(P.R4, bytes(nbytes - 28)))
    out = []
    for v in (0, 1):
        rx, idx, blk, len16 = P.lay_pool(pk[v], B, shuffled=True, seed=31 + v)
        idx, blk = idx.astype(np.uint32), blk.astype(np.uint32)
        free = np.random.default_rng(50 + v).permutation(NTX).astype(np.uint32)
        add = np.array([(9, 0x3FFE0)[v]], np.uint32)
        tx0 = _tx_pool0(7 + v)
        tx = tx0.copy()
        st, l4, echo, *form = echo_host(rx, idx, blk, len16, L4, L6, tx, free, buf_bytes=B, reply_cap=ECHO_CAP, ip_id_base=ECHO_ID,
                                        ip_id_add=int(add[0]))
        want, slack = _tx_want(tuple(form), ECHO_CAP, tx, free)
        want.update(status=st, l4=l4, echo=echo)
        args = dict(n_pkts=N, n_frags=int(idx.size), pool_bytes=int(rx.size), buf_bytes=B, reply_cap=ECHO_CAP, n_free=NTX,
                    tx_bytes=NTX * B, ip_id_base=ECHO_ID, local=(L4, L6))
        out.append(Batch(args, dict(pool=rx, idx=idx, blk=blk, len16=len16, free=free, ip_id_add=add), dict(tx_pool=tx0), want, slack,
                         dict(echo=echo, count=form[-1])))
    return tuple(out)


# ---------------------------------------------------------------------------
# the pool transmit finalize
# ---------------------------------------------------------------------------
@lru_cache(maxsize=None)
def tx_fill_pair():
    """Datagrams of every kind the transmit path hands over (test_gpu_tx.outgoing) with unfinished checksum fields;
    Y holds X's datagrams in another order, in other buffers of a pool with other bytes around them."""
    heads, pays = cut(outgoing(N, 0x57E4))
    perm = np.random.default_rng(8).permutation(N)
    out = []
    for v in (0, 1):
        h, p = (heads, pays) if v == 0 else ([heads[i] for i in perm], [pays[i] for i in perm])
        pool, idx, blk, hl, pl, _ = lay_tx_pool(h, p, B, shuffled=True, seed=61 + v)
        idx, blk = idx.astype(np.uint32), blk.astype(np.uint32)
        off, ln, first = expand(idx, blk, hl, pl, B)
        done = pool.copy()
        status = np.asarray(get_oracle().tx_chain_fill(done, off, ln, first), dtype=np.uint8)
        args = dict(n_pkts=N, n_frags=int(idx.size), pool_bytes=int(pool.size), buf_bytes=B)
        out.append(Batch(args, dict(idx=idx, blk=blk, head_len8=hl, pay_len16=pl), dict(pool=pool), dict(status=status, pool=done), {}, {}))
    return tuple(out)


# ---------------------------------------------------------------------------
# TCP send planning, segmentation, plan -> segment
# ---------------------------------------------------------------------------
PLAN_FLOWS = 90
PLAN_KEYS = ("tmpl", "head_len8", "pay_off", "pay_len", "mss", "head_off", "seg_first", "blk_flow", "n", "res", "flows_out")
PLAN_ID = 0xFFF0


def _plan_specs(v):
    """tx_plan_helper.mixed_specs' mixture with send buffers of a few KiB: empty, stopped and busy flows, IPv4 and IPv6."""
    rng = np.random.default_rng(900 + v)
    out = []
    for i in range(PLAN_FLOWS):
        kind = int(rng.integers(0, 10))
        d = dict(una=int(rng.integers(0, 1 << 32)), v6=bool(rng.integers(0, 2)), rq_len=int(rng.integers(0, 0x11000)),
                 a=int(rng.integers(0, 500)), mss=int(rng.choice([536, 1220, 1460])))
        if kind == 0:
            d.update(unsent=0, inflight=100 * (i & 1), rexmit=0)
        elif kind == 1:
            d.update(state=int(rng.integers(2, 6)), unsent=500, inflight=20, rexmit=1)
        else:
            d.update(inflight=int(rng.integers(0, 3000)), wnd=int(rng.integers(0, 0x4000)), unsent=int(rng.integers(0, 8000)),
                     rexmit=int(rng.integers(0, 2)))
        out.append(d)
    return out


@lru_cache(maxsize=None)
def plan_base():
    out = []
    for v in (0, 1):
        c = PH.mk(_plan_specs(v), seg_cap=SEG_CAP, head_first_off=HEAD0, ip_id_base=PLAN_ID, ip_id_add=(7, 0x1FF00)[v])
        assert int((c["sq_off"] + c["sq_len"]).max()) < HEAD0
        s = SimpleNamespace(c=c, add=np.array([c["ip_id_add"]], np.uint32))
        s.plan = plan_host(c["flows"], c["sq_off"], c["sq_seq"], c["sq_len"], c["mss"], c["tmpl"], c["head_len8"], rexmit=c["rexmit"],
                           ip_id_base=PLAN_ID, ip_id_add=c["ip_id_add"], head_first_off=HEAD0, seg_cap=SEG_CAP, tmpl_out_fill=POISON)
        s.arena = np.frombuffer(np.random.default_rng(70 + v).bytes(ARENA_BYTES), dtype=np.uint8).copy()
        done, st = PH.heads_ref(s.plan, s.arena)
        s.done = done
        s.status = np.full(SEG_CAP, _lib.RNS_TX_MALFORMED, np.uint8)        # past the plan's count: no entry covers them
        s.status[:st.size] = st
        s.ins = dict(flows=c["flows"], sq_off=c["sq_off"], sq_seq=c["sq_seq"], sq_len=c["sq_len"], mss=c["mss"], tmpl=c["tmpl"],
                     head_len8=c["head_len8"], rexmit=c["rexmit"], ip_id_add=s.add)
        s.args = dict(n_flows=PLAN_FLOWS, stride=int(c["tmpl"].shape[1]), seg_cap=SEG_CAP, head_first_off=HEAD0, ip_id_base=PLAN_ID)
        s.want = {"p_" + k: s.plan[k] for k in PLAN_KEYS}
        s.info = dict(n=s.plan["n"].copy(), status=s.status)
        out.append(s)
    return out


@lru_cache(maxsize=None)
def plan_pair():
    return tuple(Batch(s.args, s.ins, {}, s.want, {}, s.info) for s in plan_base())


@lru_cache(maxsize=None)
def segment_pair():
    """tx_segment over the plan's reference descriptors with n_seg = SEG_CAP."""
    keys = PLAN_KEYS[:8]
    return tuple(Batch(dict(n_entries=2 * PLAN_FLOWS, n_seg=SEG_CAP, arena_bytes=ARENA_BYTES, stride=s.args["stride"]),
                       {k: s.plan[k] for k in keys}, dict(arena=s.arena), dict(status=s.status, arena=s.done), {}, s.info)
                 for s in plan_base())


@lru_cache(maxsize=None)
def tcp_send_chain_pair():
    return tuple(Batch(dict(s.args, arena_bytes=ARENA_BYTES), s.ins, dict(arena=s.arena), dict(s.want, status=s.status, arena=s.done),
                       {}, s.info) for s in plan_base())


PAIRS = {"rx_verify_pool": verify_pair, "rx_tcp_place_pool": place_pair, "rx_tcp_flow_update": flow_pair, "tx_ack_build": ack_pair,
         "rx_tcp_conn_update": conn_pair, "tx_tcp_ctl_build": ctl_pair, "tx_tcp_close": close_pair, "rx_tcp_listen_pool": listen_pair,
         "rx_udp_demux_pool": demux_pair, "tx_udp_send_pool": udp_send_pair, "rx_icmp_echo_pool": echo_pair,
         "tx_fill_pool": tx_fill_pair, "tx_tcp_plan": plan_pair, "tx_segment": segment_pair,
         "tcp_conn": tcp_conn_chain_pair, "place_flow_ack": place_flow_ack_chain_pair, "demux_send": demux_send_chain_pair,
         "tx_tcp_send": tcp_send_chain_pair}
