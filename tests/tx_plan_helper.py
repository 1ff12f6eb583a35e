"""Helpers of the TCP send planning tests (rns_tx_tcp_plan_dev): tcp_write's loop (tcp.rs:256-292),
retransmit (tcp.rs:329-348), send_packet (tcp.rs:402-447) and tcp_output's header fields
(tcp.rs:938-976) restated over a small ``Socket`` class — the literal piece-by-piece loop with seq_gt
as util.rs:155-158, not the closed form of the code under test — ``plan_ref``, which produces every
output array of the ABI from it, and ``heads_ref``, the finished datagrams of a plan.  Nothing here
calls the code under test."""
import numpy as np

from oracle import oracle as O
from rx_flow_helper import ESTABLISHED, FLOW, template_ok
from rx_place_helper import seq_gt
from tx_segment_helper import head

RES = np.dtype([("new_bytes", "<u4"), ("new_segs", "<u4"), ("rexmit_bytes", "<u4"), ("why", "u1"), ("pad", "u1", (3,))])
PLAN_NONE, PLAN_WINDOW, PLAN_STATE, PLAN_BAD, PLAN_TMPL, PLAN_CAP = range(6)
DOMAIN = 0x3FFFFFFF
MAX_RECEIVE_WINDOW = 0xFFFF
FLAG_ACK, FLAG_PSH = 0x10, 0x08
M32 = 0xFFFFFFFF
FILL = 0xEE
KEYS = ("tmpl", "head_len8", "pay_off", "pay_len", "mss", "head_off", "seg_first", "blk_flow", "n", "res", "flows_out")


class Socket:
    """The fields of TCPSocketState the send path reads, from a flow record; ``sent`` collects what
    send_packet hands to tcp_output: (seq_num, ack_num, flags, window, offset into the send buffer,
    length)."""

    def __init__(self, rec, send_mss, queue_len):
        self.state_established = int(rec["state"]) == ESTABLISHED
        self.send_unacked = int(rec["snd_una"])
        self.send_next_seq = int(rec["snd_nxt"])
        self.send_window = int(rec["snd_wnd"])
        self.send_mss = int(send_mss)
        self.next_expect = int(rec["rcv_nxt"])            # reassembler.get_next_expect()
        self.receive_queue_len = int(rec["rq_len"])
        self.retransmit_queue_len = queue_len             # the bytes of [send_unacked, send_next_seq)
        self.sent = []

    def send_packet(self, offset, length, flags):         # tcp.rs:402-447
        receive_window = (MAX_RECEIVE_WINDOW - (self.receive_queue_len & 0xFFFF)) & 0xFFFF    # tcp.rs:403
        ack_seq = self.next_expect                        # tcp.rs:408-417: + 0 in Established
        # tcp.rs:435-446: seq_num is send_next_seq, for retransmitted data too
        self.sent.append((self.send_next_seq, ack_seq, flags, receive_window, offset, length))

    def tcp_write(self, data_len):
        """tcp.rs:256-292 up to the first wait: returns the bytes sent."""
        offset = 0                                        # tcp.rs:256
        while offset < data_len:                          # tcp.rs:257
            packet_length = min(data_len - offset, self.send_mss)                             # tcp.rs:258
            max_segment = (self.send_unacked + self.send_window) & M32                        # tcp.rs:259
            if seq_gt((self.send_next_seq + packet_length) & M32, max_segment):               # tcp.rs:260-263
                return offset, True                       # tcp.rs:269: cond.wait — the plan ends here
            # tcp.rs:278-281: the piece data[offset..offset + packet_length], behind the retransmit queue
            self.send_packet(self.retransmit_queue_len + offset, packet_length, FLAG_ACK | FLAG_PSH)
            self.send_next_seq = (self.send_next_seq + packet_length) & M32                   # tcp.rs:282
            offset += packet_length                       # tcp.rs:283-284 (the queue grows; offsets stay relative to una)
        return offset, False

    def retransmit(self):                                 # tcp.rs:329-348
        if self.retransmit_queue_len:                     # tcp.rs:338
            # tcp.rs:341: append_from_buffer(&retransmit_queue, send_mss): its first min(len, mss) bytes
            self.send_packet(0, min(self.retransmit_queue_len, self.send_mss), FLAG_ACK | FLAG_PSH)   # tcp.rs:342


def row_ref(t, hl, seq_num, ack_num, flags, window, ident):
    """The template with the fields tcp_output (tcp.rs:947-951) and ip_output_v4 (ip.rs:147) set."""
    h = bytearray(t[:hl])
    ip = 20 if hl == 40 else 40
    h[ip + 4:ip + 8] = seq_num.to_bytes(4, "big")         # tcp.rs:947
    h[ip + 8:ip + 12] = ack_num.to_bytes(4, "big")        # tcp.rs:948
    h[ip + 12] = (20 // 4) << 4                           # tcp.rs:949
    h[ip + 13] = flags                                    # tcp.rs:950
    h[ip + 14:ip + 16] = window.to_bytes(2, "big")        # tcp.rs:951
    if hl == 40:
        h[4:6] = (ident & 0xFFFF).to_bytes(2, "big")
    return np.frombuffer(bytes(h), dtype=np.uint8)


def plan_ref(flows, sq_off, sq_seq, sq_len, mss, tmpl, head_len8, *, rexmit=None, ip_id_base=0, ip_id_add=0,
             head_first_off, seg_cap, fill=FILL):
    """Every output array of rns_tx_tcp_plan_dev, as a dict of numpy arrays (KEYS): the stops and the cap
    rule as the header states them, the sends from ``Socket``.  Unwritten template bytes hold ``fill``."""
    flows = np.asarray(flows, dtype=FLOW).reshape(-1)
    nfl = flows.size
    E = 2 * nfl
    tmpl = np.asarray(tmpl, dtype=np.uint8).reshape(max(nfl, 1), -1)[:nfl]
    stride = tmpl.shape[1]
    p = {"tmpl": np.full((E, stride), fill, dtype=np.uint8), "head_len8": np.zeros(E, dtype=np.uint8),
         "pay_off": np.zeros(E, dtype=np.uint64), "pay_len": np.zeros(E, dtype=np.uint32), "mss": np.zeros(E, dtype=np.uint16),
         "head_off": np.zeros(E, dtype=np.uint64), "seg_first": np.zeros(E + 1, dtype=np.uint32),
         "blk_flow": np.full((seg_cap + 63) // 64, E, dtype=np.uint32), "n": np.zeros(2, dtype=np.uint32),
         "res": np.zeros(nfl, dtype=RES), "flows_out": flows.copy()}
    next_packet_id = (int(ip_id_base) + int(ip_id_add)) & 0xFFFF
    n_seg = n_v4 = 0
    head_at = int(head_first_off)
    dropped = False
    for f in range(nfl):
        rec, ms, hl, ql = flows[f], int(mss[f]), int(head_len8[f]), int(sq_len[f])
        p["head_len8"][2 * f:2 * f + 2], p["mss"][2 * f:2 * f + 2] = hl, ms
        inflight = (int(rec["snd_nxt"]) - int(rec["snd_una"])) & M32
        a = (int(rec["snd_una"]) - int(sq_seq[f])) & M32
        why, sends = PLAN_NONE, [[], []]
        if int(rec["state"]) != ESTABLISHED:
            why = PLAN_STATE
        elif ms == 0 or ql > DOMAIN or int(rec["snd_wnd"]) > DOMAIN or inflight > DOMAIN or a > ql or a + inflight > ql:
            why = PLAN_BAD
        elif not template_ok(tmpl[f], hl, stride):
            why = PLAN_TMPL
        else:
            timer = Socket(rec, ms, inflight)             # the timer thread first, then the writer
            if rexmit is not None and rexmit[f]:
                timer.retransmit()
            sends[0] = timer.sent
            writer = Socket(rec, ms, inflight)
            _, waited = writer.tcp_write(ql - a - inflight)
            sends[1] = writer.sent
            why = PLAN_WINDOW if waited else PLAN_NONE
        for k in (0, 1):
            e = 2 * f + k
            p["seg_first"][e], p["head_off"][e] = n_seg, head_at
            s = sends[k]
            if not s:
                continue
            if dropped or n_seg + len(s) > seg_cap:
                dropped = True
                if k == 1:
                    why = PLAN_CAP
                continue
            seq_num, ack_num, flags, window, offset, _ = s[0]
            nbytes = sum(x[5] for x in s)
            # one entry stands for its pieces: consecutive slices, the same ack, window and flags, seq + j * mss
            assert all(x[4] == offset + j * ms and x[0] == (seq_num + (0 if k == 0 else j * ms)) & M32 and
                       x[1:4] == (ack_num, flags, window) and x[5] == min(ms, nbytes - j * ms) for j, x in enumerate(s))
            p["pay_off"][e] = int(sq_off[f]) + a + offset
            p["pay_len"][e] = nbytes
            p["tmpl"][e, :hl] = row_ref(tmpl[f], hl, seq_num, ack_num, flags, window, next_packet_id)
            p["blk_flow"][(n_seg + 63) // 64:(n_seg + len(s) + 63) // 64] = e
            n_seg += len(s)
            head_at += len(s) * hl
            if hl == 40:                                  # NEXT_PACKET_ID.fetch_add(1) per datagram, ip_output_v4 only
                next_packet_id = (next_packet_id + len(s)) & 0xFFFF
                n_v4 += len(s)
            if k == 0:
                p["res"][f]["rexmit_bytes"] = nbytes
            else:
                p["res"][f]["new_bytes"], p["res"][f]["new_segs"] = nbytes, len(s)
                p["flows_out"][f]["snd_nxt"] = (int(rec["snd_nxt"]) + nbytes) & M32
        p["res"][f]["why"] = why
    p["seg_first"][E] = n_seg
    p["n"][:] = (n_seg, n_v4)
    return p


def same_plan(got, want):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k in ("res", "flows_out"):
            g, w = g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)
        if w.size == 0:                                   # no flows: the rows' width means nothing
            assert g.size == 0, k
            continue
        assert g.shape == w.shape, k
        assert np.array_equal(g.astype(w.dtype), w), (k, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:8])


def chains_of(p):
    """The [head, data slice] chains a plan's descriptors expand to, in segment order."""
    frags = []
    for e in range(p["pay_len"].size):
        pl, ms, hl = int(p["pay_len"][e]), int(p["mss"][e]), int(p["head_len8"][e])
        for j in range(-(-pl // ms) if pl else 0):
            ln = min(ms, pl - j * ms)
            frags.append((e, j, int(p["head_off"][e]) + j * hl, hl, int(p["pay_off"][e]) + j * ms, ln))
    return frags


def heads_ref(p, arena):
    """(arena with every planned datagram's head finished, status per segment): the heads built from the
    plan's template rows as rns_tx_segment_dev's header states, finished by oracle.tx_chain_fill_ref."""
    a = np.asarray(arena, dtype=np.uint8).copy()
    st = []
    for e, j, ho, hl, po, ln in chains_of(p):
        h = head(p["tmpl"][e, :hl].tobytes(), j, int(p["mss"][e]), ln)
        done, s = O.tx_chain_fill_ref([h, arena[po:po + ln].tobytes()])
        a[ho:ho + hl] = np.frombuffer(done, dtype=np.uint8)
        st.append(s)
    return a, np.array(st, dtype=np.uint8)


def tmpl4(k=0, junk=0x5A):
    from rx_flow_helper import template
    return template(bytes([10, 0, 0, 2]), bytes([10, 0, 1 + (k >> 8) & 0xFF, k & 0xFF]), 0xC000 + (k & 0xFFF), 80, junk)


def tmpl6(k=0, junk=0x5A):
    from rx_flow_helper import template
    src = bytes.fromhex("fd000000000000000000000000000002")
    return template(src, bytes.fromhex("fd0000000000000000000000") + k.to_bytes(4, "big"), 0xC000 + (k & 0xFFF), 80, junk)


def rows(tmpls, stride=64, junk=0xC3):
    """Template heads into n x stride rows, the rest of a row junk."""
    t = np.full((max(len(tmpls), 1), stride), junk, dtype=np.uint8)
    for i, x in enumerate(tmpls):
        k = min(len(x), stride)
        t[i, :k] = np.frombuffer(x[:k], dtype=np.uint8)
    return t[:len(tmpls)]


# ---------------------------------------------------------------------------
# cases: the planner's arguments from per-flow specs
# ---------------------------------------------------------------------------
def mk(specs, *, stride=64, seg_cap=1 << 20, head_first_off=0x1000, ip_id_base=0, ip_id_add=0, use_rexmit=True):
    """The arguments of plan_ref / plan_host (a dict) for flows given as dicts: una, inflight, wnd,
    unsent, mss, a (acked bytes still at the buffer's front), v6, rexmit, state, rq_len, rcv_nxt, and the
    overrides sq_len, hl, tmpl.  The send buffers lie back to back from an odd offset, one byte apart."""
    n = len(specs)
    flows = np.zeros(n, dtype=FLOW)
    sq_off, sq_seq, sq_len = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    mss, hl8, rex = np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    tm, at = [], 101
    for i, s in enumerate(specs):
        d = dict(una=1000 + 77777 * i, inflight=0, wnd=0xFFFF, unsent=0, mss=1460, a=0, v6=False, rexmit=0, state=ESTABLISHED,
                 rq_len=0, rcv_nxt=0x01020304 + i, sq_len=None, hl=None, tmpl=None)
        d.update(s)
        una = d["una"] & M32
        flows[i]["snd_una"], flows[i]["snd_nxt"], flows[i]["snd_wnd"] = una, (una + d["inflight"]) & M32, d["wnd"]
        flows[i]["rcv_nxt"], flows[i]["rcv_max"], flows[i]["rq_len"], flows[i]["state"] = d["rcv_nxt"], d["rcv_nxt"], d["rq_len"], d["state"]
        flows[i]["snd_wl1"], flows[i]["snd_wl2"], flows[i]["delayed_acks"], flows[i]["ack_timer"] = 5 + i, 9 + i, i % 5, i & 1
        sq_seq[i] = (una - d["a"]) & M32
        sq_len[i] = d["a"] + d["inflight"] + d["unsent"] if d["sq_len"] is None else d["sq_len"]
        sq_off[i] = at
        at += min(int(sq_len[i]), 1 << 16) + 1
        mss[i], rex[i] = d["mss"], d["rexmit"]
        hl8[i] = (60 if d["v6"] else 40) if d["hl"] is None else d["hl"]
        tm.append(d["tmpl"] if d["tmpl"] is not None else (tmpl6(i) if d["v6"] else tmpl4(i)))
    return dict(flows=flows, sq_off=sq_off, sq_seq=sq_seq, sq_len=sq_len, mss=mss, tmpl=rows(tm, stride), head_len8=hl8,
                rexmit=rex if use_rexmit else None, ip_id_base=ip_id_base, ip_id_add=ip_id_add, head_first_off=head_first_off,
                seg_cap=seg_cap)


def ref_of(c, **kw):
    c = dict(c, **kw)
    return plan_ref(c.pop("flows"), c.pop("sq_off"), c.pop("sq_seq"), c.pop("sq_len"), c.pop("mss"), c.pop("tmpl"),
                    c.pop("head_len8"), **c)


def edge_specs():
    """The named edges: {name: specs}."""
    bad4 = bytearray(tmpl4(3))
    bad4[9] = 17
    doff6 = bytearray(tmpl4(4))
    doff6[32] = 0x60
    return {
        "window exactly full": [dict(inflight=1000, wnd=1000 + 2 * 1460, unsent=5000)],
        "one byte short of a piece": [dict(inflight=0, wnd=1459, unsent=5000), dict(inflight=300, wnd=300 + 2919, unsent=9000)],
        "tail fits, full piece would not": [dict(wnd=1460 + 700, unsent=1460 + 700), dict(wnd=700, unsent=700),
                                            dict(wnd=1460 + 699, unsent=1460 + 700)],
        "window zero": [dict(wnd=0, unsent=100), dict(wnd=0, inflight=50, unsent=100, rexmit=1)],
        "window shrunk": [dict(inflight=5000, wnd=3000, unsent=4000, rexmit=1)],
        "across 2^32": [dict(una=0xFFFFFF00, inflight=0x80, wnd=0x4000, unsent=0x3000, a=0x300, rexmit=1),
                        dict(una=0xFFFFFFF0, inflight=0x20, wnd=0x4000, unsent=0x3000, rexmit=1),
                        dict(una=0xFFFFF000, inflight=0, wnd=0xFFFF, unsent=0x2000)],
        "receive queue": [dict(unsent=10, rq_len=0), dict(unsent=10, rq_len=0xFFFF), dict(unsent=10, rq_len=0x10000),
                          dict(unsent=10, rq_len=0x12345)],
        "mss extremes": [dict(mss=1, wnd=7, unsent=9, inflight=2, rexmit=1), dict(mss=65495, wnd=DOMAIN, unsent=3 * 65495 + 1),
                         dict(mss=65495, v6=True, wnd=65495, unsent=65495)],
        "stops": [dict(state=0, unsent=100), dict(state=2, unsent=100, inflight=10, rexmit=1), dict(mss=0, unsent=100),
                  dict(hl=20, unsent=100), dict(hl=60, unsent=100), dict(v6=True, hl=40, unsent=100),
                  dict(tmpl=bytes(bad4), unsent=100), dict(tmpl=bytes(doff6), unsent=100, inflight=5, rexmit=1),
                  dict(unsent=100)],
        "domain bounds": [dict(mss=65495, wnd=70000, unsent=0, sq_len=DOMAIN), dict(mss=65495, wnd=70000, sq_len=DOMAIN + 1),
                          dict(mss=65495, wnd=DOMAIN, unsent=70000), dict(mss=65495, wnd=DOMAIN + 1, unsent=70000),
                          dict(mss=65495, inflight=DOMAIN, wnd=DOMAIN, unsent=0, rexmit=1),
                          dict(mss=65495, inflight=DOMAIN + 1, wnd=DOMAIN, sq_len=DOMAIN, rexmit=1),
                          dict(a=500, inflight=0, unsent=0), dict(a=501, sq_len=500), dict(a=100, inflight=400, unsent=0, rexmit=1),
                          dict(a=100, inflight=401, sq_len=500, rexmit=1), dict(una=5, a=0xFFFFFFF0, sq_len=500)],
    }


def mixed_specs(n, seed, short=False):
    """n seeded random flows: IPv4 and IPv6 mixed, runs of empty and stopped flows between busy ones."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = int(rng.integers(0, 10)) if not short else 3
        run = (i // 7) % 5 == 3                           # a run of seven quiet flows every 35
        d = dict(una=int(rng.integers(0, 1 << 32)), v6=bool(rng.integers(0, 2)), rq_len=int(rng.integers(0, 0x11000)),
                 a=int(rng.integers(0, 3000)), mss=int(rng.choice([536, 1220, 1460, 8960])))
        if run or kind == 0:
            d.update(unsent=0, inflight=0 if kind & 1 else 100, rexmit=0)
        elif run or kind == 1:
            d.update(state=int(rng.integers(2, 6)), unsent=500, inflight=20, rexmit=1)
        elif short:
            d.update(unsent=int(rng.integers(1, 400)), wnd=0xFFFF, mss=1460, a=0, rq_len=i & 0xFFFF)
        else:
            d.update(inflight=int(rng.integers(0, 20000)), wnd=int(rng.integers(0, 0x10000)),
                     unsent=int(rng.integers(0, 60000)), rexmit=int(rng.integers(0, 2)))
        out.append(d)
    return out
