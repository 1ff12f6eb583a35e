"""tcp_input for an existing socket (tcp.rs:622-835), send_packet (tcp.rs:402-447), tcp_close
(tcp.rs:195-224) and the control segments' head bytes, restated from the reference's text, and the
builders the connection tests share.  Nothing here calls the code under test.

ConnSocket extends rx_flow_helper.Socket (TCPSocketState over RefReassembler with real byte strings) by
the state machine; send_packet records (seq, ack, window, flags) instead of calling tcp_output.
conn_ref puts the connection update's rules on top: which datagrams are a flow's, the stops, the
records.  close_ref is tcp_close over a batch, ctl_heads_ref tcp_output (tcp.rs:938-976) and ip_output
(ip.rs:140-177) over a template head, finalized by the transmit oracle (oracle.tx_fill_ref).
"""
import numpy as np

from oracle import oracle as O
from rx_flow_helper import (ACK, FIN, FLOW, M32, META, MAX_DELAYED_ACKS, MAX_RECEIVE_WINDOW, MAX_SEGS, NONE, P_FLOW, P_OUTSIDE, PSH,  # noqa: F401
                            RES, RST, SYN, Socket, flow_rec, metas, seq_le, seq_lt, template, template_ok, wrapping_max)

CTL = np.dtype([("flow", "<u4"), ("seq", "<u4"), ("ack_num", "<u4"), ("window", "<u2"), ("flags", "u1"), ("act", "u1")])
# TCPState as rns_tcp_flow.state numbers it
CLOSED, ESTABLISHED, SYN_RECEIVED, CLOSE_WAIT, LAST_ACK, FIN_WAIT1, FIN_WAIT2, CLOSING, TIME_WAIT, SYN_SENT, LISTEN = range(11)
STATE_NAMES = ("Closed", "Established", "SynReceived", "CloseWait", "LastAck", "FinWait1", "FinWait2", "Closing", "TimeWait",
               "SynSent", "Listen")
C_CONSUMED, C_SEND, C_ACK_TIMER, C_RESP_TIMER, C_TIMEWAIT, C_RESET, C_STATE = 1, 2, 4, 8, 16, 32, 64
EV_WND, EV_STATE = 1, 2
STOP_NONE, STOP_MANY, STOP_STATE, STOP_FLAGS, STOP_OPTIONS, STOP_OUTSIDE, STOP_PEND, STOP_TWICE = range(8)


class ConnSocket(Socket):
    """TCPSocketState in any state.  sent: (send_next_seq, ack_seq, receive_window, flags) per send_packet;
    timers: what the call set, as C_* bits."""

    def __init__(self, rec, pend=()):
        super().__init__(rec, pend)
        self.set_states = 0
        self.transitions = []        # (old state, new state) per set_state

    def send_packet(self, flags=ACK):
        """tcp.rs:402-447 with an empty packet."""
        receive_window = (MAX_RECEIVE_WINDOW - (self.receive_queue_len & 0xFFFF)) & 0xFFFF          # tcp.rs:403
        plus = self.state in (FIN_WAIT1, FIN_WAIT2, CLOSING, CLOSE_WAIT) and \
            self.receive_next_seq == self.reassembler.get_next_expect()                              # tcp.rs:408-417
        ack_seq = (self.reassembler.get_next_expect() + (1 if plus else 0)) & M32
        self.sent.append((self.send_next_seq, ack_seq, receive_window, flags))

    def set_state(self, new_state):
        """tcp.rs:449-456."""
        self.transitions.append((self.state, new_state))
        self.state = new_state
        self.set_states += 1

    def is_established(self):
        """tcp.rs:458-463."""
        return self.state not in (CLOSED, SYN_SENT, TIME_WAIT)

    def tcp_input(self, seq_num, ack_num, remote_window_size, flags, packet):
        """tcp.rs:627-835 for a segment without options.  Returns the C_* bits of what it did beyond
        consuming the segment (C_SEND is read off `sent` by the caller)."""
        did = 0
        if flags & RST:                                                           # tcp.rs:635-640
            self.set_state(CLOSED)
            return C_RESET
        if len(packet) != 0:                                                      # tcp.rs:642
            self.receive_next_seq = wrapping_max(self.receive_next_seq, (seq_num + len(packet)) & M32)
            got = self.reassembler.add_packet(packet, seq_num)
            if got is not None:
                self.appended += got
                self.receive_queue_len = (self.receive_queue_len + len(got)) & M32
            if self.state == ESTABLISHED:                                         # tcp.rs:654
                self.num_delayed_acks = (self.num_delayed_acks + 1) & 0xFFFF
                if self.num_delayed_acks >= MAX_DELAYED_ACKS or flags & FIN:      # tcp.rs:656
                    self.num_delayed_acks = 0
                    self.delayed_ack_timer_id = -1
                    self.send_packet(ACK)
                elif self.delayed_ack_timer_id == -1:                             # tcp.rs:668
                    self.delayed_ack_timer_id = 7
                    did |= C_ACK_TIMER
            else:                                                                 # tcp.rs:688-695
                self.delayed_ack_timer_id = -1
                self.send_packet(ACK)
        if flags & ACK and self.is_established():                                 # tcp.rs:698
            if seq_lt(self.send_unacked, ack_num) and seq_le(ack_num, self.send_next_seq):
                self.trimmed += (ack_num - self.send_unacked) & M32
                self.send_unacked = ack_num
            if (seq_le(self.send_unacked, ack_num) and seq_le(ack_num, self.send_next_seq)
                    and (seq_lt(self.send_last_win_seq, seq_num)
                         or (self.send_last_win_seq == seq_num and seq_le(self.send_last_win_ack, ack_num)))):
                self.send_window = remote_window_size
                self.send_last_win_seq, self.send_last_win_ack = seq_num, ack_num
                self.window_updates += 1
        st = self.state                                                           # tcp.rs:742
        if st == SYN_RECEIVED:                                                    # tcp.rs:766-774
            if flags & ACK:
                self.set_state(ESTABLISHED)
                self.send_next_seq = (self.send_next_seq + 1) & M32
                self.send_unacked = ack_num
        elif st == ESTABLISHED:                                                   # tcp.rs:776-783
            if flags & FIN:
                self.set_state(CLOSE_WAIT)
        elif st == LAST_ACK:                                                      # tcp.rs:785-789
            if flags & ACK:
                self.set_state(CLOSED)
        elif st == FIN_WAIT1:                                                     # tcp.rs:791-808
            if flags & ACK and flags & FIN and ack_num == (self.send_next_seq + 1) & M32:
                self.set_state(TIME_WAIT)
                did |= C_TIMEWAIT
            elif flags & FIN:
                self.set_state(CLOSING)
                self.send_packet(ACK)
                did |= C_RESP_TIMER
            elif flags & ACK and ack_num == (self.send_next_seq + 1) & M32:
                self.set_state(FIN_WAIT2)
        elif st == FIN_WAIT2:                                                     # tcp.rs:810-820
            if flags & FIN:
                self.send_packet(ACK)
                did |= C_RESP_TIMER
                self.set_state(TIME_WAIT)
                did |= C_TIMEWAIT
        elif st == CLOSING:                                                       # tcp.rs:822-830
            if flags & ACK:
                self.set_state(TIME_WAIT)
                did |= C_TIMEWAIT
        return did

    def tcp_close(self):
        """tcp.rs:195-224 for a connected socket (Listen's PORT_MAP removal is the host's).  True: it sent."""
        if self.state == ESTABLISHED:                                             # tcp.rs:210-214
            self.send_packet(FIN | ACK)
            self.set_state(FIN_WAIT1)
            return True
        if self.state == CLOSE_WAIT:                                              # tcp.rs:216-220
            self.send_packet(FIN | ACK)
            self.set_state(LAST_ACK)
            return True
        return False

    def record(self, rec=None):
        out = super().record({"state": self.state})
        return out


def stop_of(sk, m, pend_cap):
    """The stop that holds before segment m for socket sk (the issue's table, in its order), after STOP_MANY and n_pend."""
    flags, pay = int(m["flags"]), int(m["pay_len"])
    if sk.state in (SYN_SENT, LISTEN) or sk.state > 10:
        return STOP_STATE
    if m["tcp_hdr"] != 20:
        return STOP_OPTIONS
    if flags & RST:
        return STOP_NONE
    if flags & SYN and pay > 0:
        return STOP_FLAGS
    if m["place"] & P_OUTSIDE:
        return STOP_OUTSIDE
    if pay > 0 and m["seq"] != sk.reassembler.get_next_expect() and len(sk.reassembler.out_of_order) >= pend_cap:
        return STOP_PEND
    if pay > 0 and flags & FIN:
        if sk.state == FIN_WAIT2:
            return STOP_TWICE
        if sk.state == FIN_WAIT1 and not (flags & ACK and m["ack"] == (sk.send_next_seq + 1) & M32):
            return STOP_TWICE
    return STOP_NONE


def conn_ref(meta, flows, pend, pend_cap, payload=None):
    """What the connection update must give: (flows_out FLOW, pend lists, ctl CTL, res RES, sockets)."""
    meta, flows = np.asarray(meta).reshape(-1), np.asarray(flows).reshape(-1)
    n, nfl = meta.size, flows.size
    pend = np.zeros((nfl, 0, 2), dtype=np.uint32) if pend is None else np.asarray(pend, dtype=np.uint32).reshape(nfl, -1, 2)
    out, ctl, res = flows.copy(), np.zeros(n, dtype=CTL), np.zeros(nfl, dtype=RES)
    res["stop"] = NONE
    lists = [[] for _ in range(nfl)]
    member = np.flatnonzero(((meta["place"] & P_FLOW) != 0) & (meta["flow"] < nfl))
    for i, f in zip(member.tolist(), meta["flow"][member].tolist()):   # batch order
        lists[f].append(i)
    pends, socks = [], []
    for f in range(nfl):
        mine, rec = lists[f], flows[f]
        keep = [(int(s), int(ln)) for s, ln in pend[f, :min(int(rec["n_pend"]), pend_cap)]]
        res[f]["n_segs"] = len(mine)
        why = STOP_NONE
        if mine and len(mine) > MAX_SEGS:
            why = STOP_MANY
        elif mine and rec["n_pend"] > pend_cap:
            why = STOP_STATE
        if why or not mine:                              # untouched: the out record is the in record
            if why:
                res[f]["stop"], res[f]["why"] = mine[0], why
            pends.append(keep)
            socks.append(None)
            continue
        sk = ConnSocket(rec, keep)
        for i in mine:
            m = meta[i]
            why = stop_of(sk, m, pend_cap)
            if why:
                res[f]["stop"], res[f]["why"] = i, why
                break
            body = bytes(int(m["pay_len"])) if payload is None else payload(i)
            assert len(body) == m["pay_len"]
            n_sent, n_set = len(sk.sent), sk.set_states
            did = sk.tcp_input(int(m["seq"]), int(m["ack"]), int(m["window"]), int(m["flags"]), body)
            assert len(sk.sent) - n_sent <= 1, "a record holds one send: STOP_TWICE must have caught this"
            act = C_CONSUMED | did | (C_STATE if sk.set_states > n_set else 0)
            if len(sk.sent) > n_sent:
                ctl[i] = (f,) + sk.sent[-1] + (act | C_SEND,)
            else:
                ctl[i] = (f, 0, 0, 0, 0, act)
            res[f]["consumed"] += 1
        out[f] = sk.record()
        res[f]["readable"], res[f]["acked"] = len(sk.appended), sk.trimmed & M32
        res[f]["n_acks"] = len(sk.sent)
        res[f]["events"] = (EV_WND if sk.window_updates else 0) | (EV_STATE if sk.set_states else 0)
        pends.append([(s, len(b)) for s, b in sk.reassembler.out_of_order])
        socks.append(sk)
    return out, pends, ctl, res, socks


def same_conn(got, want, pend_cap):
    """got = (flows FLOW, pend uint32 [n_flows, pend_cap, 2] or None, ctl CTL, res RES) against conn_ref's."""
    g_flows, g_pend, g_ctl, g_res = got
    w_flows, w_pends, w_ctl, w_res = want[:4]
    for g, w, what in ((g_flows, w_flows, "flow"), (g_ctl, w_ctl, "ctl"), (g_res, w_res, "res")):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.shape == w.shape, what
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, [(int(i), g[i], w[i]) for i in bad[:5]])
    for f, want_list in enumerate(w_pends):
        if want_list and w_flows[f]["n_pend"] <= pend_cap:
            have = np.asarray(g_pend).reshape(len(w_pends), pend_cap, 2)[f, :len(want_list)]
            assert [tuple(int(x) for x in e) for e in have] == want_list, ("pend", f)


def close_ref(flows, op):
    """tcp_close over a batch: (flows_out FLOW, ctl CTL)."""
    flows = np.asarray(flows).reshape(-1)
    out, ctl = flows.copy(), np.zeros(flows.size, dtype=CTL)
    for f, rec in enumerate(flows):
        if int(op[f]) != 1:
            continue
        sk = ConnSocket(rec)
        if sk.tcp_close():
            ctl[f] = (f,) + sk.sent[-1] + (C_SEND | C_RESP_TIMER | C_STATE,)
            out[f]["state"] = sk.state
            assert sk.record().tobytes() == out[f].tobytes()         # nothing else moved: snd_nxt is not advanced
    return out, ctl


def ctl_heads_ref(ctl, tmpls, head_len, ip_id_base, ip_id_add=0, stride=64):
    """[(record index, head bytes or None for a segment that is not built)] in record order, and the IPv4
    count: tcp_output -> ip_output over the flow's template, NEXT_PACKET_ID starting at ip_id_base + ip_id_add."""
    out, first = [], (ip_id_base + ip_id_add) & 0xFFFF
    next_packet_id = first
    for i in range(len(ctl)):
        f = int(ctl[i]["flow"])
        if not ctl[i]["act"] & C_SEND or f >= len(head_len):
            continue
        hl, t = int(head_len[f]), tmpls[f]
        v4 = hl == 40
        pid = next_packet_id
        if v4:
            next_packet_id = (next_packet_id + 1) & 0xFFFF   # fetch_add in ip_output_v4 only
        if not template_ok(t, hl, stride) or ctl[i]["flags"] & SYN:   # (a SYN needs options: not this form's)
            out.append((i, None))
            continue
        h = bytearray(t[:hl])
        ip = 20 if v4 else 40
        h[ip + 4:ip + 8] = int(ctl[i]["seq"]).to_bytes(4, "big")              # tcp.rs:947
        h[ip + 8:ip + 12] = int(ctl[i]["ack_num"]).to_bytes(4, "big")
        h[ip + 12], h[ip + 13] = 0x50, int(ctl[i]["flags"])
        h[ip + 14:ip + 16] = int(ctl[i]["window"]).to_bytes(2, "big")
        h[ip + 16:ip + 18] = b"\x00\x00"
        if v4:
            h[2:4], h[4:6], h[10:12] = (40).to_bytes(2, "big"), pid.to_bytes(2, "big"), b"\x00\x00"
        else:
            h[4:6] = (20).to_bytes(2, "big")
        done, st = O.tx_fill_ref(bytes(h))
        assert st == (O.TX_IP_FILLED if v4 else 0) | O.TX_L4_FILLED
        out.append((i, done))
    return out, (next_packet_id - first) & 0xFFFF


def same_heads(got, want, cap=None):
    """got = (out uint8 [cap * 64], src, len8, count) against ctl_heads_ref's (list, v4 count)."""
    g_out, g_src, g_len, g_cnt = got
    heads, v4s = want
    assert [int(x) for x in np.asarray(g_cnt).reshape(-1)[:2]] == [len(heads), v4s], ("count", g_cnt, len(heads), v4s)
    g_out = np.asarray(g_out).reshape(-1)
    for k, (i, h) in enumerate(heads[:len(heads) if cap is None else cap]):
        assert int(g_src[k]) == i, ("src", k)
        assert int(g_len[k]) == (len(h) if h is not None else 0), ("len8", k)
        if h is not None:
            assert g_out[64 * k:64 * k + len(h)].tobytes() == h, ("head", k, i)


# ---------------------------------------------------------------------------
# the shared cases
# ---------------------------------------------------------------------------
FLAG_SETS = (0, ACK, FIN, FIN | ACK, RST, RST | ACK, SYN, SYN | ACK, PSH | ACK)


def exhaustive_table():
    """One flow per combination, one segment each (the lane path): states 0..11 x the flag sets x pay_len {0, 7} x
    four ack numbers x two sequence numbers x rcv_max {rcv_nxt, rcv_nxt + 9}, plus tcp_hdr 24 and P_OUTSIDE rows.
    Returns (meta, flows): 12 * 9 * 2 * 4 * 2 * 2 + 2 * 12 * 9 = 3672 flows."""
    rows, flows = [], []
    rcv_nxt, snd_una, snd_nxt = 0xFFFFFFFA, 5000, 5100     # rcv_nxt + 7 wraps
    acks = (snd_nxt, snd_nxt + 1, snd_una, 0x70000000)

    def add(state, flags, pay, ack, seq, rmax, **kw):
        f = len(flows)
        flows.append(flow_rec(rcv_nxt=rcv_nxt, rcv_max=rmax, snd_una=snd_una, snd_nxt=snd_nxt, snd_wnd=300, snd_wl1=seq - 1,
                              snd_wl2=snd_una, rq_len=40 + f % 7, delayed_acks=f % 5, state=state, ack_timer=(f >> 2) & 1))
        rows.append(dict(flow=f, seq=seq & M32, ack=ack, pay_len=pay, flags=flags, window=0x1000 + f % 256, **kw))

    for state in range(12):
        for flags in FLAG_SETS:
            for pay in (0, 7):
                for ack in acks:
                    for seq in (rcv_nxt, rcv_nxt + 3):
                        for rmax in (rcv_nxt, (rcv_nxt + 9) & M32):
                            add(state, flags, pay, ack, seq, rmax)
            add(state, flags, 7, snd_nxt, rcv_nxt, rcv_nxt, tcp_hdr=24)
            add(state, flags, 7, snd_nxt, rcv_nxt, rcv_nxt, place=1 | P_FLOW | P_OUTSIDE)
    return metas(rows), np.array(flows, dtype=FLOW)


def list_lengths_case():
    """Flows of 1, 2, 63, 64, 65, 1024 and 1025 segments, interleaved; each flow's last segment is a FIN|ACK."""
    lens = (1, 2, 63, 64, 65, 1024, 1025)
    rng = np.random.default_rng(7)
    slots = np.repeat(np.arange(len(lens)), lens)
    rng.shuffle(slots)
    n = slots.size
    meta = np.zeros(n, dtype=META)
    meta["flow"], meta["seq"], meta["flags"], meta["tcp_hdr"], meta["ip_hdr"] = slots, 500, ACK, 20, 20
    meta["place"] = 1 | P_FLOW
    meta["ack"] = 1000 + np.arange(n)                                 # ascending in batch order: every one trims
    for f in range(len(lens)):
        meta["flags"][np.flatnonzero(slots == f)[-1]] = FIN | ACK
    flows = np.array([flow_rec(rcv_nxt=500, rcv_max=500, snd_una=900, snd_nxt=1000 + n, snd_wl1=499,
                               state=SYN_RECEIVED if f & 1 else ESTABLISHED) for f in range(len(lens))], dtype=FLOW)
    return meta, flows, lens, slots


def established_batch():
    """6 Established flows over 200 datagrams, interleaved by a seeded permutation, built with rx_flow_helper's
    builders and free of SYN / RST / FIN; every flow's result depends on the order of its segments: out-of-order
    arrivals, a duplicate seq with another length, a stale segment inside the window, and ACK numbers and windows
    that move with every segment.  Returns (meta, flows)."""
    rng = np.random.default_rng(61)
    per, flows = [], []
    for f in range(6):
        base = (0xFFFFF000 + 0x1000 * f * 7) & M32
        segs, off = [], 0
        for j in range(33):
            ln = int(rng.integers(10, 50))
            segs.append(dict(flow=f, seq=(base + off) & M32, pay_len=ln, ack=2000 + 7 * j, window=100 + j, flags=ACK | PSH))
            off += ln
        for j in (3, 9, 20):                                         # out of order: swapped neighbours
            segs[j], segs[j + 1] = segs[j + 1], segs[j]
        segs[14], segs[16] = segs[16], segs[14]                     # and two places apart
        segs.insert(12, dict(segs[11], pay_len=segs[11]["pay_len"] + 5))         # a duplicate seq, longer
        segs.insert(25, dict(segs[2], ack=1990))                    # stale, inside the window
        per.append(segs[:34 if f < 2 else 33])
        flows.append(flow_rec(rcv_nxt=base, rcv_max=base, snd_una=1995, snd_nxt=4000, snd_wl1=(base - 1) & M32,
                              delayed_acks=f % 5, ack_timer=f & 1, rq_len=100 * f))
    slots = np.repeat(np.arange(6), [len(p) for p in per])
    assert slots.size == 200
    rng.shuffle(slots)
    it = [iter(p) for p in per]
    return metas([next(it[f]) for f in slots]), np.array(flows, dtype=FLOW)


def order_case(meta=None, flows=None):
    """established_batch (6 interleaved flows, order-sensitive) turned into connection traffic: every other flow in
    CloseWait (every data segment answered at once), a FIN or a stray SYN on the way, an RST in flow 2."""
    if meta is None:
        meta, flows = established_batch()
    meta, flows = meta.copy(), flows.copy()
    flows["state"][1::2] = CLOSE_WAIT
    for f in range(6):
        mine = np.flatnonzero(meta["flow"] == f)
        meta["flags"][mine[20]] |= FIN if f < 4 else SYN
        meta["flags"][mine[28]] = RST if f == 2 else meta["flags"][mine[28]]
    cap = 8
    return meta, flows, np.zeros((6, cap, 2), dtype=np.uint32), cap


def stops_case():
    """Four flows of five data segments; the third is a FIN with payload in FinWait2 and in FinWait1 (STOP_TWICE), a
    SYN with payload (STOP_FLAGS), and in flow 3 a FIN that acknowledges ours: one send, no stop."""
    base = dict(rcv_nxt=100, rcv_max=100, snd_una=50, snd_nxt=60, snd_wl1=99)
    flows = np.array([flow_rec(state=FIN_WAIT2, **base), flow_rec(state=FIN_WAIT1, **base),
                      flow_rec(state=ESTABLISHED, **base), flow_rec(state=FIN_WAIT1, **base)], dtype=FLOW)
    rows = []
    for j in range(5):
        for f in range(4):
            d = dict(flow=f, seq=100 + 10 * j, ack=60, pay_len=10, flags=ACK | PSH)
            if j == 2:
                d["flags"] = (FIN | ACK, FIN | ACK, SYN | ACK, FIN | ACK)[f]
                d["ack"] = 61 if f == 3 else 60
            rows.append(d)
    return metas(rows), flows


def out_of_order_case():
    """Four flows in four states, 13 data segments each arriving out of order, a FIN and a trimming ACK on the way."""
    flows, rows = [], []
    for f, st in enumerate((SYN_RECEIVED, ESTABLISHED, FIN_WAIT1, CLOSE_WAIT)):
        flows.append(flow_rec(rcv_nxt=1000, rcv_max=1000, snd_una=7, snd_nxt=9, snd_wl1=999, state=st, delayed_acks=3))
        seqs = (1010, 1020, 1000, 1040, 1030, 1050, 1070, 1060, 1090, 1100, 1110, 1120, 1080)
        for j, s in enumerate(seqs):
            fl = ACK | PSH | (FIN if j == 5 and st != FIN_WAIT1 else 0)
            rows.append(dict(flow=f, seq=s, ack=10 if j == 3 else 9, pay_len=10, flags=fl))
    return metas(rows), np.array(flows, dtype=FLOW)


def fuzz_batch(seed, n_flows=64, max_segs=40):
    """Random states and segments, tuned so that (by conn_ref's own account) at least half of all segments are
    consumed and every arm of step D and every stop reason but STOP_MANY occurs over the seeds the tests use.
    Returns (meta, flows, pend, pend_cap)."""
    rng = np.random.default_rng(seed)
    cap = 3
    flows, per = [], []
    states = [ESTABLISHED] * 4 + [SYN_RECEIVED, SYN_RECEIVED, CLOSE_WAIT, LAST_ACK, FIN_WAIT1, FIN_WAIT1, FIN_WAIT1, FIN_WAIT2,
                                  FIN_WAIT2, CLOSING, TIME_WAIT, CLOSED]
    for f in range(n_flows):
        state = states[int(rng.integers(len(states)))] if rng.random() > 0.03 else int(rng.integers(9, 13))
        rcv = int(rng.integers(0, 2 ** 32))
        snd_una = int(rng.integers(0, 2 ** 32))
        snd_nxt = (snd_una + int(rng.integers(0, 200))) & M32
        n_pend = 4 if rng.random() < 0.02 else 0
        flows.append(flow_rec(rcv_nxt=rcv, rcv_max=rcv, snd_una=snd_una, snd_nxt=snd_nxt, snd_wnd=1000,
                              snd_wl1=(rcv - 1) & M32, snd_wl2=snd_una, rq_len=int(rng.integers(0, 3000)), n_pend=n_pend,
                              delayed_acks=int(rng.integers(0, 5)), state=state, ack_timer=int(rng.integers(0, 2))))
        segs, off = [], 0
        for j in range(int(rng.integers(1, max_segs + 1))):
            r = rng.random()
            pay = int(rng.integers(1, 30)) if rng.random() < 0.5 else 0
            flags = ACK | (PSH if pay else 0)
            kw = {}
            if r < 0.10:
                flags |= FIN
            elif r < 0.13:
                flags = FIN
            elif r < 0.15:
                flags = RST | (ACK if rng.random() < 0.5 else 0)
            elif r < 0.17:
                flags = SYN | (ACK if rng.random() < 0.5 else 0)
            elif r < 0.18:
                flags = 0
            elif r < 0.185:
                kw["tcp_hdr"] = 24
            elif r < 0.19 and pay:
                kw["place"] = 1 | P_FLOW | P_OUTSIDE
            seq = (rcv + off) & M32
            if pay and rng.random() < 0.15:
                seq = (seq + int(rng.integers(1, 40))) & M32        # out of order: pended, or STOP_PEND
            elif pay:
                off += pay
            ar = rng.random()
            ack = (snd_nxt + 1) & M32 if ar < 0.3 else snd_nxt if ar < 0.6 else (snd_una + int(rng.integers(0, 220))) & M32
            if flags & FIN and flags & ACK and rng.random() < 0.5:
                ack = (snd_nxt + 1) & M32                             # the ACK of our FIN with the peer's
            segs.append(dict(flow=f, seq=seq, ack=ack, pay_len=pay, flags=flags, window=int(rng.integers(0, 65536)), **kw))
        per.append(segs)
    slots = np.repeat(np.arange(n_flows), [len(p) for p in per])
    rng.shuffle(slots)
    it = [iter(p) for p in per]
    pend = np.zeros((n_flows, cap, 2), dtype=np.uint32)
    return metas([next(it[f]) for f in slots]), np.array(flows, dtype=FLOW), pend, cap


ARMS = {(SYN_RECEIVED, ESTABLISHED), (ESTABLISHED, CLOSE_WAIT), (LAST_ACK, CLOSED), (FIN_WAIT1, TIME_WAIT), (FIN_WAIT1, CLOSING),
        (FIN_WAIT1, FIN_WAIT2), (FIN_WAIT2, TIME_WAIT), (CLOSING, TIME_WAIT)}            # step D's, tcp.rs:742-835


def fuzz_wants(seeds=(1, 2, 3)):
    """conn_ref over the fuzz batches of `seeds`, and the conditions the generator is tuned to, asserted on the
    helper's output alone: at least half of all segments consumed, every arm of step D, every stop reason a flow
    of at most 40 segments can meet (STOP_MANY needs more than 1024: list_lengths_case has it)."""
    wants = {seed: conn_ref(*fuzz_batch(seed)) for seed in seeds}
    arms, whys, consumed, total = coverage(wants.values())
    assert 2 * consumed >= total and ARMS <= arms and whys >= {0, 2, 3, 4, 5, 6, 7}, (ARMS - arms, whys, consumed, total)
    return wants


def coverage(wants):
    """Over conn_ref results: (the set_state transitions seen, the stop reasons seen, consumed segments, all
    member segments) — the fuzz's conditions are asserted on these before the device is looked at."""
    arms, whys, consumed, total = set(), set(), 0, 0
    for _, _, ctl, res, socks in wants:
        whys |= set(int(w) for w in res["why"])
        consumed += int(res["consumed"].sum())
        total += int(res["n_segs"].sum())
        for sk in socks:
            if sk is not None:
                arms |= set(sk.transitions)
    return arms, whys, consumed, total


# ---------------------------------------------------------------------------
# the hand-traced lifecycles (tests/golden/tcp_conn_kats.json) through any implementation
# ---------------------------------------------------------------------------
def load_kats():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcp_conn_kats.json")) as fh:
        return json.load(fh)


def check_kat(kats, case, update, close, heads, grouped):
    """Drives one lifecycle through update(meta, flows, pend, cap) -> (flows, pend, ctl, res), close(flows, op) ->
    (flows, ctl) and heads(ctl, tmpls, head_len, ip_id_base) -> (out, src, len8, count), all numpy, as flow 1 of
    three.  grouped: consecutive segments go in as one multi-segment batch (only the run's last 'after' can be
    checked); otherwise one call per step, every 'after' checked."""
    tmpl, hl = bytes.fromhex(kats["template"]), kats["head_len"]
    flows = np.array([flow_rec(), flow_rec(**case["flow"]), flow_rec(state=LISTEN)], dtype=FLOW)
    want_fields = dict(case["flow"])
    pid = kats["ip_id_base"]
    steps, k = case["steps"], 0

    def check_ctl(rec, st):
        assert int(rec["act"]) == st["act"], (case["name"], st["cite"], int(rec["act"]))
        w = st["ctl"] or dict(seq=0, ack_num=0, window=0, flags=0)
        assert {n: int(rec[n]) for n in w} == w and int(rec["flow"]) == 1, (case["name"], st["cite"], rec)

    def check_heads(ctl, sts):
        nonlocal pid
        out, src, len8, count = heads(ctl, [tmpl] * 3, [hl] * 3, pid)
        sends = [s for s in sts if s["head"] is not None]
        assert int(count[0]) == int(count[1]) == len(sends)
        for j, s in enumerate(sends):
            assert s["ip_id"] == (pid + j) & 0xFFFF
            assert int(len8[j]) == hl and np.asarray(out).reshape(-1)[64 * j:64 * j + hl].tobytes().hex() == s["head"], \
                (case["name"], s["cite"])
        pid = (pid + len(sends)) & 0xFFFF

    while k < len(steps):
        if steps[k]["do"] == "close":
            flows, ctl = close(flows, np.array([0, 1, 0], dtype=np.uint8))
            run = [steps[k]]
            check_ctl(ctl[1], steps[k])
            assert not ctl[0]["act"] and not ctl[2]["act"]
        else:
            e = k + 1
            while grouped and e < len(steps) and steps[e]["do"] == "seg":
                e += 1
            run = steps[k:e]
            meta = metas([dict(flow=1, **s["seg"]) for s in run])
            flows, _, ctl, res = update(meta, flows, np.zeros((3, 2, 2), dtype=np.uint32), 2)
            assert int(res[1]["consumed"]) == len(run) and int(res[1]["why"]) == 0, (case["name"], res[1])
            for rec, s in zip(ctl, run):
                check_ctl(rec, s)
        check_heads(ctl, run)
        for s in run:
            want_fields.update(s["after"])
        got = {n: int(flows[1][n]) for n in want_fields}
        assert got == want_fields, (case["name"], run[-1]["cite"], got, want_fields)
        assert flows[0].tobytes() == flow_rec().tobytes() and flows[2].tobytes() == flow_rec(state=LISTEN).tobytes()
        k += len(run)


def ctl_cases():
    """Records from every source over IPv4 and IPv6 templates, good and malformed: (ctl CTL, tmpl uint8 [n_flows,
    64], head_len uint8).  Flows 0-1 IPv4, 2 IPv6, 3 IPv4 with a bad protocol, 4 a head length of 44, 5 IPv6 with
    TCP options in the template, 6 IPv4 again."""
    v4a, v4b, v6 = bytes([10, 1, 2, 3]), bytes([10, 9, 8, 7]), bytes.fromhex("20010db8000000000000000000000042")
    tm = [template(v4a, v4b, 80, 4000), template(v4b, v4a, 443, 5000, junk=0xA5), template(v6, v6[::-1], 80, 6000),
          template(v4a, v4b, 80, 4001), template(v4a, v4b, 80, 4002), template(v6, v6[::-1], 80, 6001),
          template(v4b, v4a, 8080, 7000, junk=0x11)]
    bad = bytearray(tm[3])
    bad[9] = 17
    tm[3] = bytes(bad)
    opt = bytearray(tm[5])
    opt[52] = 0x60
    tm[5] = bytes(opt)
    head_len = np.array([40, 40, 60, 40, 44, 60, 40], dtype=np.uint8)
    tmpl = np.zeros((7, 64), dtype=np.uint8)
    for f, t in enumerate(tm):
        tmpl[f, :len(t)] = np.frombuffer(t, dtype=np.uint8)
    rows = []
    rng = np.random.default_rng(5)
    for i in range(300):
        f = int(rng.integers(0, 9))                                   # 7 and 8: no flow of ours
        flags = (ACK, FIN | ACK, RST | ACK, RST, SYN | ACK, ACK)[int(rng.integers(0, 6))]
        act = int(rng.integers(0, 128))
        if i % 3 == 0:
            act |= C_SEND
        rows.append((f, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 65536)), flags, act))
    rows[7] = (0xFFFFFFFF, 1, 2, 3, ACK, C_SEND | C_CONSUMED)
    return np.array(rows, dtype=CTL), tmpl, head_len
