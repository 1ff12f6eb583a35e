"""tcp_input's Established path and the ACKs it sends, restated from the reference, and the builders
the rx-flow tests share.  Nothing here calls the code under test.

Socket restates TCPSocketState as far as tcp.rs:402-447 (send_packet) and tcp.rs:642-740 (tcp_input
after the RST hack, state == Established) use it, over RefReassembler (tcp.rs:476-521, from
rx_place_helper) with real byte strings; send_packet records (ack, window) instead of calling
tcp_output.  update_ref puts the flow update's rules on top: which datagrams are a flow's, the stops,
the records.  ack_heads_ref is tcp_output (tcp.rs:938-976) and ip_output (ip.rs:140-177) for a pure
ACK over a template head, finalized by the transmit oracle (oracle.tx_fill_ref).
"""
import numpy as np

from oracle import oracle as O
from rx_place_helper import ACK, FIN, META, P_DONE, P_FLOW, P_OUTSIDE, P_TCP, PSH, RST, SYN, RefReassembler, seq_gt  # noqa: F401

FLOW = np.dtype([("rcv_nxt", "<u4"), ("rcv_max", "<u4"), ("snd_una", "<u4"), ("snd_nxt", "<u4"), ("snd_wnd", "<u4"),
                 ("snd_wl1", "<u4"), ("snd_wl2", "<u4"), ("rq_len", "<u4"), ("n_pend", "<u4"), ("delayed_acks", "<u2"),
                 ("state", "u1"), ("ack_timer", "u1")])
SEG = np.dtype([("ack_num", "<u4"), ("window", "<u2"), ("act", "u1"), ("pad", "u1")])
RES = np.dtype([("n_segs", "<u4"), ("consumed", "<u4"), ("stop", "<u4"), ("readable", "<u4"), ("acked", "<u4"),
                ("n_acks", "<u2"), ("events", "u1"), ("why", "u1")])
ESTABLISHED, MAX_SEGS = 1, 1024
S_CONSUMED, S_ACK, S_TIMER = 1, 2, 4
EV_WND = 1
STOP_NONE, STOP_MANY, STOP_STATE, STOP_FLAGS, STOP_OPTIONS, STOP_OUTSIDE, STOP_PEND = range(7)
NONE = 0xFFFFFFFF
MAX_DELAYED_ACKS = 5
MAX_RECEIVE_WINDOW = 0xFFFF
M32 = 0xFFFFFFFF


def seq_lt(a, b):
    return seq_gt(b, a)


def seq_le(a, b):
    return not seq_gt(a, b)


def wrapping_max(a, b):
    """util.rs:172-178."""
    return a if seq_gt(a, b) else b


class Socket:
    """TCPSocketState, Established.  receive_queue is a length (what it held before the batch) plus the
    bytes this batch appended; the out-of-order Vec's payloads are real byte strings."""

    def __init__(self, rec, pend=()):
        self.reassembler = RefReassembler()
        self.reassembler.set_next_expect(int(rec["rcv_nxt"]))
        self.reassembler.out_of_order = [(int(s), bytes(int(n))) for s, n in pend]
        self.receive_next_seq = int(rec["rcv_max"])
        self.send_unacked, self.send_next_seq = int(rec["snd_una"]), int(rec["snd_nxt"])
        self.send_window = int(rec["snd_wnd"])
        self.send_last_win_seq, self.send_last_win_ack = int(rec["snd_wl1"]), int(rec["snd_wl2"])
        self.receive_queue_len = int(rec["rq_len"])
        self.num_delayed_acks = int(rec["delayed_acks"])
        self.delayed_ack_timer_id = 7 if int(rec["ack_timer"]) else -1
        self.state = int(rec["state"])
        self.appended = b""          # receive_queue.append_buffer, this batch
        self.trimmed = 0             # retransmit_queue.trim_head, this batch
        self.sent = []               # send_packet: (ack_seq, receive_window)
        self.window_updates = 0

    def send_packet(self):
        """tcp.rs:402-447 with FLAG_ACK and an empty packet; the FIN + 1 is for other states."""
        receive_window = (MAX_RECEIVE_WINDOW - (self.receive_queue_len & 0xFFFF)) & 0xFFFF
        self.sent.append((self.reassembler.get_next_expect(), receive_window))

    def tcp_input(self, seq_num, ack_num, remote_window_size, flags, packet):
        """tcp.rs:642-740.  Returns "ack", "timer" or None: what the delayed-ACK branch did."""
        did = None
        if len(packet) != 0:
            self.receive_next_seq = wrapping_max(self.receive_next_seq, (seq_num + len(packet)) & M32)
            got = self.reassembler.add_packet(packet, seq_num)
            if got is not None:
                self.appended += got
                self.receive_queue_len = (self.receive_queue_len + len(got)) & M32
            self.num_delayed_acks = (self.num_delayed_acks + 1) & 0xFFFF
            if self.num_delayed_acks >= MAX_DELAYED_ACKS or flags & FIN:
                self.num_delayed_acks = 0
                self.delayed_ack_timer_id = -1
                self.send_packet()
                did = "ack"
            elif self.delayed_ack_timer_id == -1:
                self.delayed_ack_timer_id = 7
                did = "timer"
        if flags & ACK:
            if seq_lt(self.send_unacked, ack_num) and seq_le(ack_num, self.send_next_seq):
                self.trimmed += (ack_num - self.send_unacked) & M32
                self.send_unacked = ack_num
            if (seq_le(self.send_unacked, ack_num) and seq_le(ack_num, self.send_next_seq)
                    and (seq_lt(self.send_last_win_seq, seq_num)
                         or (self.send_last_win_seq == seq_num and seq_le(self.send_last_win_ack, ack_num)))):
                self.send_window = remote_window_size
                self.send_last_win_seq, self.send_last_win_ack = seq_num, ack_num
                self.window_updates += 1
        return did

    def record(self, rec):
        """The socket as a FLOW record (state as it was)."""
        out = np.zeros((), dtype=FLOW)
        out["rcv_nxt"], out["rcv_max"] = self.reassembler.get_next_expect(), self.receive_next_seq
        out["snd_una"], out["snd_nxt"], out["snd_wnd"] = self.send_unacked, self.send_next_seq, self.send_window
        out["snd_wl1"], out["snd_wl2"] = self.send_last_win_seq, self.send_last_win_ack
        out["rq_len"], out["n_pend"] = self.receive_queue_len, len(self.reassembler.out_of_order)
        out["delayed_acks"], out["state"] = self.num_delayed_acks, rec["state"]
        out["ack_timer"] = 0 if self.delayed_ack_timer_id == -1 else 1
        return out


def update_ref(meta, flows, pend, pend_cap, payload=None):
    """What the flow update must give: (flows_out FLOW, pend lists (one list of (seq, len) per flow),
    seg SEG, res RES, sockets).  `payload(i)`: datagram i's payload bytes (default: zeros)."""
    meta, flows = np.asarray(meta).reshape(-1), np.asarray(flows).reshape(-1)
    n, nfl = meta.size, flows.size
    pend = np.zeros((nfl, 0, 2), dtype=np.uint32) if pend is None else np.asarray(pend, dtype=np.uint32).reshape(nfl, -1, 2)
    out, seg, res = flows.copy(), np.zeros(n, dtype=SEG), np.zeros(nfl, dtype=RES)
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
        elif mine and (rec["state"] != ESTABLISHED or rec["n_pend"] > pend_cap):
            why = STOP_STATE
        if why or not mine:                              # untouched: the out record is the in record
            if why:
                res[f]["stop"], res[f]["why"] = mine[0], why
            pends.append(keep)
            socks.append(None)
            continue
        sk = Socket(rec, keep)
        for i in mine:
            m = meta[i]
            if m["flags"] & (SYN | RST | FIN):
                why = STOP_FLAGS
            elif m["tcp_hdr"] != 20:
                why = STOP_OPTIONS
            elif m["place"] & P_OUTSIDE:
                why = STOP_OUTSIDE
            elif m["pay_len"] > 0 and m["seq"] != sk.reassembler.get_next_expect() and \
                    len(sk.reassembler.out_of_order) == pend_cap:
                why = STOP_PEND
            if why:
                res[f]["stop"], res[f]["why"] = i, why
                break
            body = bytes(int(m["pay_len"])) if payload is None else payload(i)
            assert len(body) == m["pay_len"]
            did = sk.tcp_input(int(m["seq"]), int(m["ack"]), int(m["window"]), int(m["flags"]), body)
            seg[i]["act"] = S_CONSUMED | (S_ACK if did == "ack" else S_TIMER if did == "timer" else 0)
            if did == "ack":
                seg[i]["ack_num"], seg[i]["window"] = sk.sent[-1]
            res[f]["consumed"] += 1
        out[f] = sk.record(rec)
        res[f]["readable"], res[f]["acked"] = len(sk.appended), sk.trimmed & M32
        res[f]["n_acks"], res[f]["events"] = len(sk.sent), EV_WND if sk.window_updates else 0
        pends.append([(s, len(b)) for s, b in sk.reassembler.out_of_order])
        socks.append(sk)
    return out, pends, seg, res, socks


def same_update(got, want, pend_cap):
    """got = (flows FLOW, pend uint32 [n_flows, pend_cap, 2] or None, seg SEG, res RES) against update_ref's."""
    g_flows, g_pend, g_seg, g_res = got
    w_flows, w_pends, w_seg, w_res = want[:4]
    for g, w, what in ((g_flows, w_flows, "flow"), (g_seg, w_seg, "seg"), (g_res, w_res, "res")):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.shape == w.shape, what
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, [(int(i), g[i], w[i]) for i in bad[:5]])
    for f, want_list in enumerate(w_pends):
        if want_list and w_flows[f]["n_pend"] <= pend_cap:
            have = np.asarray(g_pend).reshape(len(w_pends), pend_cap, 2)[f, :len(want_list)]
            assert [tuple(int(x) for x in e) for e in have] == want_list, ("pend", f)


def metas(rows):
    """META records from dicts; defaults: a pure ACK of a flow's, 20-byte headers."""
    m = np.zeros(len(rows), dtype=META)
    for i, r in enumerate(rows):
        d = dict(flow=0, seq=0, ack=0, sport=1000, dport=80, window=0x2000, pay_len=0, flags=ACK, ip_hdr=20, tcp_hdr=20,
                 place=None)
        d.update(r)
        if d["place"] is None:
            d["place"] = P_TCP | P_FLOW | (P_DONE if d["pay_len"] and not d["flags"] & (SYN | RST) else 0)
        m[i] = tuple(d[k] for k in META.names)
    return m


def flow_rec(**kw):
    d = dict(rcv_nxt=0, rcv_max=0, snd_una=0, snd_nxt=0, snd_wnd=0, snd_wl1=0, snd_wl2=0, rq_len=0, n_pend=0,
             delayed_acks=0, state=ESTABLISHED, ack_timer=0)
    d.update(kw)
    r = np.zeros(1, dtype=FLOW)
    r[0] = tuple(d[k] for k in FLOW.names)
    return r[0]


# ---------------------------------------------------------------------------
# the ACKs
# ---------------------------------------------------------------------------
def template(src, dst, sport, dport, junk=0x5A):
    """A flow's template head: addresses, ports, TTL and protocol as ip_output / tcp_output set them,
    every field the build overwrites filled with junk."""
    t = bytearray([junk]) * 20
    t[0:2], t[2:4] = sport.to_bytes(2, "big"), dport.to_bytes(2, "big")
    t[12] = 0x50 | (junk & 0xF)
    t[18:20] = b"\x00\x00"                               # urgent pointer
    if len(src) == 4:
        h = bytearray(20)
        h[0], h[8], h[9] = 0x45, 64, 6
        h[2:6] = bytes([junk]) * 4
        h[10:12] = bytes([junk]) * 2
        h[12:16], h[16:20] = src, dst
    else:
        h = bytearray(40)
        h[0], h[6], h[7] = 0x60, 6, 64
        h[4:6] = bytes([junk]) * 2
        h[8:24], h[24:40] = src, dst
    return bytes(h + t)


def template_ok(t, hl, stride):
    if hl not in (40, 60) or hl > stride:
        return False
    if hl == 40:
        return t[0] == 0x45 and t[9] == 6 and t[32] >> 4 == 5
    return t[0] >> 4 == 6 and t[6] == 6 and t[52] >> 4 == 5


def ack_heads_ref(meta, seg, flows, tmpls, head_len, ip_id_base, stride=64):
    """[(datagram index, head bytes or None for a malformed template)] in batch order, and the IPv4 count:
    send_packet -> tcp_output -> ip_output over the flow's template, NEXT_PACKET_ID starting at ip_id_base."""
    out, next_packet_id = [], ip_id_base
    for i in range(len(meta)):
        f = int(meta[i]["flow"])
        if not seg[i]["act"] & S_ACK or f >= len(flows):
            continue
        hl, t = int(head_len[f]), tmpls[f]
        v4 = hl == 40
        pid = next_packet_id
        if v4:
            next_packet_id = (next_packet_id + 1) & 0xFFFF   # fetch_add in ip_output_v4 only
        if not template_ok(t, hl, stride):
            out.append((i, None))
            continue
        h = bytearray(t[:hl])
        ip = 20 if v4 else 40
        h[ip + 4:ip + 8] = int(flows[f]["snd_nxt"]).to_bytes(4, "big")       # tcp.rs:947
        h[ip + 8:ip + 12] = int(seg[i]["ack_num"]).to_bytes(4, "big")
        h[ip + 12], h[ip + 13] = 0x50, ACK
        h[ip + 14:ip + 16] = int(seg[i]["window"]).to_bytes(2, "big")
        h[ip + 16:ip + 18] = b"\x00\x00"
        if v4:
            h[2:4], h[4:6], h[10:12] = (40).to_bytes(2, "big"), pid.to_bytes(2, "big"), b"\x00\x00"
        else:
            h[4:6] = (20).to_bytes(2, "big")
        done, st = O.tx_fill_ref(bytes(h))
        assert st == (O.TX_IP_FILLED if v4 else 0) | O.TX_L4_FILLED
        out.append((i, done))
    return out, (next_packet_id - ip_id_base) & 0xFFFF
