"""The TCP listen responder restated from the reference, and the cases the listen tests share.  Nothing here
calls the code under test.

listen_ref restates tcp_input's lookup branch (tcp.rs:576-615), handle_new_connection (tcp.rs:894-936),
parse_options (tcp.rs:856-892), send_packet (tcp.rs:402-447), tcp_output (tcp.rs:938-976) and ip_output
(ip.rs:133-177) over the datagrams of a batch in arrival order: PORT_MAP is a dict that grows as SYNs arrive,
NEXT_PACKET_ID a counter, the ISS is taken from a list.  Where the Rust code would panic or loop for ever
in parse_options the new connection is the host's (RNS_CONN_HOST) and still owns its key.  The reference
parses every segment's options before the lookup; as rns_checksum.h says, only a new connection's are walked.
"""
from typing import NamedTuple

import numpy as np

from oracle import oracle as O
from rx_chain_helper import netbuffers, rx_verify_chain_ref
from rx_place_helper import ACK, FIN, L4, L6, PSH, R4, R6, RST, SYN, decode_ref, icmp4, ip4, ip6, key_of, udp4

C_UNMATCHED, C_SYN, C_LATER, C_RST, C_BUILT, C_NOBUF, C_HOST = 1, 2, 4, 8, 16, 32, 64
SYN_RECEIVED = 2
SENTINEL = 0xA7
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------
# datagram builders
# ---------------------------------------------------------------------------
def seg(src, sport, dport, seq, flags, opts=b"", body=b"", ack=0x01020304, window=0x2000, ihl=5):
    """A whole TCP datagram from ``src`` to the local address of its family, its option bytes ``opts`` (a
    multiple of 4), both checksums valid."""
    assert len(opts) % 4 == 0 and len(opts) <= 40
    dst = L4 if len(src) == 4 else L6
    t = bytearray(20) + bytearray(opts) + bytearray(body)
    t[0:2], t[2:4] = sport.to_bytes(2, "big"), dport.to_bytes(2, "big")
    t[4:8], t[8:12] = (seq & M32).to_bytes(4, "big"), (ack & M32).to_bytes(4, "big")
    t[12], t[13] = (5 + len(opts) // 4) << 4, flags
    t[14:16] = window.to_bytes(2, "big")
    ph = O.pseudo_header_py(src, dst, len(t), 6)
    t[16:18] = (O.ones_comp_py(ph, bytes(t)) ^ 0xFFFF).to_bytes(2, "big")
    return ip4(src, dst, 6, bytes(t), ihl=ihl) if len(src) == 4 else ip6(src, dst, 6, bytes(t))


def v4(k):
    return bytes([10, 1, (k >> 8) & 0xFF, k & 0xFF])


def v6(k):
    return bytes(R6[:12]) + int(k).to_bytes(4, "big")


MSS = bytes([2, 4, 0x05, 0xB4])  # MSS 1460


# ---------------------------------------------------------------------------
# the reference, restated
# ---------------------------------------------------------------------------
class Panic(Exception):
    """Where the Rust code panics or never returns."""


def parse_options_ref(header):
    """tcp.rs:856-892 over header[20..header_length]: max_segment_size."""
    mss, off = 0, 0
    while off < len(header):
        t = header[off]
        if t == 0:
            break
        if t == 1:
            off += 1
            continue
        if off + 1 >= len(header):
            raise Panic("header[opt_offset + 1]")
        ln = header[off + 1]
        if t == 2:
            if off + 4 > len(header):
                raise Panic("header[opt_offset + 2..opt_offset + 4]")
            mss = (header[off + 2] << 8) | header[off + 3]
        if ln == 0:
            raise Panic("opt_offset += 0 for ever")
        off += ln
    return mss


def tcp_output_ref(state, dest_ip, source_port, dest_port, seq_num, ack_num, flags, window, options):
    """tcp_output -> ip_output over an empty NetBuffer: the datagram's bytes.  ``state['next_id']`` is NEXT_PACKET_ID."""
    local = L4 if len(dest_ip) == 4 else L6
    hl = 20 + len(options)
    h = bytearray(hl)
    h[0:2], h[2:4] = source_port.to_bytes(2, "big"), dest_port.to_bytes(2, "big")
    h[4:8], h[8:12] = (seq_num & M32).to_bytes(4, "big"), (ack_num & M32).to_bytes(4, "big")
    h[12], h[13] = ((hl // 4) << 4) & 0xFF, flags
    h[14:16] = window.to_bytes(2, "big")
    h[20:] = options
    ph = O.pseudo_header_py(local, dest_ip, hl, 6)
    h[16:18] = (O.ones_comp_py(ph, bytes(h)) ^ 0xFFFF).to_bytes(2, "big")
    if len(dest_ip) == 16:                                   # ip_output_v6 (ip.rs:163-177)
        ip = bytearray(40)
        ip[0] = 0x60
        ip[4:6] = hl.to_bytes(2, "big")
        ip[6], ip[7] = 6, 64
        ip[8:24], ip[24:40] = local, dest_ip
        return bytes(ip) + bytes(h)
    ip = bytearray(20)                                       # ip_output_v4 (ip.rs:140-161)
    ip[0] = 0x45
    ip[2:4] = (20 + hl).to_bytes(2, "big")
    ip[4:6] = (state["next_id"] & 0xFFFF).to_bytes(2, "big")
    state["next_id"] += 1
    ip[8], ip[9] = 64, 6
    ip[12:16], ip[16:20] = local, dest_ip
    ip[10:12] = O.checksum_py(bytes(ip)).to_bytes(2, "big")
    return bytes(ip) + bytes(h)


class Ref(NamedTuple):
    conn: list      # per datagram: the RNS_CONN_* class bits, without BUILT / NOBUF
    replies: list   # (datagram index, bytes, is IPv4) in the order sent
    accepts: list   # dicts: key, src, listener, mss and the new socket's fields


def listen_ref(pkts, buf, keys, listen_ports, iss, ip_id=0):
    """The batch through tcp_input's lookup branch.  ``keys``: PORT_MAP's established sockets (key_of tuples);
    ``listen_ports``: the listen sockets' ports, listener l = listen_ports[l]; ``iss``: the new sockets' initial
    sequence numbers in the order they are drawn; ``ip_id``: NEXT_PACKET_ID before the batch."""
    port_map = {k: ("flow", f) for f, k in enumerate(keys)}
    listeners = {int(p): l for l, p in enumerate(listen_ports)}
    state = {"next_id": int(ip_id)}
    iss = list(iss)
    conn, replies, accepts = [], [], []
    for i, p in enumerate(pkts):
        st, _ = rx_verify_chain_ref(netbuffers(p, buf), L4, L6)
        d = decode_ref(p, int(st))
        if d is None:
            conn.append(0)
            continue
        f, src, _pay = d
        key = key_of(src, f["sport"], f["dport"])
        if key in port_map:                                  # tcp.rs:578
            conn.append(0 if port_map[key][0] == "flow" else C_UNMATCHED | C_LATER)
            continue
        listener = listeners.get(f["dport"])
        if listener is None or not f["flags"] & SYN:         # tcp.rs:582-595
            replies.append((i, tcp_output_ref(state, src, f["dport"], f["sport"], 1, f["seq"] + 1, RST | ACK, 0, b""),
                            len(src) == 4))
            conn.append(C_UNMATCHED | C_RST)
            continue
        header = p[f["ip_hdr"]:f["ip_hdr"] + f["tcp_hdr"]]
        try:
            mss = parse_options_ref(header[20:])
        except Panic:
            port_map[key] = ("host", i)
            conn.append(C_UNMATCHED | C_HOST)
            continue
        # handle_new_connection (tcp.rs:894-936)
        sock = dict(state=SYN_RECEIVED, send_mss=mss, receive_next_seq=(f["seq"] + 1) & M32,
                    next_expect=(f["seq"] + 1) & M32, send_next_seq=int(iss.pop(0)) & M32)
        replies.append((i, tcp_output_ref(state, src, f["dport"], f["sport"], sock["send_next_seq"], sock["next_expect"],
                                          SYN | ACK, 0xFFFF, bytes([2, 4, 0x5, 0xDC])), len(src) == 4))
        sock.update(send_unacked=f["seq"], send_last_win_ack=f["ack"], send_last_win_seq=f["seq"], send_window=f["window"])
        accepts.append(dict(key=key, src=i, listener=listener, mss=mss, **sock))
        port_map[key] = ("new", i)                           # tcp.rs:611
        conn.append(C_UNMATCHED | C_SYN)
    return Ref(conn, replies, accepts)


ACCEPT = np.dtype([("ip", "u1", (16,)), ("sport", "<u2"), ("dport", "<u2"), ("family", "u1"), ("pad", "u1", (3,)),
                   ("rcv_nxt", "<u4"), ("rcv_max", "<u4"), ("snd_una", "<u4"), ("snd_nxt", "<u4"), ("snd_wnd", "<u4"),
                   ("snd_wl1", "<u4"), ("snd_wl2", "<u4"), ("rq_len", "<u4"), ("n_pend", "<u4"), ("delayed_acks", "<u2"),
                   ("state", "u1"), ("ack_timer", "u1"), ("src", "<u4"), ("listener", "<u2"), ("mss", "<u2")])
assert ACCEPT.itemsize == 72


def expected(ref, n, cap):
    """What the entry must leave for ``ref`` under ``reply_cap`` = cap, every output array pre-filled with SENTINEL:
    (conn uint8 [n], out uint8 [64 * cap], rep_src uint32 [cap], rep_len8 uint8 [cap], accept ACCEPT [cap], count)."""
    conn = np.array(ref.conn, dtype=np.uint8).reshape(n)
    out = np.full(64 * cap, SENTINEL, np.uint8)
    rep_src = np.frombuffer(bytes([SENTINEL]) * (4 * cap), dtype=np.uint32).copy()
    rep_len8 = np.full(cap, SENTINEL, np.uint8)
    accept = np.frombuffer(bytes([SENTINEL]) * (72 * cap), dtype=ACCEPT).copy()
    by_src = {a["src"]: (k, a) for k, a in enumerate(ref.accepts)}
    for k, (i, head, _) in enumerate(ref.replies):
        if k >= cap:
            conn[i] |= C_NOBUF
            continue
        conn[i] |= C_BUILT
        out[64 * k:64 * k + len(head)] = np.frombuffer(head, dtype=np.uint8)
        rep_src[k], rep_len8[k] = i, len(head)
        if i in by_src:
            a, s = by_src[i]
            ip, sport, dport = s["key"]
            r = np.zeros(1, ACCEPT)[0]
            r["ip"][:len(ip)] = np.frombuffer(ip, dtype=np.uint8)
            r["sport"], r["dport"], r["family"] = sport, dport, 4 if len(ip) == 4 else 6
            r["rcv_nxt"], r["rcv_max"] = s["next_expect"], s["receive_next_seq"]
            r["snd_una"], r["snd_nxt"], r["snd_wnd"] = s["send_unacked"], s["send_next_seq"], s["send_window"]
            r["snd_wl1"], r["snd_wl2"], r["state"] = s["send_last_win_seq"], s["send_last_win_ack"], s["state"]
            r["src"], r["listener"], r["mss"] = i, s["listener"], s["send_mss"]
            accept[a] = r
    count = np.array([len(ref.replies), sum(1 for r in ref.replies if r[2]), len(ref.accepts)], dtype=np.uint32)
    return conn, out, rep_src, rep_len8, accept, count


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
class Case(NamedTuple):
    pkts: list
    keys: list          # the established flows' keys
    ports: list         # the listening ports
    buf: int = 128
    ip_id: int = 0
    ip_id_add: int = 0


FLOW_KEYS = [key_of(R4, 40000 + k, 80) for k in range(3)] + [key_of(R6, 41000, 443)]


def filler(k):
    """A datagram that is no unmatched segment: a known flow's, UDP, ICMP."""
    kind = k % 4
    if kind == 0:
        return seg(R4, 40000 + k % 3, 80, 1000 + k, ACK | PSH, body=bytes([k & 0xFF]) * (1 + k % 50))
    if kind == 1:
        return udp4(R4, bytes(k % 40))
    if kind == 2:
        return icmp4(R4, bytes(8 + k % 30))
    return seg(R6, 41000, 443, 5000 + k, ACK)


def order_case():
    """One key as stray, SYN, duplicate SYN, third ACK; the same with the two SYNs on either side of a 64-datagram
    block and of a 256-datagram scan block; several keys interleaved."""
    a, b, c = v4(1), v4(2), v6(3)
    pkts = [seg(a, 5000, 80, 100, ACK), seg(a, 5000, 80, 200, SYN, MSS), seg(a, 5000, 80, 200, SYN, MSS),
            seg(a, 5000, 80, 201, ACK, ack=777)]
    pkts += [filler(k) for k in range(len(pkts), 600)]
    pkts[62] = seg(b, 5001, 80, 10, ACK | PSH, body=b"early")          # before its key's SYN: RST
    pkts[63] = seg(b, 5001, 80, 300, SYN, MSS)
    pkts[64] = seg(b, 5001, 80, 300, SYN, MSS)                          # the next 64-datagram block: LATER
    pkts[65] = seg(b, 5001, 80, 301, ACK)
    pkts[255] = seg(c, 5002, 443, 400, SYN)
    pkts[256] = seg(c, 5002, 443, 400, SYN | ACK)                       # the next scan block: LATER
    pkts[300] = seg(c, 5002, 443, 401, RST)                             # the new socket's: LATER
    pkts[257] = seg(c, 5003, 443, 1, SYN)                               # another key (its port): a connection of its own
    for j in range(20):                                                 # several keys interleaved, their SYN in the middle
        for r, fl in enumerate((ACK, SYN, SYN, ACK | FIN)):
            pkts[400 + 20 * r + j] = seg(v4(100 + j), 6000 + j, 80 if j % 2 else 443, 50 + r, fl)
    return Case(pkts, FLOW_KEYS, [80, 443])


def options_case():
    opts = {
        "none": b"", "mss": MSS, "nops": bytes([1, 1, 1, 1]) + MSS, "two": MSS + bytes([2, 4, 0x02, 0x18]),
        "eol": bytes([0, 0, 0, 0]) + MSS, "odd length": bytes([2, 7, 0x01, 0x00, 1, 1, 1, 1]),
        "other": bytes([3, 3, 7, 1]) + bytes([8, 10] + [9] * 8) + bytes([1, 1]) + MSS,
        "past the end": bytes([1, 1, 8, 10]),                            # returns: the walk ends past the options
        "zero length": bytes([3, 0, 0, 0]), "length byte past the end": bytes([1, 1, 1, 3]),
        "truncated mss": bytes([1, 1, 2, 4]), "full": bytes([1] * 36) + MSS,  # tcp_hdr 60
        "mss zero length": bytes([2, 0, 0x05, 0xB4]),
    }
    pkts = []
    for j, (_, o) in enumerate(opts.items()):
        src = v4(j) if j % 2 == 0 else v6(j)
        pkts += [seg(src, 7000 + j, 8080, 0x7FFFFFF0 + j, SYN, o, ihl=5 + (j % 3 if len(src) == 4 and len(o) <= 32 else 0)),
                 seg(src, 7000 + j, 8080, 0x7FFFFFF1 + j, ACK)]         # its third segment: LATER, HOST shapes included
    return Case(pkts, [], [8080]), list(opts)


def family_case():
    """IPv4 and IPv6 mixed, SYNs and strays, the ids across the 0xffff wrap."""
    pkts = []
    for j in range(150):
        src = v6(j) if j % 4 == 1 else v4(j)
        fl =(SYN, ACK, RST, SYN | FIN, FIN | ACK, SYN | RST)[j % 6]
        pkts.append(seg(src, 9000 + j, (22, 23, 25)[j % 3], 0xFFFFFF00 + j, fl, MSS if j % 2 else b"",
                        body=bytes(j % 7) if j % 4 == 0 else b"", window=j))
    return Case(pkts, [], [22, 25], buf=256, ip_id=0xFFD0, ip_id_add=0x20010)


def unanswered_case():
    """Matched flows, UDP, ICMP, bad checksums and malformed datagrams: d_conn 0; among them a few strays."""
    pkts = [filler(k) for k in range(90)]
    bad = bytearray(seg(v4(7), 1234, 80, 5, SYN))
    bad[-1] ^= 0x40                                                     # the TCP checksum fails
    pkts[10] = bytes(bad)
    bad = bytearray(seg(v4(8), 1234, 80, 5, SYN))
    bad[10] ^= 0x01                                                     # the IP header checksum fails
    pkts[11] = bytes(bad)
    pkts[12] = bytes([0x50]) + bytes(39)                                # version 5
    pkts[13] = ip4(v4(9), L4, 6, bytes(12))                             # shorter than a TCP header
    short = bytearray(seg(v4(10), 1234, 80, 5, SYN))
    short[20 + 12] = 0x40                                               # data offset 4
    pkts[14] = bytes(short)
    pkts[15] = ip4(v4(11), L4, 6, seg(v4(11), 1, 80, 5, SYN)[20:], frag=0x2000)  # a fragment
    pkts[20] = seg(v4(12), 1234, 81, 5, SYN)                            # nobody listens on 81: RST
    pkts[21] = seg(v4(13), 1234, 80, 9, ACK)
    return Case(pkts, FLOW_KEYS, [80, 443])


def many_keys_case(n=2000):
    """About 2000 distinct keys, SYNs from distinct sources with a stray and a duplicate now and then."""
    pkts = []
    for j in range(n):
        src = v6(j) if j % 5 == 0 else v4(j)
        pkts.append(seg(src, 1024 + j % 50, 80, 3 * j, SYN if j % 7 else ACK, MSS if j % 2 else b""))
        if j % 11 == 0:
            pkts.append(pkts[-1])
    return Case(pkts, [], [80])


def key_dwords(src, sport, dport):
    ip = bytes(src) + bytes(16 - len(src))
    return [int.from_bytes(ip[4 * k:4 * k + 4], "little") for k in range(4)] + [sport | (dport << 16), 4 if len(src) == 4 else 6]


def colliding_case(key_hash, slots_of, n=300, want=40):
    """Keys that share the low bits of the table's hash for the slot count in use, found by search with the
    Python twin of the hash (``key_hash``; ``slots_of(n)`` = the table's slots for n datagrams): one long probe
    run.  Each key sends a SYN, and some a second SYN and a stray before it."""
    mask = slots_of(n) - 1
    found, j = [], 0
    while len(found) < want:
        src, sport = (v4(j) if j % 4 else v6(j)), 2000 + j % 30000
        if key_hash(key_dwords(src, sport, 80)) & mask == 5:
            found.append((src, sport))
        j += 1
    pkts = [seg(s, p, 80, 11, ACK) for s, p in found[::3]] + [seg(s, p, 80, 20 + k, SYN, MSS) for k, (s, p) in enumerate(found)] + \
        [seg(s, p, 80, 20 + k, SYN, MSS) for k, (s, p) in enumerate(found[::2])]
    pkts += [filler(k) for k in range(n - len(pkts))]
    assert len(pkts) == n
    return Case(pkts, FLOW_KEYS, [80])


def iss_of(n):
    """The ISS list of a case: any numbers do, the host supplies them."""
    return [(0x9E3779B1 * (k + 1)) & M32 for k in range(n)]
