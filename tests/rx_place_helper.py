"""TCP receive placement restated from the reference, and the builders the rx-place tests share.
Nothing here calls the code under test.

decode_ref restates tcp_input's decode (tcp.rs:549-574) over a datagram the receive path accepted
(rx_chain_helper.rx_verify_chain_ref over recv_packet's chains gives the status and the L4 sum),
expected() adds the lookup by PORT_MAP's key (tcp.rs:577-578) and the placement rule of
rns_checksum.h field by field, and RefReassembler is TCPReassembler (tcp.rs:476-521) over real
byte strings.  Where the Rust code would panic (header[0..20], header[20..header_length],
trim_head) the record is the undecoded one: parity is unpinned there.
"""
import numpy as np

from oracle import oracle as O
from rx_chain_helper import netbuffers, rx_verify_chain_ref
from test_rx_oracle import L4, L6, R4, R6  # noqa: F401  (the tests' local and remote addresses)

NO_FLOW = 0xFFFFFFFF
P_TCP, P_FLOW, P_DONE, P_OUTSIDE = 1, 2, 4, 8
FIN, SYN, RST, PSH, ACK = 1, 2, 4, 8, 16
SENTINEL = 0xA7

META = np.dtype([("flow", "<u4"), ("seq", "<u4"), ("ack", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                 ("window", "<u2"), ("pay_len", "<u2"), ("flags", "u1"), ("ip_hdr", "u1"), ("tcp_hdr", "u1"),
                 ("place", "u1")])


# ---------------------------------------------------------------------------
# datagram builders
# ---------------------------------------------------------------------------
def tcp(src, dst, sport, dport, seq, body=b"", ack=0x01020304, flags=ACK | PSH, window=0x2000, doff=5, hlen=None):
    """A TCP segment with a valid checksum: `doff` is the data-offset FIELD, `hlen` the bytes laid
    down before the body (default doff * 4, at least 20); option bytes are NOPs."""
    hlen = max(20, doff * 4) if hlen is None else hlen
    seg = bytearray(hlen) + bytearray(body)
    seg[0:2], seg[2:4] = sport.to_bytes(2, "big"), dport.to_bytes(2, "big")
    seg[4:8], seg[8:12] = (seq & 0xFFFFFFFF).to_bytes(4, "big"), (ack & 0xFFFFFFFF).to_bytes(4, "big")
    seg[12], seg[13] = (doff << 4) & 0xFF, flags
    seg[14:16] = window.to_bytes(2, "big")
    for k in range(20, hlen):
        seg[k] = 1
    ph = O.pseudo_header_py(src, dst, len(seg), 6)
    seg[16:18] = (O.ones_comp_py(ph, bytes(seg)) ^ 0xFFFF).to_bytes(2, "big")
    return bytes(seg)


def ip4(src, dst, proto, payload, ihl=5, frag=0):
    h = bytearray(ihl * 4)
    h[0] = 0x40 | ihl
    h[2:4] = (len(h) + len(payload)).to_bytes(2, "big")
    h[6:8] = frag.to_bytes(2, "big")
    h[8], h[9] = 64, proto
    h[12:16], h[16:20] = src, dst
    for k in range(20, len(h)):
        h[k] = 1
    h[10:12] = O.checksum_py(bytes(h)).to_bytes(2, "big")
    return bytes(h) + payload


def ip6(src, dst, proto, payload):
    h = bytearray(40)
    h[0] = 0x60
    h[4:6] = len(payload).to_bytes(2, "big")
    h[6], h[7] = proto, 64
    h[8:24], h[24:40] = src, dst
    return bytes(h) + payload


def segment(src, sport, dport, seq, body=b"", ihl=5, **kw):
    """A whole datagram to the local address of src's family: IPv4 (IHL `ihl`) or IPv6."""
    if len(src) == 4:
        return ip4(src, L4, 6, tcp(src, L4, sport, dport, seq, body, **kw), ihl=ihl)
    return ip6(src, L6, 6, tcp(src, L6, sport, dport, seq, body, **kw))


def udp4(src, body):
    return ip4(src, L4, 17, bytes(8) + body)


def icmp4(src, body):
    seg = bytearray([8, 0, 0, 0]) + bytearray(body)
    seg[2:4] = (O.ones_comp_py(0, bytes(seg)) ^ 0xFFFF).to_bytes(2, "big")
    return ip4(src, L4, 1, bytes(seg))


def body_bytes(tag, n):
    """n pseudo-random payload bytes (never the sentinel)."""
    b = O.splitmix64_bytes(0xB0D1 + tag, max(n, 1))[:n].copy()
    b[b == SENTINEL] = SENTINEL ^ 0xFF
    return b.tobytes()


# ---------------------------------------------------------------------------
# the pool form
# ---------------------------------------------------------------------------
def pool_index(len16, buf):
    """(blk_first uint32, first uint32 [n + 1], n_frags) of the pool form, in numpy."""
    nfr = -(-np.asarray(len16, dtype=np.int64) // buf)
    first = np.zeros(len(nfr) + 1, dtype=np.int64)
    np.cumsum(nfr, out=first[1:])
    return first[:-1:64].astype(np.uint32), first.astype(np.uint32), int(first[-1])


def lay_pool(pkts, buf, shuffled=False, seed=1, spare=3):
    """The datagrams in a pool of buf-byte buffers as recv_packet leaves them: (pool uint8, buf_idx
    uint32, blk_first uint32, len16 uint16); the buffers in order or a seeded permutation."""
    len16 = np.array([len(p) for p in pkts], dtype=np.uint16)
    blk_first, first, nf = pool_index(len16, buf)
    nbuf = nf + spare
    order = np.random.default_rng(seed).permutation(nbuf) if shuffled else np.arange(nbuf)
    idx = order[:nf].astype(np.uint32)
    pool = np.frombuffer(O.splitmix64_bytes(seed ^ 0x9001, nbuf * buf).tobytes(), dtype=np.uint8).copy()
    rows = pool.reshape(nbuf, buf)
    for i, p in enumerate(pkts):
        for j, f in enumerate(netbuffers(p, buf)):
            rows[idx[first[i] + j], :len(f)] = np.frombuffer(f, dtype=np.uint8)
    return pool, idx, blk_first, len16


# ---------------------------------------------------------------------------
# the reference, restated
# ---------------------------------------------------------------------------
def be16(b):
    return (b[0] << 8) | b[1]


def be32(b):
    return (b[0] << 24) | (b[1] << 16) | (b[2] << 8) | b[3]


def decode_ref(pkt, status):
    """tcp.rs:549-574 for a datagram ip_input accepted: (fields dict, source address, payload) or None."""
    if not status & O.RX_ACCEPT:
        return None
    v4 = pkt[0] >> 4 == 4
    ip_hdr = (pkt[0] & 0xF) * 4 if v4 else 40
    proto, src = (pkt[9], pkt[12:16]) if v4 else (pkt[6], pkt[8:24])
    if proto != 6:                                      # ip_input_common hands it to another handler
        return None
    packet = pkt[ip_hdr:]                               # trim_head(ip header)
    packet_length = len(packet)
    if packet_length < 20:                              # header[..] panics
        return None
    header = packet
    header_length = (header[12] >> 4) * 4
    if header_length < 20 or header_length > packet_length:   # header[20..header_length] / trim_head panic
        return None
    f = dict(sport=be16(header[0:2]), dport=be16(header[2:4]), seq=be32(header[4:8]), ack=be32(header[8:12]),
             window=be16(header[14:16]), flags=header[13], ip_hdr=ip_hdr, tcp_hdr=header_length,
             pay_len=packet_length - header_length)
    return f, bytes(src), packet[header_length:]


def key_of(src, sport, dport):
    return (bytes(src), int(sport), int(dport))


def expected(pkts, buf, keys, next_seq, win_off, win_len, stream0, status=None, ones_comp=None):
    """(status uint8, l4 uint16, meta META, stream uint8) the placement must give for the datagrams
    `pkts` in buf-byte buffers, the flows `keys` (list of key_of), their windows and the initial
    stream bytes.  `status`: per-datagram overrides (a datagram bent after it was laid out);
    `ones_comp`: the oracle's compute_ones_comp, for speed."""
    table = {k: f for f, k in enumerate(keys)}
    n = len(pkts)
    st, l4 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint16)
    meta = np.zeros(n, dtype=META)
    meta["flow"] = NO_FLOW
    stream = np.array(stream0, dtype=np.uint8, copy=True)
    for i, p in enumerate(pkts):
        if status is not None and status[i] is not None:
            st[i], l4[i] = status[i]
        else:
            st[i], l4[i] = rx_verify_chain_ref(netbuffers(p, buf), L4, L6, ones_comp=ones_comp)
        d = decode_ref(p, int(st[i]))
        if d is None:
            continue
        f, src, pay = d
        place = P_TCP
        flow = table.get(key_of(src, f["sport"], f["dport"]), NO_FLOW)
        if flow != NO_FLOW:
            place |= P_FLOW
            if len(pay) > 0 and not f["flags"] & (SYN | RST):
                d_ = (f["seq"] - int(next_seq[flow])) & 0xFFFFFFFF
                wl, wo = int(win_len[flow]), int(win_off[flow])
                if d_ < wl and len(pay) <= wl - d_ and wo + wl <= stream.size:
                    place |= P_DONE
                    stream[wo + d_:wo + d_ + len(pay)] = np.frombuffer(pay, dtype=np.uint8)
                else:
                    place |= P_OUTSIDE
        meta[i] = (flow, f["seq"], f["ack"], f["sport"], f["dport"], f["window"], f["pay_len"], f["flags"],
                   f["ip_hdr"], f["tcp_hdr"], place)
    return st, l4, meta, stream


def seq_gt(a, b):
    """util.rs:155-158."""
    diff = (a - b) & 0xFFFFFFFF
    return diff < 0x80000000 and diff != 0


class RefReassembler:
    """TCPReassembler (tcp.rs:476-521) over byte strings: add_packet returns the delivered bytes
    (the returned NetBuffer, appended buffers included) or None."""

    def __init__(self):
        self.next_sequence = 0
        self.out_of_order = []

    def set_next_expect(self, seq):
        self.next_sequence = seq & 0xFFFFFFFF

    def get_next_expect(self):
        return self.next_sequence

    def add_packet(self, packet, seq_num):
        if seq_num == self.next_sequence:
            self.next_sequence = (self.next_sequence + len(packet)) & 0xFFFFFFFF
            i = 0
            while i < len(self.out_of_order):
                if seq_gt(seq_num, self.out_of_order[i][0]):
                    self.out_of_order.pop(i)
                elif self.out_of_order[i][0] == self.next_sequence:
                    _, ooo = self.out_of_order.pop(i)
                    self.next_sequence = (self.next_sequence + len(ooo)) & 0xFFFFFFFF
                    packet = packet + ooo
                    i = 0
                else:
                    i += 1
            return packet
        self.out_of_order.append((seq_num, packet))
        return None
