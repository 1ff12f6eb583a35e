"""The reference's UDP receive path restated line by line over the NetBuffer model of icmp_echo_helper,
and the datagram and case builders the UDP demux tests share.  Nothing here calls the code under test.

ip_input_v4 / ip_input_v6 (as rx_chain_helper.rx_verify_chain_ref restates their checks) hand an accepted
protocol-17 datagram, trimmed to its L4 segment, to udp_input (udp.rs:126-148): header(), the two
big-endian ports, trim_head(8), PORT_MAP as a dict port -> deque, push_back of (source address, source
port, packet).  udp_recv (udp.rs:75-98) pops the front entry and copies min(len, cap) bytes.  Where the
Rust code would panic (header[2..4] / trim_head(8) on a segment shorter than 8 bytes) nothing is queued:
parity is unpinned there.
"""
from collections import deque

import numpy as np

from icmp_echo_helper import NetBuffer, Pool
from oracle import oracle as O
from rx_chain_helper import netbuffers, rx_verify_chain_ref
from rx_place_helper import icmp4, ip4, ip6, lay_pool, segment  # noqa: F401  (lay_pool: the receive pool form of a batch)
from test_rx_oracle import L4, L6, R4, R6  # noqa: F401  (the tests' local and remote addresses)

UDP_HEADER_LEN = 8
R4B, R6B = bytes([10, 9, 8, 7]), bytes(range(0x30, 0x40))  # a second sender of each family


class Stack:
    """The reference's PORT_MAP: udp_open's sockets, each a receive_queue."""

    def __init__(self, ports):
        self.port_map = {}
        for p in ports:
            self.udp_open(p)

    def udp_open(self, port):                           # udp.rs:61-71
        if port in self.port_map:
            raise ValueError("Port already in use")
        self.port_map[port] = deque()

    def udp_input(self, packet, source_addr):           # udp.rs:126-148
        header = packet.header()
        source_port = (int(header[0]) << 8) | int(header[1])
        dest_port = (int(header[2]) << 8) | int(header[3])
        packet.trim_head(UDP_HEADER_LEN)
        queue = self.port_map.get(dest_port)
        if queue is None:
            return                                      # "No socket listening on port"
        queue.append((bytes(source_addr), source_port, packet))

    def udp_recv(self, port, cap):                      # udp.rs:75-98 (a queue with an entry: it never waits here)
        source_addr, source_port, buf = self.port_map[port].popleft()
        copy_len = min(len(buf), cap)
        return source_addr, source_port, b"".join(buf.slices())[:copy_len]


def demux_ref(pkts, B, ports):
    """The batch through ip_input's dispatch and udp_input, each datagram a chain of B-byte NetBuffers:
    (status list as rx_verify_chain_ref gives it, the Stack with its queues filled)."""
    stack = Stack(ports)
    status = []
    for p in pkts:
        frags = netbuffers(p, B) if len(p) else []
        st, _ = rx_verify_chain_ref(frags, L4, L6)
        status.append(st)
        if not st & O.RX_ACCEPT:
            continue
        v6 = (p[0] >> 4) == 6
        h = 40 if v6 else (p[0] & 0xF) * 4
        if (p[6] if v6 else p[9]) != 17 or len(p) - h < UDP_HEADER_LEN:
            continue
        # the received chain in a pool of its own, trimmed to the L4 segment (ip.rs:92 / 119)
        mem = np.zeros(len(frags) * B, dtype=np.uint8)
        nb = NetBuffer(Pool(mem, [], B))
        for j, f in enumerate(frags):
            mem[j * B:j * B + len(f)] = np.frombuffer(f, dtype=np.uint8)
            nb.frags.append([j, 0, len(f)])
        nb.trim_head(h)
        stack.udp_input(nb, p[8:24] if v6 else p[12:16])
    return status, stack


def queues_ref(stack, ports, cap=1 << 16):
    """What repeated udp_recv calls return, socket by socket: a list per port of (address, port, payload)."""
    out = []
    for p in ports:
        q = []
        while stack.port_map[p]:
            q.append(stack.udp_recv(p, cap))
        out.append(q)
    return out


# ---------------------------------------------------------------------------
# datagram builders
# ---------------------------------------------------------------------------
def body(tag, n):
    return O.splitmix64_bytes(0x0DB0 + tag, max(n, 1))[:n].tobytes()


def udp_seg(sport, dport, pay, ulen=None, cksum=0):
    """A UDP segment; the length field defaults to the right one, the checksum to 0 (neither is read)."""
    ulen = 8 + len(pay) if ulen is None else ulen
    return sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + (ulen & 0xFFFF).to_bytes(2, "big") + \
        cksum.to_bytes(2, "big") + pay


def udp4(sport, dport, pay, src=R4, ihl=5, **kw):
    return ip4(src, L4, 17, udp_seg(sport, dport, pay, **kw), ihl=ihl)


def udp6(sport, dport, pay, src=R6, **kw):
    return ip6(src, L6, 17, udp_seg(sport, dport, pay, **kw))


def any_udp(k, dport, n):
    """Datagram k of a generated batch: the family, the IPv4 header length, the sender and the source port
    all vary with k; n payload bytes."""
    r = k % 5
    if r in (1, 3):
        return udp6(1000 + k % 50000, dport, body(k, n), src=R6B if k & 4 else R6)
    return udp4(1000 + k % 50000, dport, body(k, n), src=R4B if k & 4 else R4, ihl=(5, 5, 7, 5, 15)[r])


# ---------------------------------------------------------------------------
# the cases the CPU and the GPU tests share: name -> (datagrams, the sockets' ports)
# ---------------------------------------------------------------------------
TILE = 512  # the demux's datagrams per workgroup (rns_k_args.hpp kUdpTile)
COUNTS = (63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1)
SCAN_N = 64 * TILE + 1  # with 1024 sockets: 65 tiles, 66560 counts, 260 parts for the scan's middle kernel


def _ports(n, first=5000, step=7):
    return [first + step * s for s in range(n)]


def count_case(n):
    """n datagrams to two interleaved sockets and an unbound port, payloads 0..40."""
    ports = [53, 5353]
    return [any_udp(k, (53, 5353, 53, 9, 5353)[k % 5], (k * 11) % 41) for k in range(n)], ports


def cases(B):
    c = {}
    c["one"] = ([any_udp(k, 4000, (k * 29) % 90) for k in range(TILE + 90)], [4000])
    c["two"] = count_case(300)
    p64 = _ports(64)
    order = np.random.default_rng(64).permutation(64)
    c["wave64"] = ([any_udp(k, p64[order[k % 64]] if k < 128 else p64[k % 3], 20 + k % 30) for k in range(140)], p64)
    # 1024 sockets: the first, the last and 400..449 stay empty, 900..999 are first hit in the third tile
    p1k = _ports(1024, 2000, 3)
    early = [s for s in range(1024) if s not in (0, 1023) and not 400 <= s < 450 and not 900 <= s < 1000]
    rng = np.random.default_rng(1024)
    pk = []
    for k in range(2 * TILE + 300):
        pool = early if k < 2 * TILE else list(range(900, 1000)) + early[:50]
        pk.append(any_udp(k, p1k[pool[int(rng.integers(len(pool)))]], int(rng.integers(0, 70))))
    c["socks1024"] = (pk, p1k)
    lens = [0, 1, 15, 16, 17]
    c["lengths"] = ([f(7, 700 + (k & 1), body(n, n)) for k, n in enumerate(lens * 2)
                     for f in (udp4, udp6, lambda *a: udp4(*a, ihl=15))], [700, 701])
    edges = []
    for hdr, f in ((28, udp4), (48, udp6), (68, lambda *a: udp4(*a, ihl=15))):
        for d in (-1, 0, 1):
            for nb in (1, 2):  # the payload ends at the first buffer's end, and at the second's
                n = nb * B - hdr + d
                edges.append(f(9, 800 + len(edges) % 2, body(n + hdr, n)))
    c["edges"] = (edges, [800, 801])
    c["big"] = ([udp4(1, 900, body(1, 65535 - 28)), udp6(2, 901, body(2, 65535 - 48), src=R6B), udp4(3, 900, body(3, 5), src=R4B),
                 udp4(4, 901, body(4, 65535 - 68), ihl=15)], [900, 901])
    # what is not queued, interleaved with what is
    bad_ip = bytearray(udp4(5, 600, body(40, 30)))
    bad_ip[10] ^= 0x40
    no = [segment(R4, 1234, 600, 1000, body(41, 100)), segment(R6, 1234, 600, 1000, body(42, 33)), icmp4(R4, body(43, 20)),
          bytes(bad_ip), ip4(R4, L4, 17, udp_seg(5, 600, body(44, 30)), frag=0x2000), ip4(R4, L4, 17, udp_seg(5, 600, body(45, 30)), frag=0x0010),
          udp4(5, 601, body(46, 30)), udp6(5, 599, body(47, 30)), bytes([0x55]) + udp4(5, 600, body(48, 30))[1:]]
    no += [ip4(R4, L4, 17, udp_seg(5, 600, b"")[:k]) for k in range(8)] + [ip6(R6, L6, 17, udp_seg(5, 600, b"")[:k]) for k in range(8)]
    mixed = [udp4(6, 600, body(50, 10))]
    for k, p in enumerate(no):
        mixed += [p, any_udp(k, (600, 602)[k & 1], 10 + 37 * k)]
    c["mixed"] = (mixed, [600, 602])
    # a wrong length field and a checksum that does not verify are delivered anyway
    c["unread"] = ([udp4(7, 600, body(60, 50), ulen=9), udp6(7, 600, body(61, 50), ulen=4000, cksum=0xBEEF),
                    udp4(7, 600, body(62, 3), ulen=0, cksum=1)], [600])
    return c


_CACHE = {}


def case(name, B):
    """(datagrams, ports, the reference's statuses, the reference's queues per socket) — computed once."""
    key = (name, B)
    if key not in _CACHE:
        if name.startswith("count"):
            pkts, ports = count_case(int(name[5:]))
        elif name == "scan":
            p1k = _ports(1024, 2000, 3)
            kinds = [[any_udp(k, p1k[s], k % 19) for k in range(8)] for s in range(1024)]
            pkts, ports = [kinds[(i * 389) % 1024][i % 8] for i in range(SCAN_N)], p1k
        else:
            if ("cases", B) not in _CACHE:
                _CACHE[("cases", B)] = cases(B)
            pkts, ports = _CACHE[("cases", B)][name]
        st, stack = demux_ref(pkts, B, ports)
        _CACHE[key] = (pkts, ports, st, queues_ref(stack, ports))
    return _CACHE[key]


CASE_NAMES = ["one", "two", "wave64", "socks1024", "lengths", "edges", "big", "mixed", "unread"] + [f"count{n}" for n in COUNTS]
