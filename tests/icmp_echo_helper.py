"""The reference's echo path restated line by line over a tiny NetBuffer model, and the request
builders the ICMP echo tests share.

A NetBuffer is a list of fragments ``[buffer index, start, end)`` over a pool of B-byte buffers
(buf.rs): trim_head (buf.rs:294-329), append_from_slice / append_from_buffer (buf.rs:385-447) and
alloc_header (buf.rs:262-291) are restated on it, then icmp_input_v4 / icmp_input_v6 ->
icmp_output_v4 / icmp_output_v6 (icmp.rs:44-120) -> ip_output_v4 / ip_output_v6 (ip.rs:141-182) with
NEXT_PACKET_ID as a counter.  Fresh buffers come from a free list in order (Pool), so a reply's chain
is comparable fragment by fragment with the pool transmit form.
The checksum primitives are the pinned oracle's (ones_comp_py, buffer_ones_comp_py, pseudo_header_py).
"""
import numpy as np

from oracle import oracle as O
from rx_chain_helper import netbuffers, rx_verify_chain_ref
from rx_place_helper import ip4, ip6, lay_pool  # noqa: F401  (lay_pool: the receive pool form of a batch)
from test_rx_oracle import L4, L6, R4, R6  # noqa: F401  (the tests' local and remote addresses)

ICMP_HEADER_LEN = 4
R4B, R6B = bytes([10, 9, 8, 7]), bytes(range(0x30, 0x40))  # a second requester of each family


class Pool:
    """FRAGMENT_POOL over a numpy pool of B-byte buffers and a free list taken in order.  The
    reference allocates a reply's payload buffers before its head buffer; the pool transmit form names
    the head buffer first, so `reserve` sets the reply's first free entry aside for the fragment that
    alloc_header prepends.  Nothing observable depends on which free buffer a fragment gets."""

    def __init__(self, mem, free, B):
        self.mem, self.free, self.B, self.taken, self.held = mem, [int(f) for f in free], B, 0, None

    def reserve(self):
        self.held = self.alloc()

    def alloc(self, head=False):
        if head and self.held is not None:
            k, self.held = self.held, None
            return k
        k = self.free[self.taken]
        self.taken += 1
        return k

    def data(self, k):
        return self.mem[k * self.B:(k + 1) * self.B]


class NetBuffer:
    def __init__(self, pool, frags=None):
        self.pool, self.frags = pool, [list(f) for f in (frags or [])]

    def __len__(self):
        return sum(e - s for _, s, e in self.frags)

    def slices(self):
        return [self.pool.data(k)[s:e].tobytes() for k, s, e in self.frags]

    def header(self):
        k, s, e = self.frags[0]
        return self.pool.data(k)[s:e]

    def trim_head(self, size):                          # buf.rs:294-329
        assert size <= len(self), "Should not trim more than buffer length"
        remaining = size
        while remaining > 0:                            # Remove entire buffers if needed
            k, s, e = self.frags[0]
            if e - s > remaining:
                break
            remaining -= e - s
            self.frags.pop(0)
        if remaining > 0:                               # Truncate the first buffer
            self.frags[0][1] += remaining

    def append_from_slice(self, data):                  # buf.rs:385-420
        if len(data) == 0:
            return
        if not self.frags:
            self.frags.append([self.pool.alloc(), 0, 0])
        off = 0
        while off < len(data):
            frag = self.frags[-1]
            n = min(self.pool.B - frag[2], len(data) - off)
            self.pool.data(frag[0])[frag[2]:frag[2] + n] = np.frombuffer(data[off:off + n], dtype=np.uint8)
            frag[2] += n
            off += n
            if off < len(data):
                self.frags.append([self.pool.alloc(), 0, 0])

    def append_from_buffer(self, other):                # buf.rs:442-447
        for s in other.slices():
            self.append_from_slice(s)

    def alloc_header(self, size):                       # buf.rs:262-291
        if not self.frags or self.frags[0][1] < size:
            self.frags.insert(0, [self.pool.alloc(head=True), self.pool.B - size, self.pool.B])
        else:
            self.frags[0][1] -= size
        k, s, _ = self.frags[0]
        self.pool.data(k)[s:s + size] = 0               # Zero out contents of header


class Stack:
    """The reference's globals: the local addresses, NEXT_PACKET_ID, and what send_packet saw."""

    def __init__(self, tx_pool, local4=L4, local6=L6, next_id=0):
        self.tx, self.local4, self.local6, self.next_id, self.sent = tx_pool, local4, local6, next_id, []

    def icmp_input(self, packet, source_ip):            # icmp.rs:44-85, both families
        v6 = len(source_ip) == 16
        seed = O.pseudo_header_py(source_ip, self.local6, len(packet), 58) if v6 else 0
        header = packet.header()
        if O.buffer_ones_comp_py(seed, packet.slices()) ^ 0xFFFF:
            return False
        packet_type = int(header[0])
        packet.trim_head(ICMP_HEADER_LEN)
        if packet_type != (128 if v6 else 8):
            return False
        self.tx.reserve()
        response = NetBuffer(self.tx)
        response.append_from_buffer(packet)
        self.icmp_output(response, 129 if v6 else 0, source_ip)
        return True

    def icmp_output(self, packet, packet_type, dest):   # icmp.rs:87-120
        packet.alloc_header(ICMP_HEADER_LEN)
        packet.header()[0] = packet_type
        seed = O.pseudo_header_py(self.local6, dest, len(packet), 58) if len(dest) == 16 else 0
        checksum = O.buffer_ones_comp_py(seed, packet.slices()) ^ 0xFFFF
        packet.header()[2:4] = list(checksum.to_bytes(2, "big"))
        if len(dest) == 16:
            self.ip_output_v6(packet, 58, dest)
        else:
            self.ip_output_v4(packet, 1, dest)

    def ip_output_v4(self, packet, protocol, dest):     # ip.rs:141-165
        packet.alloc_header(20)
        length = len(packet) & 0xFFFF
        h = packet.header()
        h[0] = 0x45
        h[2:4] = list(length.to_bytes(2, "big"))
        h[4:6] = list((self.next_id & 0xFFFF).to_bytes(2, "big"))
        self.next_id += 1
        h[8], h[9] = 64, protocol
        h[12:16], h[16:20] = list(self.local4), list(dest)
        h[10:12] = list(O.checksum_py(h[:20].tobytes()).to_bytes(2, "big"))
        self.sent.append(packet)

    def ip_output_v6(self, packet, protocol, dest):     # ip.rs:167-182
        length = len(packet) & 0xFFFF
        packet.alloc_header(40)
        h = packet.header()
        h[0] = 0x60
        h[4:6] = list(length.to_bytes(2, "big"))
        h[6], h[7] = protocol, 64
        h[8:24], h[24:40] = list(self.local6), list(dest)
        self.sent.append(packet)


def respond_ref(pkts, B, tx_mem, free, next_id=0, local4=L4, local6=L6):
    """The batch through ip_input's dispatch (as rx_verify_chain_ref restates it) and the echo path
    above, each datagram a chain of B-byte NetBuffers: (answered flags, the replies' NetBuffers, their
    source indices, the ids taken).  Datagrams the reference would panic on (T - h < 4) and the
    crossed-protocol cases are left unanswered, as the entry under test leaves them (unpinned)."""
    stack = Stack(Pool(tx_mem, free, B), local4, local6, next_id)
    answered, srcs = [], []
    for i, p in enumerate(pkts):
        frags = netbuffers(p, B) if len(p) else []
        st, _ = rx_verify_chain_ref(frags, local4, local6)
        ok = False
        if st & O.RX_ACCEPT:
            v6 = (p[0] >> 4) == 6
            h = 40 if v6 else (p[0] & 0xF) * 4
            proto = p[6] if v6 else p[9]
            if proto == (58 if v6 else 1) and len(p) - h >= 4:
                # the received chain in a pool of its own, trimmed to the L4 segment (ip.rs:92 / 119)
                mem = np.zeros(len(frags) * B, dtype=np.uint8)
                nb = NetBuffer(Pool(mem, [], B))
                for j, f in enumerate(frags):
                    mem[j * B:j * B + len(f)] = np.frombuffer(f, dtype=np.uint8)
                    nb.frags.append([j, 0, len(f)])
                nb.trim_head(h)
                ok = stack.icmp_input(nb, p[8:24] if v6 else p[12:16])
        answered.append(ok)
        if ok:
            srcs.append(i)
    return answered, stack.sent, srcs, stack.next_id - next_id


# ---------------------------------------------------------------------------
# request builders
# ---------------------------------------------------------------------------
def icmp_seg(typ, body, seed=0, code=0, corrupt=False):
    seg = bytearray([typ, code, 0, 0]) + bytearray(body)
    ck = O.ones_comp_py(seed, bytes(seg)) ^ 0xFFFF
    seg[2:4] = (ck ^ (0x0100 if corrupt else 0)).to_bytes(2, "big")
    return bytes(seg)


def ping4(body, src=R4, ihl=5, typ=8, **kw):
    return ip4(src, L4, 1, icmp_seg(typ, body, **kw), ihl=ihl)


def ping6(body, src=R6, typ=128, **kw):
    seed = O.pseudo_header_py(src, L6, 4 + len(body), 58)
    return ip6(src, L6, 58, icmp_seg(typ, body, seed=seed, **kw))


def body(tag, n):
    return O.splitmix64_bytes(0xEC40 + tag, max(n, 1))[:n].tobytes()


def body_summing_to(n, target, head_sum):
    """n >= 2 bytes (n even) whose big-endian words, added to head_sum, fold to `target`."""
    b = bytearray(body(n, n))
    b[0:2] = b"\0\0"
    cur = O.ones_comp_py(head_sum, bytes(b))
    need = (target - cur) % 0xFFFF
    if need == 0 and target == 0xFFFF and cur == 0:
        need = 0xFFFF
    b[0:2] = need.to_bytes(2, "big")
    assert O.ones_comp_py(head_sum, bytes(b)) == target
    return bytes(b)


def reply_datagrams(sent):
    """The replies as flat datagrams (what a peer receives)."""
    return [b"".join(nb.slices()) for nb in sent]


# ---------------------------------------------------------------------------
# the cases the CPU and the GPU tests share: name -> list of datagrams
# ---------------------------------------------------------------------------
def tcp4(n):
    from rx_place_helper import segment
    return segment(R4, 1234, 80, 1000, body(90, n))


def udp4(n):
    return ip4(R4, L4, 17, bytes(8) + body(91, n))


def short4(k):
    """IPv4, protocol 1, an L4 segment of k < 4 bytes whose checksum verifies where one can."""
    return ip4(R4, L4, 1, bytes([0xFF, 0xFF, 0, 0][:k]))


def short6(k):
    s = O.pseudo_header_py(R6, L6, k, 58)
    return ip6(R6, L6, 58, ((0xFFFF - s).to_bytes(2, "big") + b"\0\0")[:k])


def cases(B):
    lens = [0, 1, 2, 15, 16, 17, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1]
    c = {}
    c["lengths"] = [f(body(n, n)) for n in lens for f in (ping4, ping6)]
    ihl = []
    for k in range(5, 16):  # source shifts (4k + 4) & 15 = 8, 12, 0, 4; k = 15: header + ICMP = 64 bytes
        h = 4 * k
        for n in (B - h - 5, B - h - 4, B - h - 3, B + 33, 2 * B + 5):
            ihl.append(ping4(body(k * 7 + n, n), ihl=k))
    for n in (B - 45, B - 44, B - 43, B + 33, 2 * B + 5):
        ihl.append(ping6(body(n, n)))
    c["ihl"] = ihl
    c["big"] = [ping4(body(1, 65535 - 24)), ping6(body(2, 65535 - 44), src=R6B), ping4(body(3, 5), src=R4B)]
    sums = []
    for n in (8, 9, 64):
        sums += [ping4(bytes(n)), ping6(bytes(n))]  # IPv4: the stored checksum is 0xffff
    for n in (32, 2 * B + 2):
        b4 = body_summing_to(n, 0xFFFF, 0)  # the stored checksum is 0x0000
        sums += [ping4(b4), ping4(b4 + b"\0")]
        seed = O.pseudo_header_py(L6, R6, 4 + n, 58)
        b6 = body_summing_to(n, 0xFFFF, O.ones_comp_py(seed, bytes([129, 0, 0, 0])))
        sums.append(ping6(b6))
        seed = O.pseudo_header_py(L6, R6, 4 + n + 1, 58)
        sums.append(ping6(body_summing_to(n, 0xFFFF, O.ones_comp_py(seed, bytes([129, 0, 0, 0]))) + b"\0"))
    c["sums"] = sums
    c["code"] = [ping4(body(5, 40), code=7), ping6(body(6, 40), code=0x81), ping4(body(7, 3), code=255)]
    no = [ping4(body(10, 20), corrupt=True), ping6(body(11, 20), corrupt=True), ping4(body(12, 20), typ=0),
          ping6(body(13, 20), typ=129), ping4(body(14, 20), typ=128), ping6(body(15, 20), typ=8),
          ip6(R6, L6, 1, icmp_seg(8, body(16, 20))), ip6(R6, L6, 1, icmp_seg(128, body(17, 20))),
          ip4(R4, L4, 58, icmp_seg(128, body(18, 20))), tcp4(100), udp4(30),
          ip4(R4, L4, 1, icmp_seg(8, body(19, 20)), frag=0x2000), bytes([0x55]) + ping4(body(20, 20))[1:]]
    no += [short4(k) for k in range(4)] + [short6(k) for k in range(4)]
    rej = [ping4(body(30, 10))]
    for k, p in enumerate(no):
        rej += [p, (ping6 if k & 1 else ping4)(body(31 + k, 10 + 37 * k))]
    c["rejects"] = rej
    mixed = []
    for k in range(200):
        n = (k * 53) % (2 * B + 40)
        r = k % 7
        mixed.append(ping4(body(k, n), src=R4B if k & 8 else R4, ihl=5 + k % 3) if r in (0, 3) else
                     ping6(body(k, n), src=R6B if k & 8 else R6) if r in (1, 5) else
                     tcp4(n) if r == 2 else udp4(n) if r == 4 else ping4(body(k, n), typ=0))
    c["mixed"] = mixed
    return c


def expand_replies(free, tx_blk_first, head_len8, pay_len16, B):
    """The pool transmit form's chains: per reply its fragments [buffer, start, end)."""
    out = []
    for r in range(len(pay_len16)):
        if r % 64 == 0:
            at = int(tx_blk_first[r // 64])
        hl, pl = int(head_len8[r]), int(pay_len16[r])
        fr = [[int(free[at]), B - hl, B]]
        for j in range(-(-pl // B)):
            fr.append([int(free[at + 1 + j]), 0, min(B, pl - j * B)])
        at += len(fr)
        out.append(fr)
    return out
