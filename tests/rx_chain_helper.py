"""The receive path over a NetBuffer fragment chain, restated from the reference over a list of
fragments, and the datagram / chain builders the rx-chain tests share.

rx_verify_chain_ref is a literal restatement of ip_input / ip_input_v4 / ip_input_v6 /
ip_input_common (ip.rs:38-131), NetBuffer::trim_head (buf.rs:294-329), tcp::validate_checksum
(tcp.rs:838-850) and icmp_input_v4 / icmp_input_v6 (icmp.rs:44-75), built from the pinned
oracle's primitives (ones_comp_py, buffer_ones_comp_py, pseudo_header_py; pass
ones_comp=Oracle.compute_ones_comp for long fragments).  Where the Rust code would panic or
rejects the datagram the result is RX_MALFORMED, as in oracle.rx_verify_ref.  One case has no
pinned parity: an EMPTY fragment after the first makes compute_ones_comp panic (util.rs:92);
the entry under test lets it contribute nothing, and so does this helper.
"""
import numpy as np

from oracle import oracle as O
from test_rx_oracle import L4, L6, R4, R6, icmp4, ipv4, ipv6, tcp_seg


def trim_head(frags, size):
    """buf.rs:294-329 over a list of fragment byte strings (returns the new list)."""
    assert size <= sum(len(f) for f in frags), "Should not trim more than buffer length"
    frags = list(frags)
    remaining = size
    while remaining > 0:                       # Remove entire buffers if needed
        frag_len = len(frags[0])
        if frag_len > remaining:
            break
        remaining -= frag_len
        frags.pop(0)
    if remaining > 0:                          # Truncate the first buffer
        frags[0] = frags[0][remaining:]
    return frags


def rx_verify_chain_ref(frags, local4=L4, local6=L6, ones_comp=None):
    """(status bits, complemented L4 sum) for one datagram held as the fragment list `frags`."""
    oc = ones_comp or O.ones_comp_py
    frags = [bytes(f) for f in frags]
    if not frags:                              # header() asserts on an empty buffer
        return O.RX_MALFORMED, 0
    header = frags[0]                          # packet.header(): the first fragment only
    total = sum(len(f) for f in frags)
    if len(header) == 0:                       # header[0] panics
        return O.RX_MALFORMED, 0
    version = header[0] >> 4                   # ip.rs:39-40
    if version == 4:
        hdr = (header[0] & 0xF) * 4            # ip.rs:71
        if hdr == 0 or len(header) < 16 or hdr > len(header):
            return O.RX_MALFORMED, 0           # empty slice / header[12..16] / header[..hdr] panic
        st = O.RX_IP_OK if (0xFFFF ^ oc(0, header[:hdr])) == 0 else 0    # ip.rs:76-80
        if ((header[6] << 8 | header[7]) & 0x3FFF) != 0:                 # ip.rs:84-87
            st |= O.RX_FRAGMENT
        proto, src = header[9], header[12:16]
    elif version == 6:
        hdr = 40
        if len(header) < 24 or total < 40:     # header[8..24] / trim_head(40) panic
            return O.RX_MALFORMED, 0
        st = O.RX_IP_OK
        proto, src = header[6], header[8:24]
    else:
        return O.RX_MALFORMED, 0
    seg = trim_head(frags, hdr)
    seg_len = total - hdr                      # packet.len()

    def buf_sum(seed):                         # util.rs:112-119; an empty fragment adds nothing (unpinned)
        live = [f for f in seg if len(f)]
        if ones_comp is None:
            return O.buffer_ones_comp_py(seed, live)
        s = seed
        for f in live:                         # the same loop over the caller's compute_ones_comp
            s = oc(s, f)
        return s

    l4 = 0
    if proto == 6:                             # tcp.rs:838-850
        dst = local4 if len(src) == 4 else local6
        l4 = buf_sum(O.pseudo_header_py(src, dst, seg_len, 6)) ^ 0xFFFF
        st |= O.RX_L4_OK if l4 == 0 else 0
    elif proto == 1:                           # icmp.rs:44-50
        l4 = buf_sum(0) ^ 0xFFFF
        st |= O.RX_L4_OK if l4 == 0 else 0
    elif proto == 58:                          # icmp.rs:62-75
        if len(src) == 4:
            return O.RX_MALFORMED, 0
        l4 = buf_sum(O.pseudo_header_py(src, local6, seg_len, 58)) ^ 0xFFFF
        st |= O.RX_L4_OK if l4 == 0 else 0
    elif proto == 17:
        st |= O.RX_L4_UNCHECKED
    else:
        st |= O.RX_UNKNOWN
    if (st & O.RX_IP_OK) and not (st & O.RX_FRAGMENT) and (st & (O.RX_L4_OK | O.RX_L4_UNCHECKED)):
        st |= O.RX_ACCEPT
    return st, l4


# ---------------------------------------------------------------------------
# datagrams and splits
# ---------------------------------------------------------------------------
def make_datagrams(n, seed, max_body=1400):
    """Datagrams of every kind the receive path distinguishes: IPv4 TCP / UDP / ICMP, IPv6 TCP /
    ICMPv6, IHL 5-15, fragment bits, an unknown protocol, version 5, protocol 58 under IPv4,
    lengths 0-19, 39 and 40, and corrupted bytes."""
    w = O.splitmix64_words(seed, 4 * n)
    pkts = []
    for i in range(n):
        kind = i % 14
        size = int(w[4 * i + 1] % np.uint64(max_body))
        body = O.splitmix64_bytes(int(w[4 * i + 2]), size).tobytes()
        r = int(w[4 * i + 3])
        if kind == 0:
            p = ipv4(6, tcp_seg(R4, L4, body))
        elif kind == 1:
            p = ipv6(6, tcp_seg(R6, L6, body))
        elif kind == 2:
            p = ipv4(1, icmp4(body))
        elif kind == 3:
            p = ipv6(58, tcp_seg(R6, L6, body, proto=58, field=2, hlen=4))
        elif kind == 4:
            p = ipv4(17, body + b"\x00" * 8)
        elif kind == 5:
            p = ipv4(6, tcp_seg(R4, L4, body), frag=(r & 0x3FFF) | 1)
        elif kind == 6:
            p = ipv4(6, tcp_seg(R4, L4, body), ihl=5 + (i // 14) % 11)        # IHL 5..15
        elif kind == 7:
            p = ipv4(99, body)                                                # unknown protocol
        elif kind == 8:
            p = bytes([0x50 | (r & 0xF)]) + body                              # version 5
        elif kind == 9:
            p = ipv4(58, body + b"\x00" * 8)                                  # V4 source, V6 pseudo-header
        elif kind == 10:
            ln = (list(range(20)) + [39, 40])[(i // 14) % 22]
            full = ipv4(6, tcp_seg(R4, L4, body)) if (i // 14) % 2 else ipv6(6, tcp_seg(R6, L6, body))
            p = full[:ln]
        elif kind == 11:
            p = ipv6(17, body)
        elif kind == 12:
            p = ipv6(1, icmp4(body))                                          # protocol 1 in IPv6: no pseudo-header
        else:
            p = ipv4(6, tcp_seg(R4, L4, body))
        p = bytearray(p)
        if kind == 13 or (r >> 40) % 5 == 0:                                  # corrupt one byte somewhere
            if len(p):
                p[(r >> 16) % len(p)] ^= 1 << (r & 7)
        pkts.append(bytes(p))
    return pkts


def ipv4_long(proto, payload):
    """test_rx_oracle.ipv4 for datagrams past 65535 bytes (the total-length field, which the
    receive path never reads, holds the low 16 bits)."""
    h = bytearray(20)
    h[0] = 0x45
    h[2:4] = ((20 + len(payload)) & 0xFFFF).to_bytes(2, "big")
    h[8], h[9] = 64, proto
    h[12:16], h[16:20] = R4, L4
    h[10:12] = O.checksum_py(bytes(h)).to_bytes(2, "big")
    return bytes(h) + payload


def split_even(pkt, hdr_min, w):
    """Cut pkt into fragments: the first holds at least hdr_min bytes and every non-final
    fragment leaves an even number of bytes after an even header (so the per-fragment fold
    equals the flat one)."""
    cuts, pos = [], 0
    first = True
    k = 0
    while pos < len(pkt):
        step = 2 * (1 + int(w[k % len(w)] % np.uint64(300)))
        k += 1
        if first:
            step = max(step, (hdr_min + 1) & ~1)
            first = False
        cuts.append(pkt[pos:pos + step])
        pos += step
    return cuts


def split_any(pkt, w, small=False):
    """Cut pkt into fragments of arbitrary (odd too) lengths; small: many 1..7-byte ones."""
    cuts, pos, k = [], 0, 0
    while pos < len(pkt):
        r = int(w[k % len(w)])
        k += 1
        step = 1 + (r % 7 if (small or r & 0x100) else (r >> 9) % 600)
        cuts.append(pkt[pos:pos + step])
        pos += step
    return cuts


def netbuffers(pkt, buf_bytes=512):
    """recv_packet's chain: full buf_bytes fragments, the last the remainder."""
    return [pkt[i:i + buf_bytes] for i in range(0, len(pkt), buf_bytes)]


def hdr_len(pkt):
    """Bytes the first fragment must hold for header() to show the whole IP header."""
    if not pkt:
        return 0
    v = pkt[0] >> 4
    return (pkt[0] & 0xF) * 4 if v == 4 else 40 if v == 6 else 0


# ---------------------------------------------------------------------------
# chains in an arena
# ---------------------------------------------------------------------------
def lay_chains(chains, seed=1, align=None, shuffled=False, slack=64, base=0):
    """Place every fragment of every chain into a byte arena.  align=None: arbitrary byte
    alignment with random gaps; align=k: every fragment at the next multiple of k.  shuffled:
    the fragments' memory order is a permutation.  Returns (arena uint8, frag_off uint64,
    frag_len uint32, first uint32)."""
    frs = [f for c in chains for f in c]
    nf = len(frs)
    w = O.splitmix64_words(seed, max(2 * nf, 1))
    order = np.argsort(w[:nf], kind="stable") if shuffled else np.arange(nf)
    off = np.zeros(nf, dtype=np.uint64)
    pos = base
    for rank, j in enumerate(order):
        if align:
            pos = (pos + align - 1) // align * align
        else:
            pos += int(w[nf + rank] % np.uint64(19))
        off[j] = pos
        pos += len(frs[j])
    arena = np.frombuffer(O.splitmix64_bytes(seed ^ 0xA5A5, pos + slack).tobytes(), dtype=np.uint8).copy()
    for j, f in enumerate(frs):
        arena[int(off[j]):int(off[j]) + len(f)] = np.frombuffer(f, dtype=np.uint8)
    first = np.zeros(len(chains) + 1, dtype=np.uint32)
    np.cumsum([len(c) for c in chains], out=first[1:])
    return arena, off, np.array([len(f) for f in frs], dtype=np.uint32), first
