"""Receive verify over NetBuffer fragment chains (rns_rx_verify_chain_dev / batch.rx_verify_chain)
on the GPU: status bytes and L4 values, compared exactly, with the flat receive verify
(batch.rx_verify), the pinned oracle (oracle.rx_verify_ref on the flat bytes, where every
non-final trimmed fragment is even) and the chain restatement (tests/rx_chain_helper.py:
ip.rs:38-131, buf.rs:294-329, tcp.rs:838-850, icmp.rs:44-75 over a list of fragments).  Every call
also checks that the arena is unchanged."""
import socket

import numpy as np
import pytest
import torch

from oracle import oracle as O
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import recv_batch_chain, rx_verify, rx_verify_chain
from rx_chain_helper import (hdr_len, ipv4_long, lay_chains, make_datagrams, netbuffers, rx_verify_chain_ref,
                             split_any)
from test_gpu_chains import CHAIN_SHAPES
from test_rx_oracle import L4, L6, R4, R6, icmp4, ipv4, ipv6, tcp_seg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAL = O.RX_MALFORMED


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def dev(a, view):
    return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(DEV)


def run(arena, off, ln, first, l4=True, d_arena=None):
    """rx_verify_chain over host descriptors: (status uint8, l4 uint16 or None); the arena is
    only read."""
    d_arena = torch.from_numpy(arena).to(DEV) if d_arena is None else d_arena
    n = first.size - 1
    l4t = torch.full((n,), 0x5555, dtype=torch.uint16, device=DEV) if l4 else None
    st, out = rx_verify_chain(d_arena, dev(off.astype(np.uint64), np.int64), dev(ln.astype(np.uint32), np.int32),
                              dev(first.astype(np.uint32), np.int32), L4, L6, l4_sum=l4t)
    torch.cuda.synchronize()
    assert out is l4t
    if arena is not None:
        assert np.array_equal(d_arena.cpu().numpy(), arena), "the arena changed"
    return st.cpu().numpy(), (l4t.view(torch.int16).cpu().numpy().view(np.uint16) if l4 else None)


def expect(chains, oracle):
    w = [rx_verify_chain_ref(c, L4, L6, ones_comp=oracle.compute_ones_comp) for c in chains]
    return np.array([x[0] for x in w], dtype=np.uint8), np.array([x[1] for x in w], dtype=np.uint16)


def same(got, want, chains):
    for g, w, what in zip(got, want, ("status", "l4")):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, [(int(i), hex(int(g[i])), hex(int(w[i])), [len(f) for f in chains[i]][:8])
                                      for i in bad[:6]])


# 1. one fragment per datagram -------------------------------------------------------------
def test_one_fragment_equals_flat_verify(oracle):
    pkts = make_datagrams(14 * 22, 0x1F4A)  # 308: every kind, IHL 5-15, lengths 0-19, 39, 40
    chains = [[p] for p in pkts]
    arena, off, ln, first = lay_chains(chains, seed=11)  # arbitrary byte alignment
    got = run(arena, off, ln, first)
    want = expect(chains, oracle)
    assert len(set(want[0].tolist())) >= 7
    same(got, want, chains)
    flat = [O.rx_verify_ref(p, L4, L6, ones_comp=oracle.compute_ones_comp) for p in pkts]
    assert np.array_equal(want[0], np.array([f[0] for f in flat], dtype=np.uint8))
    l4 = torch.empty(len(pkts), dtype=torch.uint16, device=DEV)
    st = rx_verify(torch.from_numpy(arena).to(DEV), dev(off, np.int64), dev(ln, np.int32), L4, L6, l4_sum=l4)
    torch.cuda.synchronize()
    assert np.array_equal(got[0], st.cpu().numpy())
    assert np.array_equal(got[1], l4.view(torch.int16).cpu().numpy().view(np.uint16))


# 2. NetBuffer chains ----------------------------------------------------------------------
LENGTHS = (20, 21, 40, 41, 60, 511, 512, 513, 532, 533, 1024, 1500, 2048)


def datagram_of(L, i):
    """A datagram of exactly L bytes: IPv4 TCP / IPv6 TCP / ICMPv4 / UDP by turns where L allows."""
    body = O.splitmix64_bytes(0xD0 + i, L).tobytes()
    k = i % 5
    if k == 1 and L >= 60:
        p = ipv6(6, tcp_seg(R6, L6, body[:L - 60]))
    elif k == 2 and L >= 24:
        p = ipv4(1, icmp4(body[:L - 24]))
    elif k == 3:
        p = ipv4(17, body[:L - 20])
    elif L >= 40:
        p = ipv4(6, tcp_seg(R4, L4, body[:L - 40]))
    else:
        p = ipv4(6, body[:L - 20])  # a segment shorter than a TCP header: still summed
    assert len(p) == L
    if i % 7 == 6:
        p = bytearray(p)
        p[(i * 31) % L] ^= 0x20
    return bytes(p)


@pytest.fixture(scope="module")
def netbuffer_batch(oracle):
    pkts = [datagram_of(LENGTHS[i % len(LENGTHS)], i) for i in range(1000)]
    want = [O.rx_verify_ref(p, L4, L6, ones_comp=oracle.compute_ones_comp) for p in pkts]
    return pkts, (np.array([w[0] for w in want], dtype=np.uint8), np.array([w[1] for w in want], dtype=np.uint16))


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 513, 1000])
def test_netbuffer_chains(netbuffer_batch, n, shuffled):
    pkts, want = netbuffer_batch
    chains = [netbuffers(p) for p in pkts[:n]]
    arena, off, ln, first = lay_chains(chains, seed=n, align=512, shuffled=shuffled)
    assert (off % 512 == 0).all()
    same(run(arena, off, ln, first), (want[0][:n], want[1][:n]), chains)


# 3. odd fragments ---------------------------------------------------------------------------
def test_odd_fragments(oracle):
    pkts = make_datagrams(14 * 30, 0x0DD, max_body=700)
    w = O.splitmix64_words(0x0DE, 8192)
    chains = []
    for i, p in enumerate(pkts):
        if i % 2:  # the first fragment holds the header and 0..4 bytes more, then any cuts
            k = min(len(p), hdr_len(p) + int(w[i] % np.uint64(5)))
            chains.append(([p[:k]] if k else []) + split_any(p[k:], w[i:], small=i % 4 == 1))
        else:
            chains.append(split_any(p, w[i:], small=i % 4 == 0))
    sizes = {len(f) for c in chains for f in c}
    assert 1 in sizes and 7 in sizes and max(len(c) for c in chains) > 64
    want = expect(chains, oracle)
    assert len(set(want[0].tolist())) >= 6
    for shuffled in (False, True):
        arena, off, ln, first = lay_chains(chains, seed=5, shuffled=shuffled)
        same(run(arena, off, ln, first), want, chains)


# 4. head edges ------------------------------------------------------------------------------
def test_head_edges(oracle):
    v4 = ipv4(6, tcp_seg(R4, L4, b"edge" * 30))
    v4o = ipv4(6, tcp_seg(R4, L4, b"opts" * 30), ihl=7)
    v6 = ipv6(6, tcp_seg(R6, L6, b"six" * 41))
    v6i = ipv6(58, tcp_seg(R6, L6, b"icmp6" * 9, proto=58, field=2, hlen=4))
    chains = [
        [v4[:20], v4[20:]], [v4[:21], v4[21:]],                 # len0 == hdr, hdr + 1
        [v4o[:28], v4o[28:]], [v4o[:29], v4o[29:]],
        [v4[:15], v4[15:]], [v4[:16], v4[16:]],                 # IPv4 len0 15 / 16 (hdr > len0)
        [v4o[:20], v4o[20:]],                                   # hdr 28 > len0 20
        [v4[:20]], [v4[:20], b""],                              # an empty segment
    ]
    for len0 in (23, 24, 25, 39, 40, 41):                       # the IPv6 header crossing fragments
        chains.append([v6[:len0], v6[len0:]])
        chains.append([v6i[:len0], v6i[len0:len0 + 9], v6i[len0 + 9:]])
    chains += [
        [v6[:24], v6[24:31], v6[31:38], v6[38:39], v6[39:]],    # the header over four short fragments
        [v6[:25], v6[25:40], v6[40:]],                          # an odd first fragment, the cut at 40
        [v6[:24], v6[24:39]], [v6[:24], v6[24:40]],             # T = 39 / 40
        [v6[:39]], [v6[:40]],
        [],                                                     # no fragments
        [b"", v4],                                              # len0 == 0
        [v4[:20], b"", v4[20:]],                                # an empty fragment in the middle (parity unpinned)
        [v4[:40], v4[40:41], b"", b"", v4[41:]],
    ]
    want = expect(chains, oracle)
    arena, off, ln, first = lay_chains(chains, seed=21)
    same(run(arena, off, ln, first), want, chains)
    assert want[0][4] == MAL and want[0][5] == MAL and want[0][6] == MAL

    # malformed ranges and fragments outside the arena: four plain chains, then the descriptors bent
    plain = [[v4[:30], v4[30:]], [v6[:50], v6[50:]], [v4o[:40], v4o[40:90], v4o[90:]], [v4]]
    pw = expect(plain, oracle)
    arena, off, ln, first = lay_chains(plain, seed=22)
    nf = off.size
    base = run(arena, off, ln, first)
    same(base, pw, plain)
    f2 = first.copy()
    f2[2] = first[1] - 1                                        # first descending: datagram 1 = [2, 1)
    st, l4 = run(arena, off, ln, f2)
    assert st[1] == MAL and l4[1] == 0 and st[3] == pw[0][3] and st[0] == pw[0][0]
    f3 = first.copy()
    f3[-1] = nf + 1                                             # first past n_frags
    st, l4 = run(arena, off, ln, f3)
    assert st[3] == MAL and l4[3] == 0 and np.array_equal(st[:3], pw[0][:3])
    for j in (int(first[2]), int(first[2]) + 1):                # a head / a payload fragment past the arena end
        o2 = off.copy()
        o2[j] = arena.size - 5
        st, l4 = run(arena, o2, ln, first)
        assert st[2] == MAL and l4[2] == 0
        assert np.array_equal(np.delete(st, 2), np.delete(pw[0], 2))
    o3 = off.copy()
    o3[0] = np.uint64(2 ** 63)
    assert run(arena, o3, ln, first)[0][0] == MAL


# 5. pass boundaries ---------------------------------------------------------------------------
def test_pass_boundaries(oracle):
    w = O.splitmix64_words(0xB0DE, 4096)
    long70 = ipv4(6, tcp_seg(R4, L4, O.splitmix64_bytes(70, 70 * 30).tobytes()))
    seven = ipv6(6, tcp_seg(R6, L6, O.splitmix64_bytes(7, 200 * 7 - 60).tobytes()))
    assert len(seven) == 1400
    pkts = make_datagrams(14 * 12, 0xB0DF, max_body=900)
    chains = [netbuffers(p, 128) for p in pkts]
    chains[40] = [long70[:40]] + [long70[40 + 30 * k:40 + 30 * (k + 1)] for k in range(68)] + [long70[40 + 30 * 68:]]
    chains[41] = [seven[7 * k:7 * k + 7] for k in range(200)]   # len0 = 7: malformed, over four passes
    chains[42] = [seven[:28]] + [seven[28 + 7 * k:28 + 7 * k + 7] for k in range(196)]  # 24 <= len0 < 40: the exact loop
    chains[43] = [seven[:42]] + [seven[42 + 7 * k:42 + 7 * k + 7] for k in range(194)]
    assert len(chains[40]) == 70 and len(chains[41]) == 200 and b"".join(chains[42]) == b"".join(chains[43]) == seven
    want = expect(chains, oracle)
    arena, off, ln, first = lay_chains(chains, seed=31)
    same(run(arena, off, ln, first), want, chains)

    # a head fragment that is the 64th fragment of its wave: nine 7-fragment datagrams, then the rest
    p = ipv4(6, tcp_seg(R4, L4, O.splitmix64_bytes(9, 7 * 40 - 40).tobytes()))
    lane63 = [[p[40 * k:40 * k + 40] for k in range(7)] for _ in range(9)]
    q = ipv4(6, tcp_seg(R4, L4, O.splitmix64_bytes(10, 500).tobytes()))
    lane63.append([q[:20], q[20:300], q[300:]])                 # head = fragment 63, payload in the next pass
    lane63.append([q[:21], q[21:301], q[301:]])
    lane63 += [split_any(x, w[i:]) for i, x in enumerate(pkts[:60])]
    first = np.cumsum([0] + [len(c) for c in lane63])
    assert first[9] == 63
    want = expect(lane63, oracle)
    arena, off, ln, first = lay_chains(lane63, seed=32)
    same(run(arena, off, ln, first), want, lane63)


# 6. large -------------------------------------------------------------------------------------
def ipv6_long(proto, payload):
    h = bytearray(40)
    h[0] = 0x60
    h[4:6] = (len(payload) & 0xFFFF).to_bytes(2, "big")
    h[6], h[7] = proto, 64
    h[8:24], h[24:40] = R6, L6
    return bytes(h) + payload


def test_large(oracle):
    big = 200 * 1024
    icmp = ipv4_long(1, icmp4(O.splitmix64_bytes(0x1C, big + 3000).tobytes()))
    v6 = ipv6_long(6, tcp_seg(R6, L6, O.splitmix64_bytes(0x16, 70001).tobytes()))
    v4 = ipv4_long(6, tcp_seg(R4, L4, O.splitmix64_bytes(0x14, 66000).tobytes()))
    assert len(v6) - 40 > 65535 and len(v4) - 20 > 65535
    bad4 = bytearray(v4)
    bad4[40000] ^= 4
    chains = [
        [icmp[:1001], icmp[1001:1001 + big], icmp[1001 + big:]],     # a 200 KiB fragment behind an odd head
        [icmp],                                                      # the head fragment itself past 128 KiB
        [icmp[:20], icmp[20:20 + big + 1], icmp[20 + big + 1:]],
        netbuffers(v6), netbuffers(v4), netbuffers(bytes(bad4)),
        [v6[:30000], v6[30000:]], [v4[:131072 + 20], v4[131072 + 20:]],  # exactly 128 KiB after the trim: no wrap
        [v4[:131072 + 22], v4[131072 + 22:]],
        [ipv4(6, tcp_seg(R4, L4, b"small"))],
    ]
    want = expect(chains, oracle)
    flat = O.rx_verify_ref(icmp, L4, L6, ones_comp=oracle.compute_ones_comp)
    assert (int(want[0][1]), int(want[1][1])) == flat                # one fragment: the flat value
    assert want[0][3] & O.RX_ACCEPT and want[0][4] & O.RX_ACCEPT and not want[0][5] & O.RX_L4_OK
    arena, off, ln, first = lay_chains(chains, seed=41)
    same(run(arena, off, ln, first), want, chains)


# 7. outputs and streams -------------------------------------------------------------------------
def test_optional_l4_and_streams(netbuffer_batch):
    pkts, want = netbuffer_batch
    n = 300
    chains = [netbuffers(p) for p in pkts[:n]]
    arena, off, ln, first = lay_chains(chains, seed=51, align=512, shuffled=True)
    st, none = run(arena, off, ln, first, l4=False)
    assert none is None and np.array_equal(st, want[0][:n])
    d_arena = torch.from_numpy(arena).to(DEV)
    s = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        same(run(arena, off, ln, first, d_arena=d_arena), (want[0][:n], want[1][:n]), chains)
    status = torch.zeros(n, dtype=torch.uint8, device=DEV)       # caller-supplied outputs
    out, _ = rx_verify_chain(d_arena, dev(off, np.int64), dev(ln, np.int32), dev(first, np.int32), L4, L6,
                             status=status)
    torch.cuda.synchronize()
    assert out is status and np.array_equal(status.cpu().numpy(), want[0][:n])
    with pytest.raises(ValueError):
        rx_verify_chain(d_arena, dev(off, np.int64), dev(ln, np.int32), dev(first, np.int32), L4, L6,
                        status=torch.zeros(n + 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        rx_verify_chain(d_arena, dev(off, np.int64).to(torch.int32), dev(ln, np.int32), dev(first, np.int32), L4, L6)
    e = rx_verify_chain(d_arena, dev(off[:0], np.int64), dev(ln[:0], np.int32), dev(first[:1], np.int32), L4, L6)
    assert e[0].numel() == 0


# 8. an arena of 4 GiB and more ----------------------------------------------------------------------
def test_arena_past_4gib(oracle):
    """The 64-bit-address instantiation: chains whose fragments lie on both sides of the 4 GiB line
    (a pass inside one buffer window), and the same chains alternating with copies near the
    arena's start (passes spanning more than 4 GiB: 64-bit loads)."""
    four_g = 1 << 32
    nbytes = four_g + (16 << 20)
    pkts = make_datagrams(14 * 10, 0x4610, max_body=1200)
    w = O.splitmix64_words(0x4611, 2048)
    chains = [netbuffers(p) if i % 2 else split_any(p, w[i:]) for i, p in enumerate(pkts)]
    want = expect(chains, oracle)
    mini, off, ln, first = lay_chains(chains, seed=61, shuffled=True)
    assert mini.size < (8 << 20)
    big = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    try:
        lo, hi = 4096, four_g - (mini.size // 2 & ~15) + 3
        d_mini = torch.from_numpy(mini).to(DEV)
        big[lo:lo + mini.size].copy_(d_mini)
        big[hi:hi + mini.size].copy_(d_mini)
        o_hi = off + np.uint64(hi)
        assert (o_hi < four_g).any() and (o_hi >= four_g).any()
        got = run(None, o_hi, ln, first, d_arena=big)
        same(got, want, chains)
        # datagram i from the high copy, the next from the low one
        nfr = np.diff(first.astype(np.int64))
        alt = np.repeat(np.arange(len(chains)) % 2 == 0, nfr)
        o_alt = np.where(alt, o_hi, off + np.uint64(lo))
        same(run(None, o_alt, ln, first, d_arena=big), want, chains)
        torch.cuda.synchronize()
        assert np.array_equal(big[hi:hi + mini.size].cpu().numpy(), mini)
        assert np.array_equal(big[lo:lo + mini.size].cpu().numpy(), mini)
    finally:
        del big
        torch.cuda.empty_cache()


# 9. end to end ----------------------------------------------------------------------------------
def test_socket_to_verdict(oracle):
    pkts = [p for p in make_datagrams(14 * 12, 0xE2E, max_body=1900) if 0 < len(p) <= 2048]
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    try:
        a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 1 << 20)
        a.setblocking(False)  # a full queue fails the test at once
        for p in pkts:
            a.send(p)
        nbuf = 4 * len(pkts) + 4
        pool = np.zeros(nbuf * 512, dtype=np.uint8)
        free = np.random.default_rng(9).permutation(nbuf).astype(np.uint32)
        n, off, ln, first, nf = recv_batch_chain(b.fileno(), pool, free, timeout_ms=1000)
    finally:
        a.close()
        b.close()
    assert n == len(pkts)
    chains = [netbuffers(p) for p in pkts]
    assert [int(x) for x in np.diff(first.astype(np.int64))] == [len(c) for c in chains]
    same(run(pool, off, ln, first), expect(chains, oracle), chains)


@pytest.mark.parametrize("pattern,n", CHAIN_SHAPES)
def test_k_branches(oracle, pattern, n):
    """Every K branch of the receive launcher (K = 1, 2 and the general form; it has no deep
    form): datagrams of every kind cut into exactly the pattern's fragment counts (the first
    fragment holds the IP header and a few bytes more, the rest is cut evenly, odd pieces
    included), at arbitrary byte alignment."""
    pkts = make_datagrams(n, 0x4B1 + n, max_body=900)
    chains = []
    for i, p in enumerate(pkts):
        k = pattern[i % len(pattern)]
        if k == 1 or len(p) < 2 * k:
            cuts = [0] + [len(p)] * k      # short datagrams: trailing empty fragments keep the count
        else:
            h = min(hdr_len(p) + i % 5, len(p) - (k - 1))
            step = -(-(len(p) - h) // (k - 1))
            cuts = [0] + [min(h + j * step, len(p)) for j in range(k)]
        chains.append([p[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    assert sum(len(c) for c in chains) * len(pattern) == n * sum(pattern)
    arena, off, ln, first = lay_chains(chains, seed=n)
    same(run(arena, off, ln, first), expect(chains, oracle), chains)
