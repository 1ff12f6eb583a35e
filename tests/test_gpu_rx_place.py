"""TCP receive placement over pool buffers (rns_rx_tcp_place_pool_dev / batch.rx_tcp_place_pool) on
the GPU.  Every status, L4 sum, meta record and stream byte is compared with the restatement in
tests/rx_place_helper.py; the stream is pre-filled with a sentinel no payload byte equals, so a stray
write and a missing one both show.  Every call also checks that the pool is unchanged."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.place import meta_records, rx_flow_table, rx_tcp_place_pool
from rx_place_helper import (ACK, FIN, L4, L6, NO_FLOW, P_DONE, P_FLOW, P_OUTSIDE, P_TCP, PSH, R4, R6, RST, SENTINEL, SYN,
                             body_bytes, expected, icmp4, ip4, key_of, lay_pool, pool_index, segment, tcp, udp4)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUFS = (128, 512)
V4B = bytes([10, 1, 2, 3])
V6B = bytes.fromhex("20010db8000000000000000000000042")


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def dev(a, view):
    return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(DEV)


def place(pool, idx, blk, len16, buf, table, next_seq, win_off, win_len, stream0):
    """One call over host arrays: (status, l4, meta records, stream) as numpy; the pool is only read."""
    d_pool = torch.from_numpy(pool).to(DEV)
    d_stream = torch.from_numpy(np.ascontiguousarray(stream0)).to(DEV)
    n = len16.size
    l4 = torch.full((n,), 0x5555, dtype=torch.uint16, device=DEV)
    meta = torch.full((n, 24), 0xEE, dtype=torch.uint8, device=DEV)
    st, out, m = rx_tcp_place_pool(d_pool, dev(idx.astype(np.uint32), np.int32), dev(blk.astype(np.uint32), np.int32),
                                   dev(len16, np.int16), L4, L6, torch.from_numpy(table).to(DEV),
                                   dev(np.asarray(next_seq, dtype=np.uint32), np.int32),
                                   dev(np.asarray(win_off, dtype=np.uint64), np.int64),
                                   dev(np.asarray(win_len, dtype=np.uint32), np.int32), d_stream, buf_bytes=buf,
                                   l4_sum=l4, meta=meta)
    torch.cuda.synchronize()
    assert out is l4 and m is meta
    assert np.array_equal(d_pool.cpu().numpy(), pool), "the pool changed"
    return st.cpu().numpy(), l4.view(torch.int16).cpu().numpy().view(np.uint16), meta_records(meta), d_stream.cpu().numpy()


def same(got, want):
    for g, w, what in zip(got, want, ("status", "l4", "meta", "stream")):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, [(int(i), g[i], w[i]) for i in bad[:6]])


def check(pkts, buf, keys, next_seq, win_off, win_len, stream_bytes, oracle, shuffled=False, seed=1, bend=None,
          status=None, table=None):
    """Lay the datagrams out, run the entry and compare everything with the restatement.  `bend`
    edits the buffer indices after the layout (with `status` the verdicts that follow from it)."""
    pool, idx, blk, len16 = lay_pool(pkts, buf, shuffled, seed)
    if bend is not None:
        bend(idx, pool_index(len16, buf)[1])
    stream0 = np.full(stream_bytes, SENTINEL, dtype=np.uint8)
    want = expected(pkts, buf, keys, next_seq, win_off, win_len, stream0, status=status,
                    ones_comp=oracle.compute_ones_comp)
    got = place(pool, idx, blk, len16, buf, rx_flow_table(keys) if table is None else table, next_seq, win_off, win_len,
                stream0)
    same(got, want)
    return want


# 1. payload sizes x destination alignments x source skips -----------------------------------------
# (source skip = ip_hdr + tcp_hdr: 40, 44, 52, 60, 72, 80, 100 and the largest, 120)
SKIPS = ((V4B, 5, 5), (V4B, 6, 5), (V4B, 5, 8), (V6B, 5, 5), (V6B, 5, 8), (V4B, 15, 5), (V6B, 5, 15), (V4B, 15, 15))


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("buf", BUFS)
def test_sizes_alignments_skips(oracle, buf, shuffled):
    pkts, keys, next_seq, win_off, win_len = [], [], [], [], []
    at = 32
    for f, (src, ihl, doff) in enumerate(SKIPS):
        skip = (ihl * 4 if len(src) == 4 else 40) + doff * 4
        assert skip in (40, 44, 52, 60, 72, 80, 100, 120)
        sizes = (0, 1, 15, 16, 17, buf - skip, buf - skip + 1, 3 * buf + 5)
        keys.append(key_of(src, 1000 + f, 80))
        next_seq.append(0x1000 * (f + 1))
        pos = 0
        for a in range(16):                               # the destination's alignment, by the seq offset
            n = sizes[(a + f) % 8]
            pos = (pos + 15) // 16 * 16 + 16 + a            # a gap of sentinel bytes before every segment
            pkts.append(segment(src, 1000 + f, 80, next_seq[f] + pos, body_bytes(100 * f + a, n), ihl=ihl, doff=doff))
            pos += n
        win_off.append(at)                                  # 16-byte aligned in a 256-byte-aligned tensor
        win_len.append(pos + 3)
        at += (pos + 3 + 31) // 16 * 16
    pkts.insert(7, udp4(V4B, b"bystander"))
    pkts.insert(70, icmp4(V4B, b"ping" * 5))
    assert len(pkts) == 130                                 # three blocks
    want = check(pkts, buf, keys, next_seq, win_off, win_len, at + 64, oracle, shuffled, seed=buf)
    done = want[2][(want[2]["place"] & P_DONE) != 0]
    assert done.size == 8 * 14 and set(done["pay_len"].tolist()) >= {1, 15, 16, 17, 3 * buf + 5}
    assert (want[2]["place"][[7, 70]] == 0).all() and (want[0][[7, 70]] & O.RX_ACCEPT).all()


# 2. datagram counts: across a block, and the most datagrams per lane the verify picks --------------
def pick_k(mean):
    """The launcher's datagrams per lane for a mean buffer count (chain_pick_k, rns_checksum.hip)."""
    K, best = 1, -1.0
    for k in range(1, 9):
        fr = k * mean
        fill = fr / math.ceil(fr) if fr > 0 else 1.0
        if fill > best + 0.02:
            best, K = fill, k
    return K


@pytest.mark.parametrize("buf", BUFS)
@pytest.mark.parametrize("n,two", [(65, 20), (513, 320)])
def test_counts(oracle, buf, n, two):
    """One flow's in-order stream cut into n segments, `two` of them in two buffers, sent shuffled."""
    rng = np.random.default_rng(n)
    lens = np.concatenate([rng.integers(buf - 40 + 1, 2 * buf - 40 + 1, two), rng.integers(1, buf - 40 + 1, n - two)])
    rng.shuffle(lens)
    if n == 513:
        assert pick_k((n + two) / n) == 8                       # 64 * 8 + 1 datagrams: two waves of the verify
    data = body_bytes(n, int(lens.sum()))
    seqs = 0xFFFF0000 + np.concatenate([[0], np.cumsum(lens)[:-1]])
    order = rng.permutation(n)
    pkts = [segment(R4, 5555, 80, int(seqs[i]), data[int(seqs[i]) - 0xFFFF0000:][:int(lens[i])]) for i in order]
    keys = [key_of(R4, 5555, 80)]
    want = check(pkts, buf, keys, [0xFFFF0000], [16], [len(data)], len(data) + 48, oracle, shuffled=True, seed=n)
    assert (want[2]["place"] == (P_TCP | P_FLOW | P_DONE)).all()
    assert want[3][16:16 + len(data)].tobytes() == data       # the in-order sender's bytes


# 3. a buffer index outside the pool ------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 2])
def test_buffer_outside_the_pool(oracle, which):
    buf = 128
    keys = [key_of(R4, 7, 8)]
    lens = [50, 300, 60, 90, 200]
    seqs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    pkts = [segment(R4, 7, 8, 100 + int(s), body_bytes(40 + i, ln)) for i, (s, ln) in enumerate(zip(seqs, lens))]
    status = [None] * 5
    status[1] = (O.RX_MALFORMED, 0)

    def bend(idx, first):
        idx[first[1] + which] = 0x00FFFFFF                    # datagram 1's head, or its last buffer

    want = check(pkts, buf, keys, [100], [0], [sum(lens)], sum(lens) + 16, oracle, shuffled=True, bend=bend, status=status)
    assert want[2]["place"].tolist() == [7, 0, 7, 7, 7] and want[2]["flow"][1] == NO_FLOW
    assert (want[3][50:350] == SENTINEL).all()                # nothing placed for it, the neighbours intact


# 4. window edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("buf", BUFS)
def test_window_edges(oracle, buf):
    F = [key_of(R4, 1, 80), key_of(R4, 2, 80), key_of(R6, 3, 80), key_of(R4, 4, 80), key_of(R4, 5, 80)]
    next_seq = [5000, 0xFFFFFF00, 70000, 9000, 100]
    win_len = [1000, 0x300, 400, 0, 256]
    stream_bytes = 2700
    win_off = [8, 1100, 1900, 2350, stream_bytes - 255]           # the last window reaches one byte past the stream
    S = lambda f, seq, n, tag, **kw: segment(F[f][0], F[f][1], 80, seq, body_bytes(tag, n), **kw)  # noqa: E731
    pkts = [
        S(0, 5000, 100, 1),                                        # d = 0
        S(0, 5000 + 1000 - 37, 37, 2),                             # fits exactly at the end
        S(0, 5000 + 1000 - 36, 37, 3),                             # one byte over
        S(0, 5000 + 1000, 1, 4),                                   # d = win_len
        S(0, 4000, 100, 5),                                        # stale
        S(0, 4995, 10, 6),                                         # straddling next_seq
        S(0, 5000 + 0x80000000, 10, 7),                            # half the sequence space away
        S(1, 0xFFFFFF00, 0x80, 8),                                 # up to the wrap
        S(1, 0xFFFFFF80, 0x100, 9),                                # across it
        S(1, 0x80, 0x180, 10),                                     # after it, to the window's end
        S(1, 0x200, 1, 11),                                        # just past the end
        S(2, 70000 + 399, 1, 12),                                  # the last byte
        S(2, 70000 + 150, 251, 13),                                # one over, IPv6
        S(3, 9000, 1, 14),                                         # win_len 0
        S(4, 100, 5, 15),                                          # a window past stream_bytes: nothing is taken
        S(4, 110, 200, 16),
        S(0, 5200, 0, 17),                                         # a pure ACK
        S(0, 5300, 7, 18, flags=ACK | FIN),                        # FIN carries data like any other
    ]
    want = check(pkts, buf, F, next_seq, win_off, win_len, stream_bytes, oracle, shuffled=True, seed=3)
    D, X = P_TCP | P_FLOW | P_DONE, P_TCP | P_FLOW | P_OUTSIDE
    assert want[2]["place"].tolist() == [D, D, X, X, X, X, X, D, D, D, X, D, X, X, X, X, P_TCP | P_FLOW, D]
    assert (want[3][win_off[4]:] == SENTINEL).all() and (want[3][1100:1100 + 0x300] != SENTINEL).all()


# 5. what is not placed -------------------------------------------------------------------------------
@pytest.mark.parametrize("buf", BUFS)
def test_not_placed(oracle, buf):
    keys = [key_of(R4, 9, 80)]
    good = segment(R4, 9, 80, 1000, body_bytes(1, 200))
    bad_tcp, bad_ip = bytearray(good), bytearray(good)
    bad_tcp[-1] ^= 0x40
    bad_ip[8] ^= 1
    seg19 = bytearray(19)
    seg19[16:18] = (O.ones_comp_py(O.pseudo_header_py(R4, L4, 19, 6), bytes(seg19)) ^ 0xFFFF).to_bytes(2, "big")
    pkts = [
        bytes(bad_tcp),                                            # a bad TCP checksum on a known flow
        bytes(bad_ip),                                             # a bad IP checksum
        ip4(R4, L4, 6, tcp(R4, L4, 9, 80, 1000, body_bytes(2, 50)), frag=0x2000),  # an IPv4 fragment
        udp4(R4, body_bytes(3, 60)),
        icmp4(R4, body_bytes(4, 60)),
        segment(R4, 9, 80, 1000, body_bytes(5, 30), flags=ACK | RST),
        segment(R4, 9, 80, 1000, body_bytes(6, 30), flags=SYN),
        segment(R4, 9, 80, 1000, body_bytes(7, 30), doff=4, hlen=20),      # data offset 4
        segment(R4, 9, 80, 1000, body_bytes(8, 10), doff=15, hlen=20),     # data offset beyond L
        ip4(R4, L4, 6, bytes(seg19)),                              # L = 19
        segment(R4, 9, 80, 1300, body_bytes(9, 40)),               # and one that is
    ]
    want = check(pkts, buf, keys, [1000], [0], [400], 400, oracle, seed=5)
    acc = (want[0] & O.RX_ACCEPT) != 0
    assert acc.tolist() == [False, False, False, True, True, True, True, True, True, True, True]
    assert want[2]["place"].tolist() == [0, 0, 0, 0, 0, 3, 3, 0, 0, 0, 7]
    assert (want[3][:300] == SENTINEL).all() and (want[3][340:] == SENTINEL).all()


# 6. lookup --------------------------------------------------------------------------------------------
def flow_keys(n):
    rng = np.random.default_rng(n)
    same4, same6 = bytes([1, 2, 3, 4]), bytes([1, 2, 3, 4]) + bytes(12)
    keys = [key_of(same4, 10, 20), key_of(same4, 10, 21), key_of(same4, 11, 20), key_of(same6, 10, 20)][:n]
    seen = set(keys)
    while len(keys) < n:
        k = key_of(bytes(rng.integers(0, 256, 4 if len(keys) % 3 else 16, dtype=np.uint8)), int(rng.integers(1, 65536)),
                   int(rng.integers(1, 65536)))
        if k not in seen:
            seen.add(k)
            keys.append(k)
    return keys


@pytest.mark.parametrize("n_flows", [1, 65, 2048])
def test_lookup(oracle, n_flows):
    """Every flow sends one segment into its own 32-byte window; keys next to the table's (another
    dport, sport, family, address byte) match nothing."""
    keys = flow_keys(n_flows)
    slots = max(64, 1 << (2 * n_flows - 1).bit_length())
    assert rx_flow_table(keys).size == 32 * slots and (n_flows != 2048 or slots == 2 * n_flows)  # 2048: a minimal table
    pkts = [segment(k[0], k[1], k[2], 7 + f, body_bytes(f, 1 + f % 23)) for f, k in enumerate(keys)]
    near = []
    for k in keys[:4]:
        other = bytes([k[0][0] ^ 0x80]) + k[0][1:]
        swap = k[0] + bytes(12) if len(k[0]) == 4 else (k[0][:4] if k[0][4:] == bytes(12) else other)
        near += [key_of(k[0], k[1], k[2] ^ 0x100), key_of(k[0], k[1] ^ 1, k[2]), key_of(other, k[1], k[2]),
                 key_of(swap, k[1], k[2])]
    near = [k for k in near if k not in set(keys)]
    pkts += [segment(k[0], k[1], k[2], 7, body_bytes(9, 5)) for k in near]
    order = np.random.default_rng(1).permutation(len(pkts))
    pkts = [pkts[i] for i in order]
    next_seq = 7 + np.arange(n_flows)
    want = check(pkts, 128, keys, next_seq, 32 * np.arange(n_flows), [32] * n_flows, 32 * n_flows, oracle, shuffled=True)
    assert sorted(want[2]["flow"].tolist()) == list(range(n_flows)) + [NO_FLOW] * len(near) and len(near) >= 3
    assert (want[2]["place"][want[2]["flow"] == NO_FLOW] == P_TCP).all()


def test_no_flows_and_a_garbage_table(oracle):
    keys = flow_keys(65)
    pkts = [segment(k[0], k[1], k[2], 7, body_bytes(f, 9)) for f, k in enumerate(keys)]
    # no flows: every segment is unmatched, whatever the table argument holds
    want = check(pkts, 128, [], [], [], [], 64, oracle, table=np.zeros(0, dtype=np.uint8))
    assert (want[2]["place"] == P_TCP).all()
    # garbage of the right size: the call ends, and every flow is none or inside the per-flow arrays
    pool, idx, blk, len16 = lay_pool(pkts, 128)
    rng = np.random.default_rng(8)
    for fill in ("random", "ones", "taken"):
        tbl = rng.integers(0, 256, 32 * 256, dtype=np.uint8)
        if fill == "ones":
            tbl[:] = 0xFF
        elif fill == "taken":                                       # every slot marked taken, no key matches
            w = tbl.view("<u4").reshape(-1, 8)
            w[:, 7] = 1
            w[:, 6] = rng.integers(0, 200, 256)
        stream0 = np.full(65 * 16, SENTINEL, dtype=np.uint8)
        st, l4, meta, stream = place(pool, idx, blk, len16, 128, tbl, [7] * 65, 16 * np.arange(65), [16] * 65, stream0)
        assert np.array_equal(st, want[0]) and np.array_equal(l4, want[1])
        assert ((meta["flow"] == NO_FLOW) | (meta["flow"] < 65)).all()
        assert (meta["flow"] == NO_FLOW).all() and (meta["place"] == P_TCP).all(), fill  # (no such key by chance)
        assert (stream == SENTINEL).all()


# 7. arrival order does not matter ---------------------------------------------------------------------
@pytest.mark.parametrize("buf", BUFS)
def test_order(oracle, buf):
    rng = np.random.default_rng(50)
    lens = rng.integers(1, 2 * buf, 50)
    data = body_bytes(50, int(lens.sum()))
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    segs = [segment(R6, 443, 50000, 0xFFFFF000 + int(s), data[int(s):int(s) + int(ln)]) for s, ln in zip(starts, lens)]
    keys = [key_of(R6, 443, 50000)]
    arenas = []
    for order in (np.arange(50)[::-1], rng.permutation(50)):
        want = check([segs[i] for i in order], buf, keys, [0xFFFFF000], [5], [len(data)], len(data) + 21, oracle,
                     shuffled=True, seed=int(order[0]))
        arenas.append(want[3])
    assert np.array_equal(arenas[0], arenas[1])
    assert arenas[0][5:5 + len(data)].tobytes() == data and (arenas[0][:5] == SENTINEL).all()


# 8. wrapper checks -------------------------------------------------------------------------------------
def test_wrapper_arguments():
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=DEV)  # noqa: E731
    args = [z(4096, torch.uint8), z(1, torch.int32), z(1, torch.int32), z(1, torch.int16), L4, L6, z(2048, torch.uint8),
            z(1, torch.int32), z(1, torch.int64), z(1, torch.int32), z(64, torch.uint8)]
    st, l4, meta = rx_tcp_place_pool(*args)
    torch.cuda.synchronize()
    assert l4 is None and st.cpu().tolist() == [O.RX_MALFORMED] and meta.shape == (1, 24)
    assert meta_records(meta)["flow"].tolist() == [NO_FLOW]
    with pytest.raises(ValueError):
        rx_tcp_place_pool(*args, buf_bytes=64)
    with pytest.raises(ValueError):
        rx_tcp_place_pool(*args, meta=z(23, torch.uint8))
    with pytest.raises(ValueError):
        rx_tcp_place_pool(*args[:8], z(2, torch.int64), *args[9:])
    with pytest.raises(TypeError):
        rx_tcp_place_pool(*args[:7], z(1, torch.int64), *args[8:])
    e = rx_tcp_place_pool(args[0], z(0, torch.int32), z(0, torch.int32), z(0, torch.int16), *args[4:])
    assert e[0].numel() == 0 and e[2].shape == (0, 24)


# 9. a pool and a stream past 4 GiB -----------------------------------------------------------------------
def test_past_4gib(oracle):
    """Buffers at pool offsets >= 2^32 and a window at a stream offset >= 2^32: the window and 4 KiB
    on either side are compared, with a second flow's window at the stream's start."""
    buf = 512
    line = (1 << 32) // buf
    nbuf = line + 4096
    stream_bytes = (1 << 32) + (1 << 20)
    try:
        big = torch.empty(nbuf * buf, dtype=torch.uint8, device=DEV)
        stream = torch.empty(stream_bytes, dtype=torch.uint8, device=DEV)
    except RuntimeError as e:  # out of memory
        pytest.skip(f"no room for a pool and a stream past 4 GiB: {e}")
    try:
        rng = np.random.default_rng(4)
        lens = rng.integers(1, 1461, 150)
        data = [body_bytes(60 + f, int(lens[f::2].sum())) for f in (0, 1)]
        keys = [key_of(R4, 1, 2), key_of(R6, 1, 2)]
        next_seq, pos, pkts = [77, 0xFFFFFE00], [0, 0], []
        for i, ln in enumerate(lens):
            f = i % 2
            pkts.append(segment(keys[f][0], 1, 2, next_seq[f] + pos[f], data[f][pos[f]:pos[f] + int(ln)]))
            pos[f] += int(ln)
        order = rng.permutation(150)
        pkts = [pkts[i] for i in order]
        len16 = np.array([len(p) for p in pkts], dtype=np.uint16)
        blk, first, nf = pool_index(len16, buf)
        idx = (line + 50 + rng.permutation(nf)).astype(np.uint32)  # every buffer above the 4 GiB line
        host = np.zeros((nf, buf), dtype=np.uint8)
        for i, p in enumerate(pkts):
            for j in range(0, len(p), buf):
                host[first[i] + j // buf, :len(p[j:j + buf])] = np.frombuffer(p[j:j + buf], dtype=np.uint8)
        where = torch.from_numpy(idx.astype(np.int64)).to(DEV)
        big.view(nbuf, buf)[where] = torch.from_numpy(host).to(DEV)
        win_off = [(1 << 32) + 4096 + 3, 11]
        win_len = [len(data[0]), len(data[1])]
        lo0, hi0 = win_off[0] - 4096, win_off[0] + win_len[0] + 4096
        hi1 = win_off[1] + win_len[1] + 4096
        stream[lo0:hi0] = SENTINEL
        stream[:hi1] = SENTINEL
        st, _, meta = rx_tcp_place_pool(big, dev(idx, np.int32), dev(blk, np.int32), dev(len16, np.int16), L4, L6,
                                        torch.from_numpy(rx_flow_table(keys)).to(DEV),
                                        dev(np.array(next_seq, dtype=np.uint32), np.int32),
                                        dev(np.array(win_off, dtype=np.uint64), np.int64),
                                        dev(np.array(win_len, dtype=np.uint32), np.int32), stream)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == (O.RX_IP_OK | O.RX_L4_OK | O.RX_ACCEPT)).all()
        m = meta_records(meta)
        assert (m["place"] == (P_TCP | P_FLOW | P_DONE)).all() and m["flow"].tolist() == (order % 2).tolist()
        assert m["pay_len"].tolist() == lens[order].tolist()
        for f, lo, hi in ((0, lo0, hi0), (1, 0, hi1)):
            got = stream[lo:hi].cpu().numpy()
            want = np.full(hi - lo, SENTINEL, dtype=np.uint8)
            want[win_off[f] - lo:win_off[f] - lo + win_len[f]] = np.frombuffer(data[f], dtype=np.uint8)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (f, bad[:8].tolist())
        assert np.array_equal(big.view(nbuf, buf)[where].cpu().numpy(), host), "the pool changed"
    finally:
        del big, stream
        torch.cuda.empty_cache()
