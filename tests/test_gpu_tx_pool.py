"""Transmit finalize of datagrams in fixed-size pool buffers (rns_tx_fill_pool_dev /
batch.tx_fill_pool) on the GPU.  One checker for every case: the datagrams are laid into a pool of
random bytes, the entry runs, and every pool byte and every status is compared with (a)
Oracle.tx_chain_fill on a host copy with the CSR chains the compact form expands to and (b)
rns_tx_fill_chain_dev on a second device copy with the same chains."""
import socket

import numpy as np
import pytest
import torch

from oracle import oracle as O
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import rx_verify_chain, tx_fill_chain, tx_fill_pool, tx_pool_layout
from rustnetworkstack_amd.pipeline import TxPoolPipeline
from rustnetworkstack_amd.workloads import TxPoolBatch
from test_gpu_tx import outgoing
from test_gpu_tx_chain_packed import cut
from test_gpu_tx_packed import edge_datagrams
from test_rx_oracle import L4, L6, R4, R6, ipv4, ipv6, tcp_seg
from tx_pool_helper import expand, lay_pool, place

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAL = _lib.RNS_TX_MALFORMED
FILLED = _lib.RNS_TX_IP_FILLED | _lib.RNS_TX_L4_FILLED


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def dev(a, view):
    return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(DEV)


def same(got, want, got_st, want_st, what):
    bad = np.flatnonzero(got_st != want_st)
    assert bad.size == 0, (what, [(int(i), int(got_st[i]), int(want_st[i])) for i in bad[:5]])
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (what, [(int(d), int(got[d]), int(want[d])) for d in diff[:8]])


def run_pool(d_pool, idx, blk, hl, pl, buf, n_frags=None, **kw):
    d_idx = dev(idx.astype(np.uint32), np.int32)[:idx.size if n_frags is None else n_frags]
    st = tx_fill_pool(d_pool, d_idx, dev(blk.astype(np.uint32), np.int32), dev(hl, np.uint8), dev(pl, np.int16),
                      buf_bytes=buf, **kw)
    torch.cuda.synchronize()
    return st


def check(oracle, pool, idx, blk, hl, pl, buf, pool_bytes=None, n_frags=None, twice=False):
    """The checker.  Returns (the pool after the finalize, the statuses, the expanded chains)."""
    pool = pool if pool_bytes is None else pool[:pool_bytes]
    off, ln, first = expand(idx, blk, hl, pl, buf, n_frags)
    want = pool.copy()
    want_st = oracle.tx_chain_fill(want, off, ln, first)
    d_pool = torch.from_numpy(pool).to(DEV)
    st = run_pool(d_pool, idx, blk, hl, pl, buf, n_frags)
    if twice:
        once = d_pool.cpu().numpy()
        st2 = run_pool(d_pool, idx, blk, hl, pl, buf, n_frags)
        same(d_pool.cpu().numpy(), once, st2.cpu().numpy(), st.cpu().numpy(), "the second run")
    got, got_st = d_pool.cpu().numpy(), st.cpu().numpy()
    same(got, want, got_st, want_st, "oracle")
    d_csr = torch.from_numpy(pool).to(DEV)
    st_csr = tx_fill_chain(d_csr, dev(off, np.int64), dev(ln, np.int32), dev(first, np.int32))
    torch.cuda.synchronize()
    same(got, d_csr.cpu().numpy(), got_st, st_csr.cpu().numpy(), "tx_fill_chain")
    return got, got_st, (off, ln, first)


# 1. every kind of datagram ------------------------------------------------------------------
@pytest.fixture(scope="module")
def kinds():
    return cut(outgoing(5000, 0x7E57))


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("buf", [256, 512, 2048])
def test_kinds(oracle, kinds, buf, shuffled):
    heads, pays = kinds
    pool, idx, blk, hl, pl, _ = lay_pool(heads, pays, buf, shuffled=shuffled, seed=buf)
    _, st, _ = check(oracle, pool, idx, blk, hl, pl, buf)
    assert len(set(st.tolist())) >= 4


# 2. wave and block edges ----------------------------------------------------------------------
def tcp4(body):
    return ipv4(6, tcp_seg(L4, R4, body))


@pytest.fixture(scope="module")
def mtu():
    return cut([tcp4(O.splitmix64_bytes(0xB10C + i, 1460).tobytes()) for i in range(700)])


@pytest.mark.parametrize("mode", ["full", "alternating", "first_block_heads"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 700])
def test_wave_and_block_edges(oracle, mtu, n, mode):
    heads = mtu[0][:n]
    drop = {"full": lambda i: False, "alternating": lambda i: i % 2 == 1, "first_block_heads": lambda i: i < 64}[mode]
    pays = [b"" if drop(i) else p for i, p in enumerate(mtu[1][:n])]
    pool, idx, blk, hl, pl, _ = lay_pool(heads, pays, 512, shuffled=True, seed=n)
    _, st, _ = check(oracle, pool, idx, blk, hl, pl, 512)
    assert (st == FILLED).all()


# 3. length edges ------------------------------------------------------------------------------
def head_kinds():
    """(name, maker): maker(payload) -> (head, payload) with the head's total length in the name."""
    def v4udp(p):
        return ipv4(17, bytes(8) + p)[:28], p
    def v4tcp(p):
        return tcp4(p)[:40], p
    def v4tcp41(p):                                    # one payload byte in the head: an odd L4 part
        d = tcp4(b"\xa7" + p)
        return d[:41], p
    def v6tcp(p):
        return ipv6(6, tcp_seg(L6, R6, p))[:60], p
    def v4opt(p):
        return ipv4(6, tcp_seg(L4, R4, p), ihl=15)[:80], p
    def v6tcpopt(p):                                   # 40 bytes of TCP options: past the stash
        return ipv6(6, tcp_seg(L6, R6, p, hlen=60))[:100], p
    def v4opt85(p):                                    # the TCP field itself past the stash: read from the pool
        return ipv4(6, tcp_seg(L4, R4, b"\x5c" * 5 + p), ihl=15)[:85], p
    return [("v4udp28", v4udp), ("v4tcp40", v4tcp), ("v4tcp41", v4tcp41), ("v6tcp60", v6tcp), ("v4opt80", v4opt),
            ("v6tcpopt100", v6tcpopt), ("v4opt85", v4opt85)]


@pytest.mark.parametrize("buf", [256, 512])
def test_length_edges(oracle, buf):
    heads, pays, want_len = [], [], {"v4udp28": 28, "v4tcp40": 40, "v4tcp41": 41, "v6tcp60": 60, "v4opt80": 80,
                                     "v6tcpopt100": 100, "v4opt85": 85}
    for name, make in head_kinds():
        for k, size in enumerate((0, 1, 2, buf - 1, buf, buf + 1, 2 * buf, 2 * buf + 1)):
            h, p = make(O.splitmix64_bytes(size * 31 + k + len(name), size).tobytes())
            assert len(h) == want_len[name] and len(p) == size
            heads.append(h)
            pays.append(p)
    # an ICMPv4 datagram whose segment is all zero: seed 0, sum 0, stored 0xffff
    z = bytearray(ipv4(1, bytes(8 + 600)))
    heads.append(bytes(z[:28]))
    pays.append(bytes(z[28:]))
    for shuffled in (False, True):
        pool, idx, blk, hl, pl, first = lay_pool(heads, pays, buf, shuffled=shuffled, seed=3)
        got, st, (off, _, cfirst) = check(oracle, pool, idx, blk, hl, pl, buf)
        v6 = np.array([h[0] >> 4 == 6 for h in heads])
        assert np.array_equal(st, np.where(v6, _lib.RNS_TX_L4_FILLED, FILLED))
        zo = int(off[cfirst[len(heads) - 1]])
        assert got[zo + 22:zo + 24].tolist() == [0xFF, 0xFF]
    # one flipped payload byte in the first, a middle and the last buffer: the field follows the oracle
    body = O.splitmix64_bytes(0xF11B, 4 * buf + 77).tobytes()
    base_h, base_p = cut([tcp4(body)])
    fields = set()
    for pos, bit in ((None, 0), (5, 0x01), (2 * buf + 9, 0x04), (4 * buf + 76, 0x10)):  # distinct changes of the sum
        p = bytearray(base_p[0])
        if pos is not None:
            p[pos] ^= bit
        pool, idx, blk, hl, pl, _ = lay_pool(base_h, [bytes(p)], buf, shuffled=True, seed=4)
        got, st, (off, _, _) = check(oracle, pool, idx, blk, hl, pl, buf)
        assert st[0] == FILLED
        fields.add(bytes(got[int(off[0]) + 36:int(off[0]) + 38]))
    assert len(fields) == 4


# 4. header-length edges, maximal datagrams -----------------------------------------------------
def test_edge_datagrams(oracle):
    """IHL 5..15 against every field position, IPv6 short segments, 65535-byte datagrams (256
    payload buffers of 256 bytes: many passes for one owner), malformed and empty ones.  A datagram
    the form cannot describe (head > 255 B, payload > 65535 B) is dropped."""
    pkts = edge_datagrams()
    heads, pays = cut(pkts)
    keep = [i for i in range(len(pkts)) if len(heads[i]) <= 255 and len(pays[i]) <= 65535]
    assert len(pkts) - len(keep) <= len(pkts) // 20
    heads, pays = [heads[i] for i in keep], [pays[i] for i in keep]
    assert max(-(-len(p) // 256) for p in pays) == 256
    for buf, shuffled in ((256, True), (512, False)):
        pool, idx, blk, hl, pl, _ = lay_pool(heads, pays, buf, shuffled=shuffled, seed=0x22)
        check(oracle, pool, idx, blk, hl, pl, buf)


# 5. rejections that touch one datagram only ------------------------------------------------------
def test_rejections(oracle):
    buf, n = 512, 130
    heads = [tcp4(b"")[:40]] * n
    pays = [O.splitmix64_bytes(0x4E1 + i, 1 + (i * 211) % 1700).tobytes() for i in range(n)]
    pool, idx, blk, hl, pl, first = lay_pool(heads, pays, buf, shuffled=True, seed=5, spare=0)
    nbuf = idx.size
    assert int((pl > 2 * buf).sum()) > 10

    def rejected(st, who, **kw):
        who = sorted(who)
        assert np.flatnonzero(st == MAL).tolist() == who, (kw, np.flatnonzero(st == MAL).tolist(), who)
        assert (np.delete(st, who) == FILLED).all()

    long = [i for i in range(n) if first[i + 1] - first[i] >= 4]
    # an index past the pool as head, middle and last buffer; index 0xFFFFFFFF
    for i, slot, val in ((long[0], 0, nbuf), (long[1], 2, nbuf + 7), (long[2], -1, nbuf), (long[3], 1, 0xFFFFFFFF),
                         (70, 0, 0xFFFFFFFF)):
        bad = idx.copy()
        k = int(first[i]) + slot if slot >= 0 else int(first[i + 1]) - 1
        bad[k] = val
        got, st, _ = check(oracle, pool, bad, blk, hl, pl, buf)
        rejected(st, [i], case=(i, slot, val))
        assert np.array_equal(got.reshape(-1, buf)[idx[first[i]]], pool.reshape(-1, buf)[idx[first[i]]])
    # pool_bytes ending exactly at, and one byte before, the end of the highest buffer's used bytes
    top = int(np.argmax(idx))                                       # the fragment in the highest buffer
    owner = int(np.searchsorted(first, top, side="right")) - 1
    off, ln, _ = expand(idx, blk, hl, pl, buf)
    end = int(off[top]) + int(ln[top])
    _, st, _ = check(oracle, pool, idx, blk, hl, pl, buf, pool_bytes=end)
    rejected(st, [])
    _, st, _ = check(oracle, pool, idx, blk, hl, pl, buf, pool_bytes=end - 1)
    rejected(st, [owner])
    # a d_blk_first entry that pushes a block's tail past n_frags, and one near 2^32.  The blocks'
    # entries are independent, so block 1 (head-only datagrams here, one buffer each) may lie last
    # in d_buf_idx; moved on by 3, its datagram j names the head buffer of datagram j + 3 — every
    # head buffer still named once — and its last 3 datagrams run past n_frags.
    pays_h = [b"" if 64 <= i < 128 else p for i, p in enumerate(pays)]
    pool_h, idx_h, blk_h, hl_h, pl_h, first_h = lay_pool(heads, pays_h, buf, shuffled=True, seed=55, spare=0)
    f64, f128 = int(first_h[64]), int(first_h[128])
    assert f128 - f64 == 64
    idx_r = np.concatenate([idx_h[:f64], idx_h[f128:], idx_h[f64:f128]])
    blk_r = np.array([0, idx_h.size - 64, f64], dtype=np.uint32)
    _, st, _ = check(oracle, pool_h, idx_r, blk_r, hl_h, pl_h, buf)
    rejected(st, [])
    blk_r[1] += 3
    _, st, _ = check(oracle, pool_h, idx_r, blk_r, hl_h, pl_h, buf)
    rejected(st, [125, 126, 127])
    blk_r[1] = 0xFFFFFFF0
    _, st, _ = check(oracle, pool_h, idx_r, blk_r, hl_h, pl_h, buf)
    rejected(st, list(range(64, 128)))
    # n_frags cut by one: the last datagram's range runs out
    _, st, _ = check(oracle, pool, idx, blk, hl, pl, buf, n_frags=nbuf - 1)
    rejected(st, [n - 1])
    # head_len 0 with and without payload, a 19-byte IPv4 head
    hl2, pl2 = hl.copy(), pl.copy()
    hl2[3], hl2[66], hl2[100] = 0, 0, 19
    pl2[66] = 0
    blk2, first2, nf2 = tx_pool_layout(pl2, buf)
    idx2 = np.delete(idx, np.arange(int(first[66]) + 1, int(first[67])))
    assert idx2.size == nf2
    pool2 = pool.copy()
    pool2.reshape(-1, buf)[idx[first[100]], buf - 19:] = np.frombuffer(heads[100][:19], dtype=np.uint8)
    _, st, _ = check(oracle, pool2, idx2, blk2, hl2, pl2, buf)
    rejected(st, [3, 66, 100])
    # two datagrams sharing their payload buffers (distinct heads): both get correct fields
    share = idx.copy()
    nfr = (first[1:] - first[:-1]).astype(np.int64)
    a, b = long[0], next(i for i in long[1:] if nfr[i] == nfr[long[0]])
    share[first[b] + 1:first[b + 1]] = idx[first[a] + 1:first[a + 1]]
    pl3 = pl.copy()
    pl3[b] = pl[a]
    _, st, _ = check(oracle, pool, share, blk, hl, pl3, buf)
    rejected(st, [])


# 6. idempotence and the receive side -----------------------------------------------------------
def test_idempotent_and_accepted_by_receive_verify(oracle, mtu):
    n, buf = 300, 512
    pays = [p[:1 + (i * 97) % 1460] for i, p in enumerate(mtu[1][:n])]
    heads = [ipv4(6, O.splitmix64_bytes(i, 20).tobytes() + p)[:40] for i, p in enumerate(pays)]  # from R4 to L4
    pool, idx, blk, hl, pl, _ = lay_pool(heads, pays, buf, shuffled=True, seed=6)
    got, st, (off, ln, first) = check(oracle, pool, idx, blk, hl, pl, buf, twice=True)
    assert (st == FILLED).all()
    rx, _ = rx_verify_chain(torch.from_numpy(got).to(DEV), dev(off, np.int64), dev(ln, np.int32), dev(first, np.int32),
                            L4, L6)
    torch.cuda.synchronize()
    assert (rx.cpu().numpy() == (O.RX_IP_OK | O.RX_L4_OK | O.RX_ACCEPT)).all()


# 7. workload batches ------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("config,n", [("c3_1500B", 2 ** 16), ("c5_imix", 2 ** 17)])
def test_workload_batches(config, n, shuffled):
    b = TxPoolBatch(config, DEV, n=n, shuffled=shuffled)
    assert b.n == n and b.d_buf_idx.numel() == b.n_frags
    twin = b.arena.clone()
    st = tx_fill_pool(b.arena, b.d_buf_idx, b.d_blk_first, b.d_head_len8, b.d_pay_len16, buf_bytes=512, status=b.status)
    st_csr = tx_fill_chain(twin, b.d_off, b.d_len, b.d_first)
    torch.cuda.synchronize()
    assert st is b.status and bool((st == FILLED).all()) and torch.equal(st, st_csr)
    assert torch.equal(b.arena, twin)


# 8. a pool just over 4 GiB ----------------------------------------------------------------------
def test_pool_past_4gib(oracle, kinds):
    """The 64-bit-address instantiation: buffers below, on both sides of and above the 4 GiB line —
    passes inside one buffer window — and a wave whose buffers alternate between the pool's start
    and its end (a pass spanning more than 4 GiB: 64-bit loads).  Only the named buffers are
    compared."""
    buf = 512
    nbuf = (1 << 32) // buf + 4096
    try:
        big = torch.empty(nbuf * buf, dtype=torch.uint8, device=DEV)
    except RuntimeError as e:  # out of memory
        pytest.skip(f"no room for a pool past 4 GiB: {e}")
    rows = big.view(nbuf, buf)
    try:
        heads, pays = kinds[0][:220], kinds[1][:220]
        hl = np.array([len(h) for h in heads], dtype=np.uint8)
        pl = np.array([len(p) for p in pays], dtype=np.uint16)
        blk, first, nf = tx_pool_layout(pl, buf)
        line = (1 << 32) // buf
        layouts = {
            "straddling": line - nf // 2 + np.arange(nf),                       # consecutive indices across the line
            "above": line + 100 + np.random.default_rng(3).permutation(nf),
            "spread": np.where(np.arange(nf) % 2 == 0, 8 + np.arange(nf), nbuf - 1 - np.arange(nf)),
        }
        host = np.frombuffer(O.splitmix64_bytes(0x4616, nf * buf).tobytes(), dtype=np.uint8).copy().reshape(nf, buf)
        place(host, np.arange(nf), first, heads, pays, buf)
        # the same chains in a small pool (buffer k of the small pool = the big pool's buffer where[k])
        off, ln, cfirst = expand(np.arange(nf, dtype=np.uint32), blk, hl, pl, buf)
        want = host.reshape(-1).copy()
        want_st = oracle.tx_chain_fill(want, off, ln, cfirst)
        assert len(set(want_st.tolist())) >= 4
        for name, where in layouts.items():
            idx = where.astype(np.uint32)
            assert name != "straddling" or ((idx < line).any() and (idx >= line).any())
            at = torch.from_numpy(idx.astype(np.int64)).to(DEV)
            rows[at] = torch.from_numpy(host).to(DEV)
            st = run_pool(big, idx, blk, hl, pl, buf)
            same(rows[at].cpu().numpy().reshape(-1), want, st.cpu().numpy(), want_st, name)
    finally:
        del big, rows
        torch.cuda.empty_cache()


# 9. wrapper checks and the optional status --------------------------------------------------------
def test_optional_outputs(oracle, kinds):
    n, buf = 300, 512
    pool, idx, blk, hl, pl, _ = lay_pool(kinds[0][:n], kinds[1][:n], buf, shuffled=True, seed=9)
    want, want_st, _ = check(oracle, pool, idx, blk, hl, pl, buf)
    d_pool = torch.from_numpy(pool).to(DEV)
    args = (d_pool, dev(idx, np.int32), dev(blk, np.int32), dev(hl, np.uint8), dev(pl, np.int16))
    lib = _lib.load()
    with torch.cuda.device(DEV):                                   # d_status NULL
        assert lib.rns_tx_fill_pool_dev(d_pool.data_ptr(), d_pool.numel(), 9, args[1].data_ptr(), idx.size,
                                        args[2].data_ptr(), args[3].data_ptr(), args[4].data_ptr(), n, None,
                                        torch.cuda.current_stream().cuda_stream) == _lib.RNS_OK
    torch.cuda.synchronize()
    assert np.array_equal(d_pool.cpu().numpy(), want)
    status = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    out = tx_fill_pool(*args, status=status)
    torch.cuda.synchronize()
    assert out is status and np.array_equal(status.cpu().numpy(), want_st)
    with pytest.raises(ValueError):
        tx_fill_pool(*args, status=torch.zeros(n + 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        tx_fill_pool(*args, buf_bytes=500)
    with pytest.raises(ValueError):
        tx_fill_pool(*args, buf_bytes=128)
    with pytest.raises(ValueError):
        tx_fill_pool(d_pool[8:], *args[1:])                        # not 16-byte aligned
    with pytest.raises(ValueError):
        tx_fill_pool(args[0], args[1], args[2][:4], *args[3:])     # too few block entries
    with pytest.raises(ValueError):
        tx_fill_pool(*args[:3], args[3][:-1], args[4])             # one head length short
    with pytest.raises(TypeError):
        tx_fill_pool(args[0], args[1].to(torch.int64), *args[2:])
    with pytest.raises(ValueError, match="no CPU fallback"):
        tx_fill_pool(args[0], args[1].cpu(), *args[2:])
    e = tx_fill_pool(d_pool, dev(idx[:0], np.int32), dev(blk[:0], np.int32), dev(hl[:0], np.uint8), dev(pl[:0], np.int16))
    assert e.numel() == 0


# 10. the pipeline ---------------------------------------------------------------------------------
def test_pipeline(oracle):
    buf = 512
    pkts = [p for p in outgoing(260, 0xE31) if p]
    heads, pays = cut(pkts)
    first_b, second_b = list(range(0, 120)), list(range(120, 150))
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    need = sum(1 + -(-len(pays[i]) // buf) for i in first_b)
    pipe = TxPoolPipeline(pool_bufs=need + 4, max_pkts=256, buf_bytes=buf)
    try:
        a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 4 << 20)
        b.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 4 << 20)
        a.setblocking(False)
        b.setblocking(False)
        pipe.host.array[:] = np.frombuffer(O.splitmix64_bytes(0x70, pipe.host.array.size).tobytes(), dtype=np.uint8)

        def batch(which):
            hs, ps = [heads[i] for i in which], [pays[i] for i in which]
            hl, pl = [len(h) for h in hs], [len(p) for p in ps]
            idx = pipe.alloc(hl, pl)
            blk, first, nf = tx_pool_layout(np.array(pl), buf)
            assert idx.size == nf
            place(pipe.host.array.reshape(-1, buf), idx, first, hs, ps, buf)
            st = pipe.send(a.fileno(), idx, hl, pl)
            want = [O.tx_chain_fill_ref([h] + ([p] if p else []), ones_comp=oracle.compute_ones_comp) for h, p in zip(hs, ps)]
            assert st.tolist() == [w[1] for w in want]
            got = []
            while True:
                try:
                    got.append(b.recv(70000))
                except BlockingIOError:
                    break
            assert got == [w[0] + p for w, p in zip(want, ps)]
            n = len(which)
            assert pipe.d2h_bytes == n * min(buf, 256)
            assert pipe.desc_bytes == 3 * n + 4 * nf + 4 * ((n + 63) // 64)
            assert pipe.h2d_bytes == (int(idx.max()) + 1 - int(idx.min())) * buf
            return idx, first

        idx1, first1 = batch(first_b)
        assert np.unique(idx1).size == idx1.size == need and pipe.free_bufs == 4
        with pytest.raises(ValueError):
            pipe.alloc([40] * 3, [1000] * 3)                         # more buffers than are free
        # every other datagram of the first batch is released, the rest stay held across the next call
        gone = np.concatenate([idx1[first1[i]:first1[i + 1]] for i in range(len(first_b)) if i % 2 == 0])
        held = np.concatenate([idx1[first1[i]:first1[i + 1]] for i in range(len(first_b)) if i % 2])
        pipe.release(gone)
        with pytest.raises(ValueError):
            pipe.release(gone[:1])                                   # not held any more
        before = pipe.host.array.reshape(-1, buf)[held].copy()
        idx2, _ = batch(second_b)
        assert set(idx2.tolist()) & set(gone.tolist()) and not set(idx2.tolist()) & set(held.tolist())
        assert np.array_equal(pipe.host.array.reshape(-1, buf)[held], before)          # held buffers intact,
        assert np.array_equal(pipe.d_pool.cpu().numpy().reshape(-1, buf)[held], before)  # on the device too
    finally:
        a.close()
        b.close()
        pipe.close()
