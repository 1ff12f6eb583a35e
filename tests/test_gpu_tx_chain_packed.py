"""Transmit finalize of [head, payload] chains over COMPACT descriptors on the GPU
(rns_tx_fill_chain_packed_dev: the transmit-rows kernel's compact mode — u8 head lengths, u16
payload lengths, one head offset and one payload offset per 64 datagrams) against
oracle.tx_chain_fill_ref, the reference's transmit path (tcp.rs:957-973, udp.rs:151-171,
icmp.rs:87-112, ip.rs:140-160 over alloc_header's head fragment, buf.rs:262-291), and against
rns_tx_fill_chain_dev on the equivalent CSR descriptors.  Every arena byte after the finalize and
the status per datagram are compared."""
import socket
import threading

import numpy as np
import pytest
import torch

from oracle import oracle as O
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import (csum_batch, csum_chain, fill_splitmix64, tx_chain_packed_layout,
                                        tx_fill_chain, tx_fill_chain_packed)
from test_gpu_tx import outgoing
from test_gpu_tx_chain import l4_header_len
from test_gpu_tx_packed import edge_datagrams
from test_rx_oracle import L4, R4, ipv4, tcp_seg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILLED = _lib.RNS_TX_IP_FILLED | _lib.RNS_TX_L4_FILLED


def dev(a, view):
    return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def cut(pkts, head_only=lambda i: False):
    """[head, payload] per datagram: the head is the IP + L4 headers (what alloc_header put into
    the head fragment); head_only(i) keeps the whole datagram's first header bytes only."""
    heads, pays = [], []
    for i, p in enumerate(pkts):
        hl = min(len(p), l4_header_len(p))
        heads.append(p[:hl])
        pays.append(b"" if head_only(i) else p[hl:])
    return heads, pays


class Plan:
    """A compact layout: block b's heads back to back from hblk[b], its payloads at
    2^align_log2 steps from pblk[b]; `order` = the blocks' order in memory (any permutation)."""

    def __init__(self, heads, pays, head_first=3, pay_first=None, align_log2=4, order=None, pay_shift=0):
        n = len(heads)
        self.heads, self.pays, self.align_log2 = heads, pays, align_log2
        assert all(len(h) <= 255 for h in heads) and all(len(p) <= 65535 for p in pays)
        self.hl = np.array([len(h) for h in heads], dtype=np.uint8)
        self.pl = np.array([len(p) for p in pays], dtype=np.uint16)
        nb = (n + 63) // 64
        order = list(range(nb)) if order is None else order
        if pay_first is None:
            pay_first = ((head_first + int(self.hl.sum()) + 4096) & ~15) + pay_shift
        self.hblk, self.pblk = np.zeros(nb, np.uint64), np.zeros(nb, np.uint64)
        self.hoff, self.poff = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        hpos, ppos = head_first, pay_first
        for b in order:
            s = slice(64 * b, min(64 * b + 64, n))
            hb, pb, ho, po, hpos, ppos = tx_chain_packed_layout(self.hl[s], self.pl[s], align_log2, hpos, ppos)
            self.hblk[b], self.pblk[b] = hb[0], pb[0]
            self.hoff[s], self.poff[s] = ho, po
        assert hpos <= pay_first  # the header region ends below the payload region
        self.end = max(hpos, ppos)

    def place(self, arena, base=0):
        for h, p, ho, po in zip(self.heads, self.pays, self.hoff.tolist(), self.poff.tolist()):
            arena[ho - base:ho - base + len(h)] = np.frombuffer(h, dtype=np.uint8)
            arena[po - base:po - base + len(p)] = np.frombuffer(p, dtype=np.uint8)

    def expected(self, oracle, arena, base=0):
        """The arena and the statuses after the reference's transmit path (computed once per plan)."""
        want = arena.copy()
        st = np.zeros(len(self.heads), dtype=np.uint8)
        for i, (h, p, ho) in enumerate(zip(self.heads, self.pays, self.hoff.tolist())):
            hh, st[i] = O.tx_chain_fill_ref([h] + ([p] if p else []), ones_comp=oracle.compute_ones_comp)
            want[ho - base:ho - base + len(hh)] = np.frombuffer(hh, dtype=np.uint8)
        return want, st

    def csr(self):
        """The same chains as rns_tx_fill_chain_dev's descriptors."""
        has = self.pl > 0
        cnt = 1 + has.astype(np.int64)
        first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        off, ln = np.zeros(int(first[-1]), np.uint64), np.zeros(int(first[-1]), np.uint32)
        f0 = first[:-1].astype(np.int64)
        off[f0], ln[f0] = self.hoff, self.hl
        off[f0[has] + 1], ln[f0[has] + 1] = self.poff[has], self.pl[has]
        return off, ln, first

    def run(self, arena, base_shift=0):
        big = torch.from_numpy(np.concatenate([np.zeros(base_shift, np.uint8), arena])).to(DEV)
        a = big[base_shift:]
        st = tx_fill_chain_packed(a, dev(self.hblk, np.int64), dev(self.hl, np.uint8), dev(self.pblk, np.int64),
                                  dev(self.pl, np.int16), pay_align_log2=self.align_log2)
        torch.cuda.synchronize()
        return a.cpu().numpy(), st.cpu().numpy()

    def run_csr(self, arena, base_shift=0):
        off, ln, first = self.csr()
        big = torch.from_numpy(np.concatenate([np.zeros(base_shift, np.uint8), arena])).to(DEV)
        a = big[base_shift:]
        st = tx_fill_chain(a, dev(off, np.int64), dev(ln, np.int32), dev(first, np.int32))
        torch.cuda.synchronize()
        return a.cpu().numpy(), st.cpu().numpy()


def same(got, want, got_st, want_st, what):
    bad = np.flatnonzero(got_st != want_st)
    assert bad.size == 0, (what, [(int(i), int(got_st[i]), int(want_st[i])) for i in bad[:5]])
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (what, [(int(d), int(got[d]), int(want[d])) for d in diff[:8]])


def check(oracle, plan, seed, base_shift=0):
    """The checker: compact finalize == the oracle == the CSR finalize, bytes and statuses."""
    arena = O.splitmix64_bytes(seed ^ 0xC0DE, plan.end + 64)
    plan.place(arena)
    want, want_st = plan.expected(oracle, arena)
    got, got_st = plan.run(arena, base_shift)
    same(got, want, got_st, want_st, "oracle")
    got2, got2_st = plan.run_csr(arena, base_shift)
    same(got, got2, got_st, got2_st, "csr")
    return want_st


@pytest.mark.parametrize("base_shift", [0, 5])
def test_mixed_traffic_matches_reference_and_csr(oracle, base_shift):
    """TCP / UDP / ICMP over IPv4 and IPv6, options, unknown protocols, short segments, garbage,
    empty: heads from an odd offset, payloads 16-byte aligned; then an unaligned arena base (every
    payload block unaligned in memory: the exact loop)."""
    pkts = outgoing(5000, 0xC9A1 + base_shift)
    st = check(oracle, Plan(*cut(pkts), head_first=3), 0x51 + base_shift, base_shift)
    assert len(set(st.tolist())) >= 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("mode", ["full", "alternate", "block_head_only"])
def test_wave_and_block_edges(oracle, n, mode):
    """1500-byte IPv4/TCP datagrams at the wave and block edges; head-only and full datagrams
    alternating; every datagram of the first 64-block head-only (a wave with no payload region)."""
    pkts = [ipv4(6, tcp_seg(L4, R4, O.splitmix64_bytes(n * 1000 + k, 1460).tobytes())) for k in range(n)]
    ho = {"full": lambda i: False, "alternate": lambda i: i % 2 == 1, "block_head_only": lambda i: i < 64}[mode]
    st = check(oracle, Plan(*cut(pkts, ho), head_first=0), 0x60 + n)
    assert (st == FILLED).all()


def test_edge_datagrams(oracle):
    """IHL 5..15 against every field position, IPv6 short segments, 65535-byte datagrams,
    malformed and empty ones; 80-byte heads at an unaligned start force the exact loop on their
    waves.  A datagram the form cannot describe (head > 255 B, payload > 65535 B) is dropped."""
    pkts = edge_datagrams()
    heads, pays = cut(pkts)
    keep = [i for i in range(len(pkts)) if len(heads[i]) <= 255 and len(pays[i]) <= 65535]
    assert len(pkts) - len(keep) <= len(pkts) // 20
    assert max(len(heads[i]) for i in keep) == 80
    check(oracle, Plan([heads[i] for i in keep], [pays[i] for i in keep], head_first=3), 0x22)
    check(oracle, Plan([heads[i] for i in keep], [pays[i] for i in keep], head_first=0, align_log2=9), 0x23)


def test_fallback_equivalence(oracle):
    """The same 300 datagrams through the rows (16-aligned payload blocks) and through the exact
    loop (the payload region moved by 8 bytes): both equal the oracle byte for byte."""
    pkts = outgoing(300, 0xFA11)
    heads, pays = cut(pkts)
    rows = Plan(heads, pays, head_first=0)
    st_rows = check(oracle, rows, 0x70)
    assert not (rows.pblk & np.uint64(15)).any()
    loop = Plan(heads, pays, head_first=0, pay_shift=8)
    st_loop = check(oracle, loop, 0x70)
    assert ((loop.pblk & np.uint64(15)) == 8).all()
    assert np.array_equal(st_rows, st_loop)


def test_independent_blocks(oracle):
    """The blocks' offsets are independent: blocks 1 and 2 swapped in memory (not ascending)."""
    pkts = outgoing(64 * 4 + 20, 0xB10C)
    plan = Plan(*cut(pkts), head_first=5, order=[0, 2, 1, 3, 4])
    assert plan.hblk[2] < plan.hblk[1] and plan.pblk[2] < plan.pblk[1]
    check(oracle, plan, 0x80)


def test_rejects(oracle):
    """A block whose heads lie past the arena, a payload that runs past the arena's end, a head of
    length 0 with and without a payload, a 19-byte IPv4 head: RNS_TX_MALFORMED and not a byte
    written; their neighbours in the same wave are finalized as the oracle does."""
    n = 64 * 3
    pkts = [ipv4(6, tcp_seg(L4, R4, O.splitmix64_bytes(k, 300 + k).tobytes())) for k in range(n)]
    heads, pays = cut(pkts)
    heads[5], pays[5] = b"", b""                  # head_len == 0, head only
    heads[6] = b""                                # head_len == 0 with a payload
    heads[7], pays[7] = pkts[7][:19], pkts[7][19:]  # the head does not hold the IPv4 header
    plan = Plan(heads, pays, head_first=3)
    # the arena ends inside the payload of datagram n - 3: it and the two behind it run past the end
    bytes_ = int(plan.poff[n - 3]) + 100
    arena = O.splitmix64_bytes(0xBAD, bytes_)
    for i in range(n - 3):
        arena[int(plan.hoff[i]):int(plan.hoff[i]) + len(heads[i])] = np.frombuffer(heads[i], dtype=np.uint8)
        arena[int(plan.poff[i]):int(plan.poff[i]) + len(pays[i])] = np.frombuffer(pays[i], dtype=np.uint8)
    for i in range(n - 3, n):
        arena[int(plan.hoff[i]):int(plan.hoff[i]) + len(heads[i])] = np.frombuffer(heads[i], dtype=np.uint8)
    plan.hblk[1] = bytes_ + 1000                  # block 1: every head past the arena
    rejected = [5, 6, 7] + list(range(64, 128)) + [n - 3, n - 2, n - 1]
    want = arena.copy()
    want_st = np.full(n, _lib.RNS_TX_MALFORMED, dtype=np.uint8)
    for i in sorted(set(range(n)) - set(rejected)):
        hh, want_st[i] = O.tx_chain_fill_ref([heads[i], pays[i]], ones_comp=oracle.compute_ones_comp)
        want[int(plan.hoff[i]):int(plan.hoff[i]) + len(hh)] = np.frombuffer(hh, dtype=np.uint8)
    assert (want_st[[4, 8, 0, 63, 128, n - 4]] == FILLED).all()
    assert O.tx_chain_fill_ref([heads[7], pays[7]])[1] == O.TX_MALFORMED
    got, got_st = plan.run(arena)
    same(got, want, got_st, want_st, "oracle")
    # the wrapper's own checks
    a = torch.from_numpy(arena).to(DEV)
    d = (dev(plan.hblk, np.int64), dev(plan.hl, np.uint8), dev(plan.pblk, np.int64), dev(plan.pl, np.int16))
    with pytest.raises(ValueError):
        tx_fill_chain_packed(a, d[0], d[1][:-1], d[2], d[3])
    with pytest.raises(ValueError):
        tx_fill_chain_packed(a, d[0], d[1], d[2], d[3][:-1])
    with pytest.raises(ValueError):
        tx_fill_chain_packed(a, d[0][:2], d[1], d[2], d[3])
    with pytest.raises(ValueError):
        tx_fill_chain_packed(a, *d, status=torch.empty(n - 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        tx_fill_chain_packed(a, *d, pay_align_log2=3)
    assert torch.equal(a.cpu(), torch.from_numpy(arena))


def test_big_arena(oracle):
    """The BUF=false instantiation: about 2000 datagrams of every kind in three windows of an arena
    past 4 GiB (near its start, across the 4 GiB line, ending at its last bytes); every window
    byte and status against the oracle."""
    from test_gpu_big_arena import FOUR_G, NBYTES, SPAN, Windows
    arena = torch.empty(NBYTES, dtype=torch.uint8, device=DEV)
    try:
        fill_splitmix64(arena, 0xB16B)
        assert arena.numel() >= FOUR_G
        win = Windows(arena)
        inp = [h.copy() for h in win.orig]
        want, plans, want_st = [], [], []
        for k in range(3):
            pk = outgoing(640 + (45 if k == 2 else 0), 0x8D0 + k)   # blocks never span windows
            heads, pays = cut(pk)
            size = Plan(heads, pays, head_first=3).end + 64
            assert size <= SPAN
            rel = (0, (SPAN // 2 - size // 2) & ~15, (SPAN - size) & ~15)[k]
            plan = Plan(heads, pays, head_first=win.starts[k] + rel + 3)
            assert plan.end <= win.starts[k] + SPAN
            plan.place(inp[k], base=win.starts[k])
            w, st = plan.expected(oracle, inp[k], base=win.starts[k])
            want.append(w)
            want_st.append(st)
            plans.append(plan)
        assert plans[1].hoff[0] < FOUR_G < plans[1].poff[-1]
        win.write(inp)
        st = tx_fill_chain_packed(arena, dev(np.concatenate([p.hblk for p in plans]), np.int64),
                                  dev(np.concatenate([p.hl for p in plans]), np.uint8),
                                  dev(np.concatenate([p.pblk for p in plans]), np.int64),
                                  dev(np.concatenate([p.pl for p in plans]), np.int16))
        torch.cuda.synchronize()
        same(np.concatenate(win.snapshot()), np.concatenate(want), st.cpu().numpy(), np.concatenate(want_st), "oracle")
    finally:
        del arena
        torch.cuda.empty_cache()


def test_idempotent_and_receive_side():
    """Finalizing twice stores the same bytes; after one finalize of 3000 IPv4/TCP datagrams every
    IP header verifies to 0 and every [TCP header, payload] chain verifies to 0 with the
    receiver's pseudo-header (tcp.rs:838-850), and the heads equal the whole-datagram finalize."""
    pkts = [ipv4(6, tcp_seg(R4, L4, O.splitmix64_bytes(k, 1 + k % 1459).tobytes())) for k in range(3000)]
    plan = Plan(*cut(pkts), head_first=3)
    arena = O.splitmix64_bytes(0x33, plan.end + 64)
    plan.place(arena)
    a = torch.from_numpy(arena).to(DEV)
    d = (dev(plan.hblk, np.int64), dev(plan.hl, np.uint8), dev(plan.pblk, np.int64), dev(plan.pl, np.int16))
    st = tx_fill_chain_packed(a, *d)
    assert int((st != FILLED).sum().item()) == 0
    once = a.clone()
    st2 = tx_fill_chain_packed(a, *d)
    assert torch.equal(a, once) and torch.equal(st, st2)
    got = a.cpu().numpy()
    for i in range(0, 3000, 8):
        assert bytes(got[int(plan.hoff[i]):int(plan.hoff[i]) + 40]) == O.tx_fill_ref(pkts[i])[0][:40]
    ip = csum_batch(a, dev(plan.hoff, np.int64), dev(np.full(3000, 20, np.uint32), np.int32), complement=True)
    assert int(ip.view(torch.int16).ne(0).sum().item()) == 0
    off, ln, first = plan.csr()
    hidx = first[:-1].astype(np.int64)
    off[hidx] += 20
    ln[hidx] -= 20
    seeds = np.array([O.pseudo_header_py(R4, L4, len(p) - 20, 6) for p in pkts], dtype=np.uint16)
    l4 = csum_chain(a, dev(off, np.int64), dev(ln, np.int32), dev(first, np.int32), dev(seeds, np.int16),
                    complement=True)
    assert int(l4.view(torch.int16).ne(0).sum().item()) == 0


def test_pipeline_compact_and_csr_routes(oracle):
    """TxChainPipeline(compact=True) over a socketpair: a packed batch takes the compact route
    (3 B per datagram + 16 B per 64 of descriptors to the device), a batch with one displaced
    payload the CSR route; the far end receives the oracle-finalized datagrams either way."""
    from rustnetworkstack_amd.batch import recv_batch
    from rustnetworkstack_amd.pipeline import TxChainPipeline
    pkts = [p for p in outgoing(700, 0x7C4B) if 0 < len(p) <= 2048][:500]
    heads = [p[:min(len(p), max(1, l4_header_len(p)), TxChainPipeline.HEAD_MAX)] for p in pkts]  # (garbage: IHL 0)
    want = []
    for p, h in zip(pkts, heads):
        hh, st = O.tx_chain_fill_ref([h] + ([p[len(h):]] if len(p) > len(h) else []), ones_comp=oracle.compute_ones_comp)
        want.append((hh + p[len(h):], st))
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_SEQPACKET)
    for s_, opt in ((a, socket.SO_SNDBUF), (b, socket.SO_RCVBUF)):
        s_.setsockopt(socket.SOL_SOCKET, opt, 32 << 20)
    received = []

    def drain():
        buf = np.empty(2048 * 1024, dtype=np.uint8)
        while len(received) < 2 * len(pkts):
            off, ln = recv_batch(b.fileno(), buf, 2048, 1024, timeout_ms=5000)
            if ln.shape[0] == 0:
                return
            received.extend(buf[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, ln))

    t = threading.Thread(target=drain)
    t.start()
    pipe = TxChainPipeline(device=0, max_pkts=4096, compact=True)
    n = len(pkts)
    forms, desc, statuses = [], [], []
    for displaced in (False, True):
        hreg, preg = pipe.heads(), pipe.payloads()
        hl, po, pl = [], [], []
        hpos = ppos = 0
        for i in range(n):
            h, body = heads[i], pkts[i][len(heads[i]):]
            if displaced and i == 300:
                ppos += 16                       # one payload a chunk later than the packed layout
            hreg[hpos:hpos + len(h)] = np.frombuffer(h, dtype=np.uint8)
            preg[ppos:ppos + len(body)] = np.frombuffer(body, dtype=np.uint8)
            hl.append(len(h))
            po.append(ppos)
            pl.append(len(body))
            hpos += len(h)
            ppos = (ppos + len(body) + 15) & ~15
        statuses.append(pipe.send(a.fileno(), np.array(hl), np.array(po), np.array(pl)))
        forms.append(pipe.last_form)
        desc.append(pipe.last_desc_bytes)
    t.join(timeout=60)
    pipe.close()
    a.close()
    b.close()
    assert forms == ["compact", "csr"]
    nf = n + sum(1 for p, h in zip(pkts, heads) if len(p) > len(h))
    assert desc == [3 * n + 16 * ((n + 63) // 64), 12 * nf + 4 * (n + 1)]
    want_st = np.array([w[1] for w in want], dtype=np.uint8)
    assert np.array_equal(statuses[0], want_st) and np.array_equal(statuses[1], want_st)
    assert len(received) == 2 * n
    bad = [i for i in range(2 * n) if received[i] != want[i % n][0]]
    assert not bad, bad[:5]


@pytest.mark.parametrize("config", ["c3_1500B", "c5_imix"])
def test_workload_batch_carries_compact_descriptors(config):
    """workloads.TxChainBatch (one payload fragment) carries the compact descriptors of its arena:
    finalizing through them stores the bytes and statuses of the CSR descriptors (a 1/512 shard)."""
    from rustnetworkstack_amd.workloads import TxChainBatch
    b = TxChainBatch(config, DEV, shard=(3, 512))
    n = b.layout.n
    assert b.d_head_len8.numel() == n and b.d_pay_len16.numel() == n
    assert b.d_head_blk_off.numel() == b.d_pay_blk_off.numel() == (n + 63) // 64
    a2 = b.arena.clone()
    st = tx_fill_chain(b.arena, b.d_off, b.d_len, b.d_first, status=b.status)
    st2 = tx_fill_chain_packed(a2, b.d_head_blk_off, b.d_head_len8, b.d_pay_blk_off, b.d_pay_len16)
    assert int((st != FILLED).sum().item()) == 0
    assert torch.equal(st, st2) and torch.equal(b.arena, a2)
    assert not hasattr(TxChainBatch(config, DEV, frag=512, shard=(3, 512)), "d_head_len8")
