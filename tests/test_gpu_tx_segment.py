"""TCP segmentation offload (rns_tx_segment_dev / batch.tx_segment) on the GPU.  One checker for every
case: the flows are laid into an arena of random bytes, the entry runs, and every arena byte and every
status is compared with (a) Oracle.tx_chain_fill on a host copy that holds the heads
tx_segment_helper builds field by field from the templates, over the chains of its own numpy
expansion, and (b) rns_tx_fill_chain_dev on a second device copy holding the same heads."""
import socket
import threading

import numpy as np
import pytest
import torch

from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import tx_fill_chain, tx_segment
from rustnetworkstack_amd.pipeline import TxSegmentPipeline
from tx_segment_helper import Flow, data_bytes, datagrams, expected, lay, template, with_heads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAL = _lib.RNS_TX_MALFORMED
V4, V6 = _lib.RNS_TX_IP_FILLED | _lib.RNS_TX_L4_FILLED, _lib.RNS_TX_L4_FILLED


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


def run(d_arena, L, base=0, **kw):
    st = tx_segment(d_arena, dev(L.tmpl, np.uint8), dev(L.hl, np.uint8), dev(L.po + np.uint64(base), np.int64),
                    dev(L.pl, np.int32), dev(L.mss, np.int16), dev(L.ho + np.uint64(base), np.int64),
                    dev(L.seg_first, np.int32), dev(L.blk_flow, np.int32), L.n_seg, **kw)
    torch.cuda.synchronize()
    return st


def check(oracle, L, twice=False):
    """The checker.  Returns (the arena after the call, the statuses)."""
    want, want_st, (off, ln, first, seg) = expected(oracle, L)
    d_arena = torch.from_numpy(L.arena).to(DEV)
    st = run(d_arena, L)
    if twice:
        once = d_arena.cpu().numpy()
        st2 = run(d_arena, L)
        same(d_arena.cpu().numpy(), once, st2.cpu().numpy(), st.cpu().numpy(), "the second run")
    got, got_st = d_arena.cpu().numpy(), st.cpu().numpy()
    same(got, want, got_st, want_st, "oracle")
    d_csr = torch.from_numpy(with_heads(L)).to(DEV)
    st_csr = tx_fill_chain(d_csr, dev(off, np.int64), dev(ln, np.int32), dev(first, np.int32))
    torch.cuda.synchronize()
    same(got, d_csr.cpu().numpy(), got_st[seg], st_csr.cpu().numpy(), "tx_fill_chain")
    return got, got_st


TEMPLATES = {"v4": dict(), "v6": dict(v6=True), "v4opt52": dict(opts=12), "v6opt72": dict(v6=True, opts=12),
             "v4opt72": dict(opts=32)}


def flow(kind, n, mss, align=0, salt=0, **kw):
    return Flow(template(**TEMPLATES[kind], **kw), data_bytes(0x5E6 + 131 * n + mss + salt, n), mss, align=align)


# 1. length edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v4", "v6"])
@pytest.mark.parametrize("mss", [1, 2, 15, 16, 17, 537, 1459, 1460])
def test_length_edges(oracle, mss, kind):
    lens = [1, mss - 1, mss, mss + 1, 2 * mss, 44 * mss + 7]
    flows = [flow(kind, n, mss, align=(5 * i + mss) % 16, salt=i) for i, n in enumerate(lens)]
    _, st = check(oracle, lay(flows, head_align=mss % 4, seed=mss))
    assert (st == (V4 if kind == "v4" else V6)).all()


# 2. alignments, head kinds ----------------------------------------------------------------------
@pytest.mark.parametrize("head_align", [0, 1, 2, 3, 7, 15])
def test_alignments_and_head_kinds(oracle, head_align):
    kinds = list(TEMPLATES)
    flows = [flow(kinds[a % len(kinds)], 2 * 537 + 1 + a, 537 if a % 2 else 536, align=a) for a in range(16)]
    L = lay(flows, head_align=head_align, seed=head_align)
    assert head_align % 2 == 0 or (L.ho % 2 == 1).any()
    assert sorted(set((L.po % 16).tolist())) == list(range(16)) and set(L.hl.tolist()) == {40, 52, 60, 72}
    _, st = check(oracle, L)
    assert set(st.tolist()) == {V4, V6}


# 3. id and seq wrap -----------------------------------------------------------------------------
def test_id_and_seq_wrap(oracle):
    flows = [flow("v4", 5 * 300, 300, seq=0xFFFFFF00, ident=0xFFFE), flow("v6", 3 * 200, 200, align=3, seq=0xFFFFFF00),
             flow("v4opt52", 70, 1, align=9, seq=0xFFFFFFFE, ident=0xFFC0)]
    got, st = check(oracle, lay(flows, head_align=2))
    assert (st != MAL).all()


# 4. wave boundaries inside and between flows ------------------------------------------------------
@pytest.mark.parametrize("shape", ["70_segments_mss1", "130_one_segment_flows", "zero_length_between"])
def test_wave_boundaries(oracle, shape):
    if shape == "70_segments_mss1":
        flows = [flow("v4", 3, 2), flow("v4", 70, 1, align=1), flow("v6", 70, 1, align=6), flow("v4", 9, 4)]
    elif shape == "130_one_segment_flows":
        flows = [flow("v4" if i % 3 else "v6", 1 + (37 * i) % 600, 600, align=i % 16, salt=i) for i in range(130)]
    else:
        flows = []
        for i in range(40):
            flows += [flow("v4", 0, 100), flow("v4opt52", 1 + 97 * i % 500, 128, align=i % 16, salt=i), flow("v6", 0, 0)]
        flows = [flow("v4", 0, 7)] * 70 + flows + [flow("v4", 0, 7)] * 3   # more empty flows than a search chunk
    _, st = check(oracle, lay(flows, head_align=1, seed=len(flows)))
    assert (st != MAL).all()


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 191, 193])
def test_segment_counts(oracle, n):
    flows = [flow("v4", 0, 16), flow("v4", 16 * n - 5, 16, align=n % 16)]
    _, st = check(oracle, lay(flows, seed=n))
    assert st.size == n and (st == V4).all()
    flows = [flow("v4", 20 * (n - 40), 20, align=3), flow("v6", 33 * 40, 33, align=8)]   # the total, in two flows
    _, st = check(oracle, lay(flows, head_align=3, seed=n))
    assert st.size == n


# 5. malformed flows between good neighbours -------------------------------------------------------
def patched(t, at, val):
    b = bytearray(t)
    b[at] = val
    return bytes(b)


MALFORMED = ["bad_version", "ihl6", "protocol17", "hl_not_iphdr_plus_doff", "v6_next_header", "mss0", "hl_plus_mss",
             "wrong_count_more", "wrong_count_fewer", "data_past_arena", "heads_past_arena", "hl_past_stride"]


@pytest.mark.parametrize("kind", MALFORMED)
def test_malformed_flow_between_good_neighbours(oracle, kind):
    t, d = template(), data_bytes(0xBAD, 300)
    bad = {
        "bad_version": lambda: Flow(patched(t, 0, 0x55), d, 100, bad=True),
        "ihl6": lambda: Flow(patched(t, 0, 0x46), d, 100, bad=True),
        "protocol17": lambda: Flow(patched(t, 9, 17), d, 100, bad=True),
        "hl_not_iphdr_plus_doff": lambda: Flow(patched(t, 32, 0x60), d, 100, bad=True),
        "v6_next_header": lambda: Flow(patched(template(v6=True), 6, 17), d, 100, bad=True),
        "mss0": lambda: Flow(t, d, 0, nseg=2, bad=True),
        "hl_plus_mss": lambda: Flow(t, d, 65535 - 39, bad=True),
        "wrong_count_more": lambda: Flow(t, d, 100, nseg=4, bad=True),
        "wrong_count_fewer": lambda: Flow(t, d, 100, nseg=2, bad=True),
        "data_past_arena": lambda: Flow(t, d, 100, bad=True),
        "heads_past_arena": lambda: Flow(t, d, 100, bad=True),
        "hl_past_stride": lambda: Flow(template(opts=40), d, 100, bad=True),
    }[kind]()
    before = [flow("v4", 61 * 50 + 1, 50, align=5), flow("v6", 7, 9, align=11)]   # the bad flow straddles a wave edge
    after = [flow("v4opt52", 300, 100, align=2), flow("v4", 64 * 8, 8)]
    L = lay(before + [bad] + after, head_align=1, seed=len(kind), stride=72 if kind == "hl_past_stride" else None)
    size = L.arena.size
    if kind == "data_past_arena":
        L.po[2] = size - 299
    if kind == "heads_past_arena":
        L.ho[2] = size - 3 * 40 + 1
    if kind == "hl_plus_mss":
        assert int(L.hl[2]) + int(L.mss[2]) == 65536
    _, st = check(oracle, L)
    s0, s1 = int(L.seg_first[2]), int(L.seg_first[3])
    assert s1 > s0 and (st[s0:s1] == MAL).all() and (st[:s0] != MAL).all() and (st[s1:] != MAL).all()


def test_segments_no_flow_covers(oracle):
    """n_seg past the flows' total, and a blk_flow entry that points at the wrong flow: MALFORMED
    segments, no byte written for them, the others exact."""
    flows = [flow("v4", 100 * 10, 10, align=1), flow("v6", 40 * 30, 30, align=7)]
    L = lay(flows, head_align=3)
    want, want_st, _ = expected(oracle, L)
    d_arena = torch.from_numpy(L.arena).to(DEV)
    L.n_seg += 70                                                  # two more blocks, covered by no flow
    L.blk_flow = np.concatenate([L.blk_flow, [1, 7]]).astype(np.uint32)
    st = run(d_arena, L).cpu().numpy()
    same(d_arena.cpu().numpy(), want, st, np.concatenate([want_st, np.full(70, MAL, dtype=np.uint8)]), "past the flows")
    d_arena = torch.from_numpy(L.arena).to(DEV)
    L.blk_flow[1] = 1                                              # segment 64 lies in flow 0: the search starts past it
    st = run(d_arena, L).cpu().numpy()
    assert (st[64:100] == MAL).all() and np.array_equal(st[:64], want_st[:64]) and np.array_equal(st[100:140], want_st[100:])
    got = d_arena.cpu().numpy()
    lo, hi = int(L.ho[0]) + 64 * 40, int(L.ho[0]) + 100 * 40
    assert np.array_equal(got[lo:hi], L.arena[lo:hi])              # untouched
    assert np.array_equal(got[:lo], want[:lo]) and np.array_equal(got[hi:], want[hi:])


# 6. a second run, a mixed batch -------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    kinds = list(TEMPLATES)
    flows, total, i = [], 0, 0
    while total < 3000:
        mss = [1460, 537, 1, 16, 1459, 88][i % 6]
        nseg = [44, 1, 70, 3, 2, 0, 17][i % 7]
        n = max(nseg * mss - (i % mss if nseg else 0), 0)
        flows.append(flow(kinds[i % len(kinds)], n, mss, align=(7 * i) % 16, salt=i, seq=0xFFFFF000 + 977 * i, ident=0xFF00 + 31 * i))
        total += flows[-1].nseg
        i += 1
    return lay(flows, head_align=1, seed=0x3000)


def test_mixed_segments_and_a_second_run(oracle, mixed):
    assert mixed.n_seg >= 3000
    _, st = check(oracle, mixed, twice=True)
    assert set(st.tolist()) == {V4, V6}


# 7. behind 4 GiB: the 64-bit instantiations --------------------------------------------------------
def test_flows_behind_4gib(oracle, mixed):
    line = 1 << 32
    want, want_st, _ = expected(oracle, mixed)
    size = mixed.arena.size
    big = torch.empty(line + (64 << 20), dtype=torch.uint8, device=DEV)
    try:
        for name, base in (("straddling", (line - size // 2) & ~15), ("above", line + 4096 + 16)):
            big[base:base + size] = torch.from_numpy(mixed.arena).to(DEV)
            st = run(big, mixed, base=base)
            same(big[base:base + size].cpu().numpy(), want, st.cpu().numpy(), want_st, name)
    finally:
        del big
        torch.cuda.empty_cache()


# 8. wrapper checks and the optional status --------------------------------------------------------
def test_optional_outputs(oracle):
    L = lay([flow("v4", 3000, 1460, align=3), flow("v6", 100, 7)], head_align=1)
    want, want_st, _ = expected(oracle, L)
    d_arena = torch.from_numpy(L.arena).to(DEV)
    args = (d_arena, dev(L.tmpl, np.uint8), dev(L.hl, np.uint8), dev(L.po, np.int64), dev(L.pl, np.int32),
            dev(L.mss, np.int16), dev(L.ho, np.int64), dev(L.seg_first, np.int32), dev(L.blk_flow, np.int32), L.n_seg)
    lib = _lib.load()
    with torch.cuda.device(DEV):                                   # d_status NULL
        assert lib.rns_tx_segment_dev(d_arena.data_ptr(), d_arena.numel(), args[1].data_ptr(), L.stride,
                                      *[a.data_ptr() for a in args[2:9]], len(L.flows), L.n_seg, None,
                                      torch.cuda.current_stream().cuda_stream) == _lib.RNS_OK
    torch.cuda.synchronize()
    assert np.array_equal(d_arena.cpu().numpy(), want)
    status = torch.full((L.n_seg,), 0xEE, dtype=torch.uint8, device=DEV)
    out = tx_segment(*args, status=status)
    torch.cuda.synchronize()
    assert out is status and np.array_equal(status.cpu().numpy(), want_st)
    with pytest.raises(ValueError):
        tx_segment(*args, status=torch.zeros(L.n_seg + 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        tx_segment(*args[:8], args[8][:0], L.n_seg)                # too few block entries
    with pytest.raises(ValueError):
        tx_segment(*args[:2], args[2][:-1], *args[3:])             # one head length short
    with pytest.raises(TypeError):
        tx_segment(*args[:3], args[3].to(torch.int32), *args[4:])
    with pytest.raises(ValueError, match="no CPU fallback"):
        tx_segment(args[0], args[1].cpu(), *args[2:])


# 9. the pipeline ----------------------------------------------------------------------------------
def test_pipeline(oracle):
    kinds = list(TEMPLATES)
    flows = [flow(kinds[i % len(kinds)], [44 * 1460 + 7, 1, 537, 3 * 1459, 70][i % 5], [1460, 9, 537, 1459, 1][i % 5],
                  align=(5 * i) % 16, salt=i, seq=0xFFFFFF00 + i, ident=0xFFF0 + i) for i in range(16)]
    L = lay(flows)
    want, want_st, ch = expected(oracle, L)
    expect = datagrams(want, ch)
    assert 300 <= len(expect) <= 800
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    pay_bytes = int(L.ho[0])
    pipe = TxSegmentPipeline(pay_bytes=pay_bytes, max_flows=16, max_segs=1024, tmpl_stride=100)
    try:
        a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 8 << 20)
        b.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 8 << 20)
        b.settimeout(20)
        got = []

        def drain():                                               # the far end reads while the pipeline sends
            try:
                while len(got) < len(expect):
                    got.append(b.recv(70000))
            except socket.timeout:
                pass

        t = threading.Thread(target=drain)
        t.start()
        pipe.host.array[:pay_bytes] = L.arena[:pay_bytes]
        st = pipe.send(a.fileno(), [f.tmpl for f in flows], L.po, L.pl, L.mss)
        t.join(timeout=60)
        assert np.array_equal(st, want_st)
        assert got == expect
        assert pipe.d2h_bytes == sum(f.nseg * f.hl for f in flows)
        assert pipe.desc_bytes == 27 * len(flows) + 4 * ((L.n_seg + 63) // 64)
        with pytest.raises(ValueError):
            pipe.send(a.fileno(), [flows[0].tmpl], [pay_bytes - 10], [100], [50])   # data outside the payload region
    finally:
        a.close()
        b.close()
        pipe.close()
