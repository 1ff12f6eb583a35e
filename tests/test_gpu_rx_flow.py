"""The TCP flow update and the ACK build (rns_rx_tcp_flow_update_dev / rns_tx_ack_build_dev) on the GPU,
compared record for record with the restatement in tests/rx_flow_helper.py.  Every output is
pre-filled with 0xEE between two sentinel guards, so a missing write and a stray one both show."""
import numpy as np
import pytest
import torch

from gpu_guard import DEV, FILL, Guarded
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.flow import flow_update_work, rx_tcp_flow_update, tx_ack_build
from rustnetworkstack_amd.place import meta_records, rx_flow_table, rx_tcp_place_pool
from rx_flow_helper import (ACK, FLOW, META, NONE, P_FLOW, P_TCP, PSH, RES, S_ACK, S_CONSUMED, SEG, STOP_MANY, STOP_NONE,
                            STOP_PEND, STOP_STATE, ack_heads_ref, flow_rec, metas, same_update, template, update_ref)
from rx_place_helper import L4, L6, SENTINEL, body_bytes, key_of, lay_pool, segment

pytestmark = pytest.mark.gpu
V4A, V4B = bytes([10, 1, 2, 3]), bytes([10, 9, 8, 7])
V6A = bytes.fromhex("20010db8000000000000000000000042")


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def run_update(meta, flows, pend, cap, work=None):
    """One call over host arrays: (flows_out, pend_out or None, seg, res) as numpy, guards checked."""
    meta, flows = np.asarray(meta, dtype=META).reshape(-1), np.asarray(flows, dtype=FLOW).reshape(-1)
    n, nfl = meta.size, flows.size
    o_fl, o_seg, o_res = Guarded(40 * nfl), Guarded(8 * n), Guarded(24 * nfl)
    o_pd = Guarded(8 * nfl * cap, dtype=torch.int32)
    d_pend = dev(np.asarray(pend, dtype=np.uint32)).view(torch.int32) if cap else None
    d_meta, d_flows = dev(meta), dev(flows)
    rx_tcp_flow_update(d_meta, d_flows, d_pend, pend_cap=cap, flows_out=o_fl.t, pend_out=o_pd.t if cap else None,
                       seg=o_seg.t, res=o_res.t, work=work)
    torch.cuda.synchronize()
    assert np.array_equal(d_meta.cpu().numpy().view(META), meta) and np.array_equal(d_flows.cpu().numpy().view(FLOW), flows)
    if cap:
        assert np.array_equal(d_pend.cpu().numpy().view(np.uint32), np.asarray(pend, dtype=np.uint32).reshape(-1))
    pd = o_pd.host(np.uint32).reshape(nfl, cap, 2)
    return o_fl.host(FLOW), pd if cap else None, o_seg.host(SEG), o_res.host(RES)


def check_update(meta, flows, pend, cap, **kw):
    want = update_ref(meta, flows, pend, cap, **kw)
    got = run_update(meta, flows, pend, cap)
    same_update(got, want, cap)
    return got, want


# 6. order ------------------------------------------------------------------------------------------------
def order_batch():
    """6 flows over 200 datagrams, interleaved by a seeded permutation; every flow's result depends on
    the order of its segments: out-of-order arrivals, a duplicate seq with another length, stale
    segments inside the window, and ACK numbers and windows that move with every segment."""
    rng = np.random.default_rng(61)
    per, flows = [], []
    for f in range(6):
        base = (0xFFFFF000 + 0x1000 * f * 7) & 0xFFFFFFFF
        segs, off = [], 0
        for j in range(33):
            ln = int(rng.integers(10, 50))
            segs.append(dict(flow=f, seq=(base + off) & 0xFFFFFFFF, pay_len=ln, ack=2000 + 7 * j, window=100 + j,
                             flags=ACK | PSH))
            off += ln
        for j in (3, 9, 20):                                         # out of order: swapped neighbours
            segs[j], segs[j + 1] = segs[j + 1], segs[j]
        segs[14], segs[16] = segs[16], segs[14]                     # and two places apart
        segs.insert(12, dict(segs[11], pay_len=segs[11]["pay_len"] + 5))         # a duplicate seq, longer
        segs.insert(25, dict(segs[2], ack=1990))                    # stale, inside the window
        per.append(segs[:34 if f < 2 else 33])
        flows.append(flow_rec(rcv_nxt=base, rcv_max=base, snd_una=1995, snd_nxt=4000, snd_wl1=(base - 1) & 0xFFFFFFFF,
                              delayed_acks=f % 5, ack_timer=f & 1, rq_len=100 * f))
    slots = np.repeat(np.arange(6), [len(p) for p in per])
    assert slots.size == 200
    rng.shuffle(slots)
    it = [iter(p) for p in per]
    return metas([next(it[f]) for f in slots]), np.array(flows, dtype=FLOW)


def test_order_is_the_batch_order():
    meta, flows = order_batch()
    cap = 8
    pend = np.zeros((6, cap, 2), dtype=np.uint32)
    want = update_ref(meta, flows, pend, cap)
    assert (want[3]["why"] == STOP_NONE).all() and (want[3]["consumed"] == want[3]["n_segs"]).all()
    assert want[3]["n_acks"].min() >= 5
    rev = meta.copy()
    mine = np.flatnonzero(meta["flow"] == 0)
    rev[mine] = meta[mine[::-1]]                                      # in the helper alone: flow 0's list reversed
    other = update_ref(rev, flows, pend, cap)
    assert other[0][0] != want[0][0], "the batch does not depend on the order: an unsorted walk could pass"
    got = run_update(meta, flows, pend, cap)
    same_update(got, want, cap)
    again = run_update(meta, flows, pend, cap)
    for a, b in zip(got, again):
        n_pend = got[0]["n_pend"]
        if a.dtype == np.uint32:                                      # the pending lists: their valid entries
            assert all(np.array_equal(a[f, :n_pend[f]], b[f, :n_pend[f]]) for f in range(6))
        else:
            assert a.tobytes() == b.tobytes()


# 7. list lengths, and many flows ---------------------------------------------------------------------
def test_list_lengths():
    lens = (1, 2, 63, 64, 65, 1024, 1025)
    rng = np.random.default_rng(7)
    slots = np.repeat(np.arange(len(lens)), lens)
    rng.shuffle(slots)
    n = slots.size
    assert n == 2244
    meta = np.zeros(n, dtype=META)
    meta["flow"], meta["seq"], meta["flags"], meta["tcp_hdr"], meta["ip_hdr"] = slots, 500, ACK, 20, 20
    meta["place"] = P_TCP | P_FLOW
    meta["ack"] = 1000 + np.arange(n)                                 # ascending in batch order: every one trims
    meta["window"] = np.arange(n) % 65521                             # the last segment's window is the flow's
    flows = np.array([flow_rec(rcv_nxt=500, snd_una=999, snd_nxt=99999, snd_wl1=500, snd_wl2=0)] * len(lens), dtype=FLOW)
    got, want = check_update(meta, flows, None, 0)
    res = got[3]
    assert res["n_segs"].tolist() == list(lens) and res["consumed"].tolist() == list(lens[:-1]) + [0]
    assert res["why"].tolist() == [STOP_NONE] * 6 + [STOP_MANY]
    last = np.flatnonzero(slots == 6)
    assert res[6]["stop"] == last[0] and not got[2][last].view(np.uint8).any()
    assert got[0][6].tobytes() == flows[6].tobytes()                  # nothing consumed
    for f in range(6):
        mine = np.flatnonzero(slots == f)
        assert got[0][f]["snd_wnd"] == meta["window"][mine[-1]] and got[0][f]["snd_una"] == meta["ack"][mine[-1]]


def test_many_flows_one_segment_each():
    nfl = 70000
    rng = np.random.default_rng(70)
    order = rng.permutation(nfl)
    meta = np.zeros(nfl, dtype=META)
    meta["flow"], meta["tcp_hdr"], meta["ip_hdr"], meta["place"] = order, 20, 20, P_TCP | P_FLOW | 4
    meta["seq"] = 1000 + 3 * order
    meta["pay_len"] = 1 + order % 100
    meta["flags"], meta["ack"], meta["window"] = ACK | PSH, 5000 + order % 7, order % 65536
    meta["seq"][order % 11 == 3] += 1                                 # out of order: pending
    flows = np.zeros(nfl, dtype=FLOW)
    f = np.arange(nfl)
    flows["rcv_nxt"], flows["rcv_max"], flows["state"] = 1000 + 3 * f, 1000 + 3 * f, 1
    flows["snd_una"], flows["snd_nxt"], flows["snd_wl1"] = 5000, 5005, 999
    flows["delayed_acks"], flows["ack_timer"] = f % 5, f % 2
    flows["state"][f % 13 == 5] = 3
    cap = 1
    got, want = check_update(meta, flows, np.zeros((nfl, cap, 2), dtype=np.uint32), cap)
    res = got[3]
    assert (res["n_segs"] == 1).all() and set(res["why"].tolist()) == {STOP_NONE, STOP_STATE}
    assert (got[2]["act"] & S_ACK).sum() > 5000 and got[0]["n_pend"].sum() > 5000


# 8. the edges ------------------------------------------------------------------------------------------
def test_edges_and_garbage():
    flows = np.array([flow_rec(rcv_nxt=10, n_pend=1), flow_rec(rcv_nxt=20, n_pend=2), flow_rec(rcv_nxt=30, n_pend=3)],
                     dtype=FLOW)
    cap = 2
    pend = np.array([[[100, 5], [0, 0]], [[200, 5], [300, 5]], [[1, 1], [2, 2]]], dtype=np.uint32)
    # no datagrams: a copy and a zero result
    got, _ = check_update(np.zeros(0, dtype=META), flows, pend, cap)
    assert got[0].tobytes() == flows.tobytes() and not (got[3]['n_segs'] | got[3]['consumed'] | got[3]['why']).any()
    assert (got[3]["stop"] == NONE).all() and np.array_equal(got[1][0, :1], pend[0, :1]) and np.array_equal(got[1][1], pend[1])
    # no flows: zero records
    rows = metas([dict(flow=0, seq=10, pay_len=4), dict(flow=7), dict(flow=0, place=0xFF)])
    got, _ = check_update(rows, np.zeros(0, dtype=FLOW), None, 0)
    assert not got[2].view(np.uint8).any()
    # pend_cap == 0: the first out-of-order segment stops its flow
    rows = metas([dict(flow=0, seq=10, pay_len=4), dict(flow=0, seq=99, pay_len=4), dict(flow=0, seq=14, pay_len=4)])
    got, _ = check_update(rows, np.array([flow_rec(rcv_nxt=10)], dtype=FLOW), None, 0)
    assert (got[3][0]["why"], got[3][0]["consumed"], got[3][0]["stop"]) == (STOP_PEND, 1, 1)
    # n_pend at the cap, more than the cap (garbage), flow indices past the table, every place bit
    rows = metas([dict(flow=1, seq=20, pay_len=180), dict(flow=1, seq=900, pay_len=1), dict(flow=2, seq=30, pay_len=1),
                  dict(flow=3, seq=1), dict(flow=0xFFFFFFFE, seq=1), dict(flow=0, seq=10, pay_len=90, place=0xFF),
                  dict(flow=0, seq=10, pay_len=90, place=0xF7), dict(flow=1, seq=205, pay_len=95),
                  dict(flow=1, seq=901, pay_len=1), dict(flow=1, seq=902, pay_len=1), dict(flow=1, seq=903, pay_len=1)])
    got, _ = check_update(rows, flows, pend, cap)
    assert got[3]["why"].tolist() == [5, STOP_PEND, STOP_STATE]       # flow 0: RNS_PLACE_OUTSIDE among the bits
    assert got[3][1]["consumed"] == 4 and got[0][1]["rcv_nxt"] == 305 and got[0][2].tobytes() == flows[2].tobytes()


# 9. the ACK build ------------------------------------------------------------------------------------
def ack_case():
    """Five flows (IPv4, IPv6, IPv4, a malformed IPv4 template, IPv6), 60 data segments round robin, every
    flow one short of an immediate ACK: the update gives 3 ACKs per flow."""
    srcs = (V4A, V6A, V4B, V4A, V6A)
    tm = [template(L4 if len(s) == 4 else L6, s, 80, 4000 + f, junk=0x5A + f) for f, s in enumerate(srcs)]
    bad = bytearray(tm[3])
    bad[32] = 0x60                                                    # data offset 6
    tm[3] = bytes(bad)
    hl = np.array([len(t) for t in tm], dtype=np.uint8)
    tmpl = np.full((5, 64), 0xA5, dtype=np.uint8)
    for f, t in enumerate(tm):
        tmpl[f, :len(t)] = np.frombuffer(t, dtype=np.uint8)
    flows = np.array([flow_rec(rcv_nxt=1000 * (f + 1), snd_nxt=0xFFFFFFF0 + f, delayed_acks=4, rq_len=9 * f)
                      for f in range(5)], dtype=FLOW)
    rows = [dict(flow=k % 5, seq=1000 * (k % 5 + 1) + 10 * (k // 5), pay_len=10, flags=ACK | PSH) for k in range(60)]
    rows.insert(17, dict(flow=9, seq=1))
    return metas(rows), flows, tmpl, hl, [bytes(r) for r in tmpl]


@pytest.mark.parametrize("cap_delta", [-3, 0, 5])
def test_ack_build(cap_delta):
    meta, flows, tmpl, hl, tm = ack_case()
    (fl, _, seg, res), _ = check_update(meta, flows, None, 0)
    seg = seg.copy()
    stray = 17
    seg[stray]["act"] = S_CONSUMED | S_ACK                            # an ACK flag on a datagram of no flow: ignored
    base = 0xFFFE
    heads, n4 = ack_heads_ref(meta, seg, fl, tm, hl, base)
    assert len(heads) == 15 and n4 == 9 and sum(h is None for _, h in heads) == 3
    cap = len(heads) + cap_delta
    o_out, o_src, o_len, o_n = Guarded(64 * cap), Guarded(4 * cap, dtype=torch.int32), Guarded(cap), Guarded(8, dtype=torch.int32)
    d_meta, d_seg = dev(meta), dev(seg)
    work = torch.empty(flow_update_work(meta.size, 5), dtype=torch.uint8, device=DEV)
    tx_ack_build(d_meta, d_seg, dev(fl), torch.from_numpy(tmpl).to(DEV), torch.from_numpy(hl).to(DEV), base, ack_cap=cap,
                 out=o_out.t, ack_src=o_src.t, ack_len8=o_len.t, n_acks=o_n.t, work=work)
    torch.cuda.synchronize()
    out, src = o_out.host(np.uint8).reshape(cap, 64), o_src.host(np.uint32)
    ln, n_acks = o_len.host(np.uint8), o_n.host(np.uint32)
    assert n_acks.tolist() == [15, 9]                                 # counted past the cap too
    wrote = min(cap, 15)
    assert (np.diff(src[:wrote].astype(np.int64)) > 0).all()          # batch order
    ids = []
    for k in range(wrote):
        i, head = heads[k]
        assert src[k] == i
        if head is None:
            assert ln[k] == 0 and (out[k] == FILL).all()              # keeps its slot, no byte written
            continue
        assert ln[k] == len(head) and out[k, :len(head)].tobytes() == head, k
        assert (out[k, len(head):] == FILL).all()                     # the slot's tail
        if len(head) == 40:
            ids.append(int.from_bytes(head[4:6], "big"))
    assert ids == [(base + j) & 0xFFFF for j in (0, 1, 3, 4, 6, 7)][:len(ids)] and 1 in ids   # across the wrap, IPv4 ACKs only
    assert (out[wrote:] == FILL).all() and (ln[wrote:] == FILL).all()


def test_ack_build_counts_only():
    meta, flows, tmpl, hl, tm = ack_case()
    fl, _, seg, _ = run_update(meta, flows, None, 0)
    _, _, _, n_acks = tx_ack_build(dev(meta), dev(seg), dev(fl), torch.from_numpy(tmpl).to(DEV), torch.from_numpy(hl).to(DEV),
                                   7, ack_cap=0)
    assert n_acks.cpu().tolist() == [15, 9]                           # the malformed template's ACKs count too
    _, _, _, n_acks = tx_ack_build(dev(meta[:0]), dev(seg[:0]), dev(fl), torch.from_numpy(tmpl).to(DEV),
                                   torch.from_numpy(hl).to(DEV), 7, ack_cap=0)
    assert n_acks.cpu().tolist() == [0, 0]


def scan_ack_case(n):
    """n flows with one data segment each (in reverse flow order), every flow one short of an immediate
    ACK, IPv4 and IPv6 heads alternating: every datagram is an ACK, every other one takes an id."""
    f = np.arange(n)
    tmpl = np.full((n, 64), 0xA5, dtype=np.uint8)
    t4, t6 = template(L4, V4A, 80, 4000, junk=0x5A), template(L6, V6A, 80, 4000, junk=0x3C)
    tmpl[0::2, :40], tmpl[1::2, :60] = np.frombuffer(t4, dtype=np.uint8), np.frombuffer(t6, dtype=np.uint8)
    hl = np.where(f % 2 == 0, 40, 60).astype(np.uint8)
    ports = (1024 + f % 60000).astype(">u2").view(np.uint8).reshape(n, 2)
    tmpl[0::2, 22:24], tmpl[1::2, 42:44] = ports[0::2], ports[1::2]   # the destination port
    flows = np.zeros(n, dtype=FLOW)
    flows["rcv_nxt"] = flows["rcv_max"] = 1000 + 7 * f
    flows["snd_nxt"], flows["rq_len"], flows["delayed_acks"], flows["state"] = 0xFFFF0000 + f, f % 65536, 4, 1
    meta = np.zeros(n, dtype=META)
    meta["flow"], meta["tcp_hdr"], meta["ip_hdr"], meta["place"] = f[::-1], 20, 20, P_TCP | P_FLOW | 4
    meta["seq"], meta["pay_len"], meta["flags"] = 1000 + 7 * f[::-1], 1 + f % 50, ACK | PSH
    return meta, flows, tmpl, hl


@pytest.mark.parametrize("n", [255, 256, 257, 65537])
def test_ack_build_scan_block_boundaries(n):
    """The scan under the ACK build at its block boundaries: one block short by one, one block, one more,
    and one more than 256 blocks (the middle kernel's loop runs twice).  The two scan components differ."""
    meta, flows, tmpl, hl = scan_ack_case(n)
    (fl, _, seg, _), _ = check_update(meta, flows, None, 0)
    base = 0xFFF0
    heads, n4 = ack_heads_ref(meta, seg, fl, [bytes(r) for r in tmpl], hl, base)
    assert len(heads) == n and n4 == (n + 1) // 2 and all(h is not None for _, h in heads)
    want_out = np.full((n, 64), FILL, dtype=np.uint8)
    for k, (_, head) in enumerate(heads):
        want_out[k, :len(head)] = np.frombuffer(head, dtype=np.uint8)
    want_len = np.array([len(h) for _, h in heads], dtype=np.uint8)
    assert set(want_len[:2].tolist()) == {40, 60}
    o_out, o_src, o_len, o_n = Guarded(64 * n), Guarded(4 * n, dtype=torch.int32), Guarded(n), Guarded(8, dtype=torch.int32)
    tx_ack_build(dev(meta), dev(seg), dev(fl), torch.from_numpy(tmpl).to(DEV), torch.from_numpy(hl).to(DEV), base, ack_cap=n,
                 out=o_out.t, ack_src=o_src.t, ack_len8=o_len.t, n_acks=o_n.t)
    torch.cuda.synchronize()
    assert o_n.host(np.uint32).tolist() == [n, n4]
    assert np.array_equal(o_src.host(np.uint32), np.array([i for i, _ in heads], dtype=np.uint32))
    assert np.array_equal(o_len.host(np.uint8), want_len)
    got = o_out.host(np.uint8).reshape(n, 64)
    bad = np.flatnonzero((got != want_out).any(axis=1))
    assert bad.size == 0, (bad[:5].tolist(), got[bad[0]].tobytes().hex(), want_out[bad[0]].tobytes().hex())


# 10. end to end: placement -> update -> build ---------------------------------------------------------
@pytest.mark.parametrize("buf", [128, 512])
def test_end_to_end(buf):
    rng = np.random.default_rng(buf)
    srcs = (V4A, V6A, V4B)
    keys = [key_of(s, 5000 + f, 80) for f, s in enumerate(srcs)]
    next_seq = [0xFFFFFE00, 70000, 1]
    per, win_len = [], []
    for f, s in enumerate(srcs):
        segs, off = [], 0
        for j in range(40):
            ln = int(rng.integers(1, 3 * buf // 2))
            body = body_bytes(1000 * f + j, ln)
            segs.append((segment(s, 5000 + f, 80, next_seq[f] + off, body, ack=3000 + 11 * j, window=900 + j), body))
            off += ln
        for j in (4, 17, 30):
            segs[j], segs[j + 2] = segs[j + 2], segs[j]
        del segs[36]                                                  # a hole: the tail stays pending
        per.append(segs)
        win_len.append(off + 9)
    slots = np.repeat(np.arange(3), [len(p) for p in per])
    rng.shuffle(slots)
    it = [iter(p) for p in per]
    both = [next(it[f]) for f in slots]
    pkts, bodies = [p for p, _ in both], [b for _, b in both]
    assert len(pkts) == 117
    win_off = np.concatenate([[16], 16 + np.cumsum([(w + 31) // 16 * 16 for w in win_len])[:-1]]).astype(np.uint64)
    total = int(win_off[-1]) + win_len[-1] + 16
    pool, idx, blk, len16 = lay_pool(pkts, buf, shuffled=True, seed=buf)
    d_stream = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32)).to(DEV)  # noqa: E731
    st, _, d_meta = rx_tcp_place_pool(torch.from_numpy(pool).to(DEV), i32(idx), i32(blk),
                                      torch.from_numpy(len16.view(np.int16)).to(DEV), L4, L6,
                                      torch.from_numpy(rx_flow_table(keys)).to(DEV), i32(next_seq),
                                      torch.from_numpy(win_off.view(np.int64)).to(DEV), i32(win_len), d_stream, buf_bytes=buf)
    meta = meta_records(d_meta)
    assert (meta["place"] == 7).all()
    flows = np.array([flow_rec(rcv_nxt=next_seq[f], rcv_max=next_seq[f], snd_una=2990, snd_nxt=9000 + f, snd_wl1=0)
                      for f in range(3)], dtype=FLOW)
    cap = 8
    want = update_ref(meta, flows, np.zeros((3, cap, 2), dtype=np.uint32), cap, payload=lambda i: bodies[i])
    d_fl, d_pd, d_seg, d_res = rx_tcp_flow_update(d_meta.reshape(-1), dev(flows), torch.zeros(3 * cap * 2, dtype=torch.int32,
                                                                                             device=DEV), pend_cap=cap)
    tm = [template(L4 if len(s) == 4 else L6, s, 80, 5000 + f) for f, s in enumerate(srcs)]
    hl = np.array([len(t) for t in tm], dtype=np.uint8)
    tmpl = np.zeros((3, 64), dtype=np.uint8)
    for f, t in enumerate(tm):
        tmpl[f, :len(t)] = np.frombuffer(t, dtype=np.uint8)
    out, src, ln, n_acks = tx_ack_build(d_meta.reshape(-1), d_seg.reshape(-1), d_fl, torch.from_numpy(tmpl).to(DEV),
                                        torch.from_numpy(hl).to(DEV), 77, ack_cap=64)
    torch.cuda.synchronize()
    got = (d_fl.cpu().numpy().view(FLOW), d_pd.cpu().numpy().view(np.uint32).reshape(3, cap, 2),
           d_seg.cpu().numpy().reshape(-1).view(SEG), d_res.cpu().numpy().reshape(-1).view(RES))
    same_update(got, want, cap)
    stream = d_stream.cpu().numpy()
    sent = []
    for f, sk in enumerate(want[4]):
        advance = (int(got[0][f]["rcv_nxt"]) - next_seq[f]) & 0xFFFFFFFF
        assert advance == len(sk.appended) == got[3][f]["readable"] > 0 and got[0][f]["n_pend"] == 3
        w = stream[int(win_off[f]):int(win_off[f]) + win_len[f]]
        assert w[:advance].tobytes() == sk.appended                   # the window's readable bytes are the delivered ones
        sent.append(list(sk.sent))
    heads, n4 = ack_heads_ref(meta, got[2], got[0], tm, hl, 77)
    n = int(n_acks[0])
    assert n == len(heads) == sum(len(s) for s in sent) and int(n_acks[1]) == n4
    out, src, ln = out.cpu().numpy(), src.cpu().numpy().view(np.uint32), ln.cpu().numpy()
    for k, (i, head) in enumerate(heads):
        f = int(meta[i]["flow"])
        ip = 20 if len(head) == 40 else 40
        assert src[k] == i and ln[k] == len(head) and out[k, :len(head)].tobytes() == head
        ack_seq, window = sent[f].pop(0)                              # the ACKs send_packet recorded, in its order
        assert int.from_bytes(head[ip + 8:ip + 12], "big") == ack_seq and int.from_bytes(head[ip + 14:ip + 16], "big") == window
