"""The TCP connection update, the control-segment build and the close step (rns_rx_tcp_conn_update_dev,
rns_tx_tcp_ctl_build_dev, rns_tx_tcp_close_dev) on the GPU, compared bytewise with the restatement in
tests/tcp_conn_helper.py (itself held to the hand-traced lifecycles of tests/golden/tcp_conn_kats.json by
test_tcp_conn_ref.py).  Every output is pre-filled with 0xEE between two sentinel guards, so a missing write and
a stray one both show."""
import numpy as np
import pytest
import torch

import rx_place_helper as P
import tcp_conn_helper as H
import tcp_listen_helper as LH
from gpu_guard import DEV, FILL, Guarded
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.conn import rx_tcp_conn_update, tcp_conn, tx_tcp_close, tx_tcp_ctl_build
from rustnetworkstack_amd.flow import rx_tcp_flow_update, tx_ack_build
from rustnetworkstack_amd.listen import ACCEPT_DTYPE, accept_merge, tcp_listen
from rustnetworkstack_amd.place import meta_records, rx_flow_table
from rustnetworkstack_amd.udp import port_table
from rx_flow_helper import SEG, template

pytestmark = pytest.mark.gpu
FLOW, META, CTL, RES = H.FLOW, P.META, H.CTL, H.RES
KATS = H.load_kats()


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def run_update(meta, flows, pend, cap):
    """One call over host arrays: (flows_out, pend_out or None, ctl, res) as numpy, guards and inputs checked."""
    meta, flows = np.asarray(meta, dtype=META).reshape(-1), np.asarray(flows, dtype=FLOW).reshape(-1)
    n, nfl = meta.size, flows.size
    o_fl, o_ctl, o_res = Guarded(40 * nfl), Guarded(16 * n), Guarded(24 * nfl)
    o_pd = Guarded(8 * nfl * cap, dtype=torch.int32)
    d_pend = dev(np.asarray(pend, dtype=np.uint32)).view(torch.int32) if cap else None
    d_meta, d_flows = dev(meta), dev(flows)
    rx_tcp_conn_update(d_meta, d_flows, d_pend, pend_cap=cap, flows_out=o_fl.t, pend_out=o_pd.t if cap else None,
                       ctl=o_ctl.t, res=o_res.t)
    torch.cuda.synchronize()
    assert np.array_equal(d_meta.cpu().numpy().view(META), meta) and np.array_equal(d_flows.cpu().numpy().view(FLOW), flows)
    if cap:
        assert np.array_equal(d_pend.cpu().numpy().view(np.uint32), np.asarray(pend, dtype=np.uint32).reshape(-1))
    pd = o_pd.host(np.uint32).reshape(nfl, cap, 2)
    return o_fl.host(FLOW), pd if cap else None, o_ctl.host(CTL), o_res.host(RES)


def check_update(meta, flows, pend, cap, **kw):
    want = H.conn_ref(meta, flows, pend, cap, **kw)
    got = run_update(meta, flows, pend, cap)
    H.same_conn(got, want, cap)
    return got, want


def run_close(flows, op, in_place=False):
    flows = np.asarray(flows, dtype=FLOW).reshape(-1)
    o_fl, o_ctl = Guarded(40 * flows.size, init=flows if in_place else None), Guarded(16 * flows.size)
    d_in = o_fl.t if in_place else dev(flows)
    tx_tcp_close(d_in, dev(np.asarray(op, dtype=np.uint8)), flows_out=o_fl.t, ctl=o_ctl.t)
    torch.cuda.synchronize()
    return o_fl.host(FLOW), o_ctl.host(CTL)


def run_build(ctl, tmpl, head_len, base, cap, add=None, null_arrays=False):
    """(out [cap * 64], src, len8, count), every array prefilled with 0xEE between guards."""
    ctl = np.asarray(ctl, dtype=CTL).reshape(-1)
    o_out, o_src, o_len, o_cnt = Guarded(64 * cap), Guarded(4 * cap, dtype=torch.int32), Guarded(cap), Guarded(8, dtype=torch.int32)
    d_ctl, d_tm, d_hl = dev(ctl), torch.from_numpy(np.ascontiguousarray(tmpl)).to(DEV), dev(head_len)
    kw = {} if null_arrays or cap == 0 else dict(out=o_out.t, src=o_src.t, len8=o_len.t)
    tx_tcp_ctl_build(d_ctl, len(head_len), d_tm, d_hl, base, out_cap=cap, ip_id_add=None if add is None else i32([add]),
                     count=o_cnt.t, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(d_ctl.cpu().numpy().view(CTL), ctl)
    return o_out.host(), o_src.host(np.uint32), o_len.host(), o_cnt.host(np.uint32)


def check_build(ctl, tmpl, head_len, base, cap, add=None):
    """Against ctl_heads_ref, every byte: what the contract does not write still holds 0xEE."""
    heads, v4s = H.ctl_heads_ref(ctl, [bytes(t) for t in tmpl], head_len, base, add or 0)
    out, src, len8, count = run_build(ctl, tmpl, head_len, base, cap, add)
    e_out, e_src, e_len = np.full(64 * cap, FILL, np.uint8), np.full(4 * cap, FILL, np.uint8).view(np.uint32), np.full(cap, FILL, np.uint8)
    for k, (i, h) in enumerate(heads[:cap]):
        e_src[k], e_len[k] = i, 0 if h is None else len(h)
        if h is not None:
            e_out[64 * k:64 * k + len(h)] = np.frombuffer(h, dtype=np.uint8)
    assert count.tolist() == [len(heads), v4s]
    assert np.array_equal(src, e_src) and np.array_equal(len8, e_len)
    assert np.array_equal(out, e_out), np.nonzero(out != e_out)[0][:8] // 64
    return heads, (out, src, len8, count)


# the lane path ---------------------------------------------------------------------------------------------
def test_exhaustive_one_segment_table():
    meta, flows = H.exhaustive_table()
    assert len(flows) == 3672
    got, want = check_update(meta, flows, None, 0)
    assert set(int(w) for w in want[3]["why"]) == {0, 2, 3, 4, 5, 6, 7} and (want[3]["n_segs"] == 1).all()


def test_flows_without_segments_and_strangers():
    flows = np.array([H.flow_rec(rcv_nxt=5 + k, state=k % 12, n_pend=k % 3) for k in range(600)], dtype=FLOW)
    meta = H.metas([dict(flow=0xFFFFFFFF), dict(flow=600), dict(flow=7, place=1), dict(flow=9, flags=H.FIN | H.ACK)])
    got, want = check_update(meta, flows, np.zeros((600, 1, 2), dtype=np.uint32), 1)
    assert int(want[3]["n_segs"].sum()) == 1 and not got[2][:3].view(np.uint8).any()
    got = run_update(np.zeros(0, dtype=META), flows, None, 0)               # n_pkts == 0: copies and zero results
    assert np.array_equal(got[0], flows) and not got[3]["n_segs"].any() and (got[3]["stop"] == H.NONE).all()
    got = run_update(meta, np.zeros(0, dtype=FLOW), None, 0)                # n_flows == 0: zero records
    assert not got[2].view(np.uint8).any()


# the wave path ---------------------------------------------------------------------------------------------
def gpu_heads(ctl, tmpls, head_len, base):
    tm = np.zeros((len(tmpls), 64), dtype=np.uint8)
    for f, t in enumerate(tmpls):
        tm[f, :len(t)] = np.frombuffer(bytes(t), dtype=np.uint8)
    return run_build(ctl, tm, np.asarray(head_len, dtype=np.uint8), base, max(len(ctl), 1))


@pytest.mark.parametrize("case", KATS["cases"], ids=lambda c: c["name"])
def test_kat_lifecycles(case):
    upd = lambda m, f, p, c: run_update(m, f, p, c)  # noqa: E731
    H.check_kat(KATS, case, upd, run_close, gpu_heads, grouped=True)
    H.check_kat(KATS, case, upd, run_close, gpu_heads, grouped=False)


def test_list_lengths():
    meta, flows, lens, slots = H.list_lengths_case()
    got, want = check_update(meta, flows, None, 0)
    res = want[3]
    assert res["why"].tolist() == [0] * 6 + [H.STOP_MANY] and res["consumed"].tolist() == list(lens[:6]) + [0]
    assert (want[0]["state"][:6] == H.CLOSE_WAIT).all() and want[0]["state"][6] == H.ESTABLISHED
    assert int(res["stop"][6]) == int(np.flatnonzero(slots == 6)[0])


def test_order_is_the_batch_order_and_runs_repeat():
    meta, flows, pend, cap = H.order_case()                           # interleaved and order-sensitive
    want = H.conn_ref(meta, flows, pend, cap)
    rev = meta.copy()
    mine = np.flatnonzero(meta["flow"] == 0)
    rev[mine] = meta[mine[::-1]]                                      # in the helper alone: flow 0's list reversed
    assert H.conn_ref(rev, flows, pend, cap)[0][0] != want[0][0], "the batch does not depend on the order"
    got = run_update(meta, flows, pend, cap)
    H.same_conn(got, want, cap)
    assert {int(w) for w in want[3]["why"]} >= {0, H.STOP_FLAGS} and want[3]["n_acks"].max() >= 15
    again = run_update(meta, flows, pend, cap)
    for a, b in zip(got, again):
        if a.dtype == np.uint32:                                      # the pending lists: their valid entries
            assert all(np.array_equal(a[f, :got[0]["n_pend"][f]], b[f, :got[0]["n_pend"][f]]) for f in range(6))
        else:
            assert a.tobytes() == b.tobytes()


def test_stops_in_the_middle_of_a_list():
    meta, flows = H.stops_case()
    got, want = check_update(meta, flows, None, 0)
    assert want[3]["why"].tolist() == [H.STOP_TWICE, H.STOP_TWICE, H.STOP_FLAGS, 0]
    assert want[3]["consumed"].tolist() == [2, 2, 2, 5] and want[3]["stop"].tolist()[:3] == [8, 9, 10]
    for f in range(3):
        assert not got[2][np.arange(8 + f, 20, 4)].view(np.uint8).any()   # the stopping segment and all after it: zero
    assert want[0]["state"][3] == H.TIME_WAIT


@pytest.mark.parametrize("cap", (0, 4))
def test_out_of_order_data_across_a_state_change(cap):
    meta, flows = H.out_of_order_case()
    got, want = check_update(meta, flows, np.zeros((4, cap, 2), dtype=np.uint32), cap)
    if cap:
        assert (want[3]["why"] == 0).all() and want[0]["n_pend"].max() == 0 and (want[0]["rcv_nxt"] == 1130).all()
        assert want[0]["state"].tolist() == [H.CLOSE_WAIT, H.CLOSE_WAIT, H.FIN_WAIT2, H.CLOSE_WAIT]
    else:
        assert (want[3]["why"] == H.STOP_PEND).all() and (want[3]["consumed"] == 0).all()


# equivalence with the flow update and the ACK build ---------------------------------------------------------
def test_established_traffic_equals_the_flow_update():
    meta, flows = H.established_batch()
    cap, n, nfl = 8, len(meta), len(flows)
    pend = np.zeros((nfl, cap, 2), dtype=np.uint32)
    got = run_update(meta, flows, pend, cap)
    d_meta, d_flows, d_pend = dev(meta), dev(flows), dev(pend).view(torch.int32)
    f_fl, f_pd, f_seg, f_res = rx_tcp_flow_update(d_meta, d_flows, d_pend, pend_cap=cap)
    seg = f_seg.cpu().numpy().reshape(-1).view(SEG)
    assert got[0].tobytes() == f_fl.cpu().numpy().tobytes() and got[3].tobytes() == f_res.cpu().numpy().tobytes()
    f_pend = f_pd.cpu().numpy().view(np.uint32).reshape(nfl, cap, 2)
    assert all(np.array_equal(got[1][f, :got[0]["n_pend"][f]], f_pend[f, :got[0]["n_pend"][f]]) for f in range(nfl))
    ctl = got[2]
    assert np.array_equal(ctl["ack_num"], seg["ack_num"]) and np.array_equal(ctl["window"], seg["window"])
    assert np.array_equal(ctl["act"] & 7, seg["act"]) and (ctl["act"] < 8).all() and seg["act"].any()
    assert np.array_equal(ctl["flags"], np.where(seg["act"] & 2, H.ACK, 0)) and (ctl["flow"] == meta["flow"]).all()
    assert np.array_equal(ctl["seq"][seg["act"] & 2 != 0], got[0]["snd_nxt"][meta["flow"][seg["act"] & 2 != 0]])
    tm = np.zeros((nfl, 64), dtype=np.uint8)
    hl = np.array([40, 60, 40, 40, 60, 44], dtype=np.uint8)                # the last one malformed
    for f in range(nfl):
        src = bytes([10, 0, 0, f]) if hl[f] != 60 else bytes(range(16))
        t = template(src, src[::-1], 80 + f, 4000)
        tm[f, :len(t)] = np.frombuffer(t, dtype=np.uint8)
    a_out, a_src, a_len, a_n = tx_ack_build(d_meta, f_seg, f_fl, torch.from_numpy(tm).to(DEV), dev(hl), 0xFFF8, ack_cap=n)
    k = int(a_n.cpu()[0])
    out, src, len8, count = run_build(ctl, tm, hl, 0xFFF8, n)
    assert count.tolist() == a_n.cpu().numpy().view(np.uint32).tolist() and k > 20
    assert np.array_equal(src[:k], a_src.cpu().numpy().view(np.uint32)[:k]) and np.array_equal(len8[:k], a_len.cpu().numpy()[:k])
    a_out = a_out.cpu().numpy().reshape(-1, 64)
    for j in range(k):
        assert np.array_equal(out[64 * j:64 * j + int(len8[j])], a_out[j, :int(len8[j])]), j
    assert 0 in len8[:k] and 40 in len8[:k] and 60 in len8[:k]


# the control-segment build -----------------------------------------------------------------------------------
@pytest.mark.parametrize("base,add", ((0x10, None), (0xFFF0, 9), (0xFFFF, 0xFFFF)))
def test_ctl_build(base, add):
    ctl, tmpl, hl = H.ctl_cases()
    heads, _ = check_build(ctl, tmpl, hl, base, len(ctl), add)
    flags = {int(ctl[i]["flags"]) for i, h in heads if h is not None}
    assert flags >= {0x10, 0x11, 0x14, 0x04} and not flags & {0x12} and {len(h) for _, h in heads if h is not None} == {40, 60}
    assert sum(1 for i, h in heads if h is None and ctl[i]["flags"] & H.SYN) > 3


@pytest.mark.parametrize("cap", ("below", "at", "above", 0))
def test_ctl_build_caps(cap):
    ctl, tmpl, hl = H.ctl_cases()
    total = len(H.ctl_heads_ref(ctl, [bytes(t) for t in tmpl], hl, 0)[0])
    cap = {"below": total - 3, "at": total, "above": total + 5, 0: 0}[cap]
    check_build(ctl, tmpl, hl, 0xFFFE, cap)
    if cap == 0:
        _, _, _, count = run_build(ctl, tmpl, hl, 0xFFFE, 0, null_arrays=True)
        assert count[0] == total
    empty = run_build(np.zeros(0, dtype=CTL), tmpl, hl, 1, 4)
    assert empty[3].tolist() == [0, 0] and (empty[0] == FILL).all()


# the close step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", (False, True))
def test_close_every_state_and_op(in_place):
    flows = np.array([H.flow_rec(rcv_nxt=900, rcv_max=900 + 9 * (k & 1), snd_nxt=77 + k, rq_len=3 * k, state=k % 12)
                      for k in range(96 * 4)], dtype=FLOW)
    op = np.array([(k // 24) % 4 for k in range(96 * 4)], dtype=np.uint8)   # 0, 1, 2, 3: only 1 closes; two blocks
    want = H.close_ref(flows, op)
    got = run_close(flows, op, in_place)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert int((want[1]["act"] != 0).sum()) == 16


def test_close_then_build_then_the_peers_replies():
    flows = np.array([H.flow_rec(rcv_nxt=300, rcv_max=300, snd_una=40, snd_nxt=40, snd_wl1=299, state=H.ESTABLISHED),
                      H.flow_rec(rcv_nxt=300, rcv_max=300, snd_una=40, snd_nxt=40, snd_wl1=299, state=H.CLOSE_WAIT),
                      H.flow_rec(rcv_nxt=300, rcv_max=309, snd_una=40, snd_nxt=40, snd_wl1=299, state=H.CLOSE_WAIT)], dtype=FLOW)
    closed, ctl = run_close(flows, [1, 1, 1])
    want = H.close_ref(flows, [1, 1, 1])
    assert closed.tobytes() == want[0].tobytes() and ctl["ack_num"].tolist() == [300, 301, 300]
    tmpl = np.zeros((3, 64), dtype=np.uint8)
    for f in range(3):
        t = template(bytes([10, 0, 0, 1]), bytes([10, 0, 0, 9]), 80, 4000 + f)
        tmpl[f, :40] = np.frombuffer(t, dtype=np.uint8)
    heads, _ = check_build(ctl, tmpl, np.full(3, 40, np.uint8), 7, 3)
    assert all(h[33] == 0x11 for _, h in heads)
    rows = [dict(flow=0, seq=300, ack=41), dict(flow=1, seq=301, ack=41), dict(flow=2, seq=300, ack=41, pay_len=9,
                                                                                 flags=H.ACK | H.PSH),
            dict(flow=0, seq=300, ack=41, flags=H.FIN | H.ACK)]
    got, want = check_update(H.metas(rows), closed, None, 0)
    assert want[0]["state"].tolist() == [H.TIME_WAIT, H.CLOSED, H.CLOSED] and int(got[2][3]["ack_num"]) == 301


# the stream: accept -> handshake -> request -> close over three batches ----------------------------------------
def test_three_batches_through_the_stream():
    B, NC, PORT, WIN = 512, 12, 80, 4096
    srcs = [LH.v6(k) if k % 4 == 3 else LH.v4(k) for k in range(NC)]
    isn = [0xFFFFFF00 + 50 * k for k in range(NC)]
    iss = np.array(LH.iss_of(256), dtype=np.uint32)
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(DEV)  # noqa: E731
    ltbl = d(port_table([PORT]), np.int16)

    def lay(pkts, seed):
        pool, idx, blk, len16 = P.lay_pool(pkts, B, shuffled=True, seed=seed)
        return d(pool, np.uint8), i32(idx), i32(blk), d(len16, np.int16)

    # batch 1: SYNs (each twice) among strays, through the listen responder
    pk1 = []
    for j in range(200):
        k = j % NC
        pk1.append(LH.seg(srcs[k], 5000 + k, PORT, isn[k], P.SYN, LH.MSS) if j < 2 * NC else
                   LH.seg(LH.v4(100 + j), 7000, 81, j, P.ACK))
    e = torch.zeros(0, dtype=torch.int32, device=DEV)
    _, _, lis = tcp_listen(*lay(pk1, 1), P.L4, P.L6, d(rx_flow_table([]), np.uint8), e, torch.zeros(0, dtype=torch.int64, device=DEV),
                           e, torch.zeros(16, dtype=torch.uint8, device=DEV), ltbl, 1, i32(iss), buf_bytes=B, ip_id_base=100)
    cnt = lis.count.cpu().numpy().view(np.uint32)
    assert cnt[2] == NC and cnt[0] == 200 - NC
    acc = lis.accept.cpu().numpy()[:72 * NC].view(ACCEPT_DTYPE)
    keys, flows, next_seq, win_off, win_len = accept_merge(acc, new_win_off=WIN * np.arange(NC), new_win_len=WIN)
    assert (flows["state"] == H.SYN_RECEIVED).all()
    order = [int(a["src"]) % NC for a in acc]                           # flow f is connection order[f]
    tmpl = np.zeros((NC, 64), dtype=np.uint8)
    hl = np.zeros(NC, dtype=np.uint8)
    for f, k in enumerate(order):
        t = template(P.L4 if len(srcs[k]) == 4 else P.L6, srcs[k], PORT, 5000 + k)
        tmpl[f, :len(t)], hl[f] = np.frombuffer(t, dtype=np.uint8), len(t)
    d_tmpl, d_hl, table = d(tmpl, np.uint8), d(hl, np.uint8), d(rx_flow_table(keys), np.uint8)
    flows, pend = flows.view(FLOW), np.zeros((NC, 2, 2), dtype=np.uint32)
    body = lambda k, j: bytes([(k * 16 + j) & 0xFF]) * (30 + k)       # noqa: E731

    def batch(pkts, seed, flows, pend, next_seq, ip_id):
        """One tcp_conn call and its comparison with the helper over the same datagrams; returns the new state."""
        stream = torch.zeros(WIN * NC, dtype=torch.uint8, device=DEV)
        r = tcp_conn(*lay(pkts, seed), P.L4, P.L6, table, i32(next_seq), d(win_off.astype(np.int64), np.int64), i32(win_len), stream,
                     ltbl, 1, i32(iss), d(flows, np.uint8), d(pend, np.uint8).view(torch.int32), d_tmpl, d_hl, pend_cap=2,
                     buf_bytes=B, ip_id_base=ip_id)
        torch.cuda.synchronize()
        meta = meta_records(r.meta)
        payload = lambda i: pkts[i][int(meta[i]["ip_hdr"]) + 20:]     # noqa: E731
        want = H.conn_ref(meta, flows, pend, 2, payload=payload)
        got = (r.flows.cpu().numpy().reshape(-1).view(FLOW), r.pend.cpu().numpy().view(np.uint32).reshape(NC, 2, 2),
               r.ctl.cpu().numpy().reshape(-1).view(CTL), r.res.cpu().numpy().reshape(-1).view(RES))
        H.same_conn(got, want, 2)
        replies = int(r.listen.count.cpu()[1])
        H.same_heads((r.out.cpu().numpy(), r.src.cpu().numpy().view(np.uint32), r.len8.cpu().numpy(), r.count.cpu().numpy()),
                     H.ctl_heads_ref(want[2], [bytes(t) for t in tmpl], hl, ip_id, replies))
        win = stream.cpu().numpy()
        for f, sk in enumerate(want[4]):                              # the windows' contents: what the reassembler appended
            if sk is not None and sk.appended:
                assert win[WIN * f:WIN * f + len(sk.appended)].tobytes() == sk.appended, f
        return got[0], got[1], want

    # batch 2: third ACKs, requests (one out of order), some FINs, a stranger's stray and an RST
    pk2 = []
    for f, k in enumerate(order):
        s0, a0 = (isn[k] + 1) & 0xFFFFFFFF, (int(iss[f]) + 1) & 0xFFFFFFFF
        third = LH.seg(srcs[k], 5000 + k, PORT, s0, P.ACK, ack=a0)
        r1 = LH.seg(srcs[k], 5000 + k, PORT, s0, P.ACK | P.PSH, body=body(k, 1), ack=a0)
        r2 = LH.seg(srcs[k], 5000 + k, PORT, s0 + 30 + k, P.ACK | P.PSH | (P.FIN if k % 3 == 0 else 0), body=body(k, 2), ack=a0)
        mine = [r1, third, r2] if k == 5 else [third, r2, r1] if k == 7 else [third, r1, r2]   # data first; out of order
        if k % 3 == 1:
            mine.append(LH.seg(srcs[k], 5000 + k, PORT, s0 + 60 + 2 * k, P.FIN | P.ACK, ack=a0))   # a bare FIN
        if k == 11:
            mine.append(LH.seg(srcs[k], 5000 + k, PORT, 1, P.RST))
        pk2.append(mine)
    pkts2 = [LH.seg(LH.v4(200 + j), 7000, 81, j, P.ACK) for j in range(150)]
    for j, mine in enumerate(pk2):                                     # interleaved: connection j's t-th segment at 12 t + j
        for t, p in enumerate(mine):
            pkts2.insert(min(len(pkts2), 12 * t + j + 3 * t), p)
    flows2, pend2, want2 = batch(pkts2, 2, flows, pend, next_seq, 300)
    st2 = flows2["state"].tolist()
    assert H.CLOSE_WAIT in st2 and H.ESTABLISHED in st2 and H.CLOSED in st2 and (want2[3]["why"] == 0).all()
    # our side closes every connection; the FINs go through the same build
    closed, cctl = run_close(flows2, np.ones(NC, dtype=np.uint8))
    wclosed, wctl = H.close_ref(flows2, np.ones(NC, dtype=np.uint8))
    assert closed.tobytes() == wclosed.tobytes() and cctl.tobytes() == wctl.tobytes()
    check_build(cctl, tmpl, hl, 400, NC)
    # batch 3: the ACKs of our FINs, the peers' FINs, last ACKs
    pkts3 = [LH.seg(LH.v4(300 + j), 7000, 81, j, P.ACK) for j in range(170)]
    at = 0
    for f, k in enumerate(order):
        fl = closed[f]
        seq, ack = int(fl["rcv_nxt"]), (int(fl["snd_nxt"]) + 1) & 0xFFFFFFFF
        if fl["state"] == H.LAST_ACK:
            mine = [LH.seg(srcs[k], 5000 + k, PORT, (seq + 1) & 0xFFFFFFFF, P.ACK, ack=ack)]
        elif fl["state"] == H.FIN_WAIT1:
            mine = ([LH.seg(srcs[k], 5000 + k, PORT, seq, P.FIN | P.ACK, ack=ack)] if k % 2 else
                    [LH.seg(srcs[k], 5000 + k, PORT, seq, P.FIN | P.ACK, ack=ack - 1),
                     LH.seg(srcs[k], 5000 + k, PORT, (seq + 1) & 0xFFFFFFFF, P.ACK, ack=ack)] if k % 4 == 0 else
                    [LH.seg(srcs[k], 5000 + k, PORT, seq, P.ACK, ack=ack), LH.seg(srcs[k], 5000 + k, PORT, seq, P.FIN | P.ACK, ack=ack)])
        else:
            mine = [LH.seg(srcs[k], 5000 + k, PORT, seq, P.ACK, ack=ack)]
        for p in mine:
            pkts3.insert(at, p)
            at += 9
    flows3, _, want3 = batch(pkts3, 3, closed, pend2, flows2["rcv_nxt"], 500)
    assert set(flows3["state"].tolist()) == {H.CLOSED, H.TIME_WAIT} and (want3[3]["why"] == 0).all()


# seeded fuzz ---------------------------------------------------------------------------------------------------
FUZZ_SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def fuzz_wants():
    """The helper's results for every seed, with the generator's conditions asserted over them before any test looks
    at the device's."""
    return H.fuzz_wants(FUZZ_SEEDS)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(seed, fuzz_wants):
    meta, flows, pend, cap = H.fuzz_batch(seed)
    want = fuzz_wants[seed]
    arms, whys, consumed, total = H.coverage([want])                  # and each seed for itself
    assert 2 * consumed >= total and len(arms) >= 6, (arms, consumed, total)
    got = run_update(meta, flows, pend, cap)
    H.same_conn(got, want, cap)
    again = run_update(meta, flows, pend, cap)                        # the scatter's atomics may order differently
    assert got[0].tobytes() == again[0].tobytes() and got[2].tobytes() == again[2].tobytes() and got[3].tobytes() == again[3].tobytes()
