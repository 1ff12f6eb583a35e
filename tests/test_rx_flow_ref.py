"""The TCP flow update without a GPU: the restatement of tcp.rs:642-740 (rx_flow_helper.update_ref) and
the package's host walk (flow.flow_update_host) agree record for record on the reference's reassembler
unit tests (tests/golden/reassembler_kats.json) run as one-flow batches, on the delayed-ACK cadence,
on the ACK-field and window rules across the 2^32 wrap, and on every stop reason."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from rustnetworkstack_amd import _lib, batch, flow
from rx_flow_helper import (ACK, EV_WND, FIN, FLOW, META, NONE, P_FLOW, P_OUTSIDE, P_TCP, PSH, RES, RST, S_ACK, S_CONSUMED,
                            S_TIMER, SEG, STOP_FLAGS, STOP_MANY, STOP_NONE, STOP_OPTIONS, STOP_OUTSIDE, STOP_PEND,
                            STOP_STATE, SYN, flow_rec, metas, same_update, update_ref)

with open(os.path.join(GOLDEN, "reassembler_kats.json")) as _f:
    KATS = json.load(_f)["kats"]
CAP = 4


def host(meta, flows, pend, cap):
    """flow_update_host, checked against update_ref; returns the host's outputs."""
    flows = np.asarray(flows, dtype=FLOW).reshape(-1)
    want = update_ref(meta, flows, pend, cap)
    got = flow.flow_update_host(meta, flows, pend, cap)
    same_update(got, want, cap)
    return got


def test_layouts_and_exports():
    assert (flow.FLOW_DTYPE, flow.SEG_DTYPE, flow.RES_DTYPE) == (FLOW, SEG, RES)
    assert flow.META_DTYPE == META
    for name in ("FLOW_DTYPE", "SEG_DTYPE", "RES_DTYPE", "rx_tcp_flow_update", "tx_ack_build", "flow_update_host"):
        assert getattr(batch, name) is getattr(flow, name)
    assert (_lib.RNS_SEG_CONSUMED, _lib.RNS_SEG_ACK, _lib.RNS_SEG_TIMER, _lib.RNS_EV_WND) == (S_CONSUMED, S_ACK, S_TIMER, EV_WND)
    assert (_lib.RNS_STOP_NONE, _lib.RNS_STOP_MANY, _lib.RNS_STOP_STATE, _lib.RNS_STOP_FLAGS, _lib.RNS_STOP_OPTIONS,
            _lib.RNS_STOP_OUTSIDE, _lib.RNS_STOP_PEND) == (STOP_NONE, STOP_MANY, STOP_STATE, STOP_FLAGS, STOP_OPTIONS,
                                                           STOP_OUTSIDE, STOP_PEND)


# 1. the reference's reassembler tests as one-flow batches -------------------------------------------
@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kats_whole_and_call_by_call(kat):
    calls = kat["calls"]
    meta = metas([dict(seq=c["seq"], pay_len=c["len"], flags=ACK | PSH) for c in calls])
    start = np.array([flow_rec(rcv_nxt=kat["next_expect"], rcv_max=kat["next_expect"])], dtype=FLOW)
    fl, pend, seg, res = host(meta, start, np.zeros((1, CAP, 2), dtype=np.uint32), CAP)     # once whole
    assert (fl[0]["rcv_nxt"], fl[0]["n_pend"]) == (calls[-1]["next_expect"], calls[-1]["pending"])
    assert res[0]["readable"] == sum(c["delivered"] for c in calls) and res[0]["consumed"] == len(calls)
    assert res[0]["why"] == STOP_NONE and res[0]["stop"] == NONE and (seg["act"] & S_CONSUMED).all()
    fl, pend = start, np.zeros((1, CAP, 2), dtype=np.uint32)                                 # one call per batch
    for i, c in enumerate(calls):
        fl, pend, seg, res = host(meta[i:i + 1], fl, pend, CAP)
        assert (fl[0]["rcv_nxt"], fl[0]["n_pend"], res[0]["readable"]) == (c["next_expect"], c["pending"], c["delivered"])
    assert fl[0]["rq_len"] == sum(c["delivered"] for c in calls)


# 2. the delayed-ACK cadence ---------------------------------------------------------------------------
def test_delayed_ack_cadence():
    meta = metas([dict(seq=5000 + 100 * k, pay_len=100) for k in range(12)])
    fl, _, seg, res = host(meta, [flow_rec(rcv_nxt=5000, rq_len=7)], None, 0)
    act = seg["act"].tolist()
    assert [k + 1 for k, a in enumerate(act) if a & S_TIMER] == [1, 6, 11]
    assert [k + 1 for k, a in enumerate(act) if a & S_ACK] == [5, 10]
    assert seg[4]["ack_num"] == 5500 and seg[4]["window"] == 0xFFFF - 507
    assert seg[9]["ack_num"] == 6000 and seg[9]["window"] == 0xFFFF - 1007
    assert (seg["ack_num"][[0, 5, 11]] == 0).all() and all(a & S_CONSUMED for a in act)
    assert (fl[0]["delayed_acks"], fl[0]["ack_timer"], res[0]["n_acks"], res[0]["readable"]) == (2, 1, 2, 1200)
    # a timer already running and four segments deferred: the first segment is answered at once
    fl, _, seg, res = host(meta[:3], [flow_rec(rcv_nxt=5000, delayed_acks=4, ack_timer=1)], None, 0)
    assert seg["act"].tolist() == [S_CONSUMED | S_ACK, S_CONSUMED | S_TIMER, S_CONSUMED]
    assert (seg[0]["ack_num"], seg[0]["window"], fl[0]["delayed_acks"], fl[0]["ack_timer"]) == (5100, 0xFFFF - 100, 2, 1)
    # pure ACKs neither count nor arm the timer
    fl, _, seg, res = host(metas([dict(seq=5000)] * 7), [flow_rec(rcv_nxt=5000)], None, 0)
    assert (seg["act"] == S_CONSUMED).all() and fl[0]["delayed_acks"] == 0 and fl[0]["ack_timer"] == 0


# 3. the ACK field and the window ---------------------------------------------------------------------
@pytest.mark.parametrize("una", [1000, 0xFFFFFF00])
def test_ack_field(una):
    nxt = (una + 600) & 0xFFFFFFFF
    base = dict(snd_una=una, snd_nxt=nxt, snd_wnd=111, snd_wl1=49, snd_wl2=(una - 5) & 0xFFFFFFFF, rcv_nxt=50)
    for d, acked in ((-1, 0), (0, 0), (300, 300), (600, 600), (601, 0)):      # below, at, inside, at snd_nxt, beyond
        ack = (una + d) & 0xFFFFFFFF
        fl, _, seg, res = host(metas([dict(seq=50, ack=ack, window=0x1234)]), [flow_rec(**base)], None, 0)
        assert res[0]["acked"] == acked and fl[0]["snd_una"] == ((una + acked) & 0xFFFFFFFF)
        moved = 0 <= d <= 600
        assert (res[0]["events"] == EV_WND) == moved and fl[0]["snd_wnd"] == (0x1234 if moved else 111)
        assert seg[0]["act"] == S_CONSUMED
    # no ACK flag: nothing of it runs
    fl, _, _, res = host(metas([dict(seq=50, ack=(una + 300) & 0xFFFFFFFF, flags=PSH, pay_len=1)]), [flow_rec(**base)], None, 0)
    assert res[0]["acked"] == 0 and res[0]["events"] == 0 and fl[0]["snd_una"] == una


def test_window_update_rule():
    una = 0xFFFFFFF0
    st = dict(snd_una=una, snd_nxt=(una + 100) & 0xFFFFFFFF, snd_wnd=500, snd_wl1=200, snd_wl2=una, rcv_nxt=200)
    old = metas([dict(seq=150, ack=una, window=9)])                   # an old segment must not move the window
    fl, _, _, res = host(old, [flow_rec(**st)], None, 0)
    assert fl[0]["snd_wnd"] == 500 and res[0]["events"] == 0
    dup = metas([dict(seq=200, ack=una, window=77)])                  # a duplicate may: wl1 == seq, wl2 <= ack
    fl, _, _, res = host(dup, [flow_rec(**st)], None, 0)
    assert (fl[0]["snd_wnd"], fl[0]["snd_wl1"], fl[0]["snd_wl2"], res[0]["events"]) == (77, 200, una, EV_WND)
    st2 = dict(st, snd_wl2=(una + 10) & 0xFFFFFFFF)
    stale = metas([dict(seq=200, ack=(una + 10 - 1) & 0xFFFFFFFF, window=77)])    # wl1 == seq but an older ack
    fl, _, _, res = host(stale, [flow_rec(**st2)], None, 0)
    assert fl[0]["snd_wnd"] == 500 and res[0]["events"] == 0
    both = metas([dict(seq=201, ack=(una + 40) & 0xFFFFFFFF, window=5), dict(seq=150, ack=(una + 60) & 0xFFFFFFFF, window=6)])
    fl, _, _, res = host(both, [flow_rec(**st)], None, 0)              # the second trims but is too old for the window
    assert (fl[0]["snd_wnd"], fl[0]["snd_wl1"], res[0]["acked"], fl[0]["snd_una"]) == (5, 201, 60, (una + 60) & 0xFFFFFFFF)


# 4. every stop reason, at the first, a middle and the last segment ------------------------------------
def stopper(why, seq):
    if why == STOP_FLAGS:
        return dict(seq=seq, pay_len=10, flags=ACK | FIN)
    if why == STOP_OPTIONS:
        return dict(seq=seq, pay_len=10, tcp_hdr=24)
    if why == STOP_OUTSIDE:
        return dict(seq=seq, pay_len=10, place=P_TCP | P_FLOW | P_OUTSIDE)
    return dict(seq=seq + 5000, pay_len=10)                          # STOP_PEND: out of order, the list full


@pytest.mark.parametrize("why", [STOP_FLAGS, STOP_OPTIONS, STOP_OUTSIDE, STOP_PEND])
@pytest.mark.parametrize("at", [0, 3, 6])
def test_stops_per_segment(why, at):
    rows = []
    for k in range(7):                                               # flow 1's segments, flow 0's and 2's between them
        rows.append(dict(flow=0, seq=100 + 10 * k, pay_len=10))
        rows.append(stopper(why, 1000 + 10 * k) | dict(flow=1) if k == at else dict(flow=1, seq=1000 + 10 * k, pay_len=10))
        rows.append(dict(flow=2, seq=77, ack=3000 + k))
    meta = metas(rows)
    cap = 2
    pend = np.zeros((3, cap, 2), dtype=np.uint32)
    pend[1] = [[9000, 5], [9100, 5]]                                  # flow 1's list is full
    flows = np.array([flow_rec(rcv_nxt=100), flow_rec(rcv_nxt=1000, n_pend=2, rq_len=3),
                      flow_rec(rcv_nxt=77, snd_una=2990, snd_nxt=4000)], dtype=FLOW)
    fl, pd, seg, res = host(meta, flows, pend, cap)
    assert (res[1]["why"], res[1]["consumed"], res[1]["stop"], res[1]["n_segs"]) == (why, at, 3 * at + 1, 7)
    mine = seg[1::3].copy()
    assert (mine["act"][:at] & S_CONSUMED).all() and not mine[at:].view(np.uint8).any()   # later segments zero
    assert fl[1]["rcv_nxt"] == 1000 + 10 * at and res[1]["readable"] == 10 * at
    if at == 0:
        assert fl[1].tobytes() == flows[1].tobytes()
    alone = flow.flow_update_host(meta[meta["flow"] != 1], flows, pend, cap)              # other flows unaffected
    for f in (0, 2):
        assert fl[f] == alone[0][f] and res[f]["consumed"] == 7 and res[f]["why"] == STOP_NONE
    for why2 in (SYN, RST):
        m2 = metas([dict(seq=1000, flags=ACK | why2)])
        assert host(m2, [flow_rec(rcv_nxt=1000)], None, 0)[3][0]["why"] == STOP_FLAGS


def test_stops_per_flow():
    n = 1025
    rows = [dict(flow=0, seq=10)] * n + [dict(flow=1, seq=10, ack=k) for k in range(1024)] + [dict(flow=2, seq=1)] * 2
    rows.insert(0, dict(flow=3, seq=1))
    flows = np.array([flow_rec(snd_nxt=5), flow_rec(snd_una=0, snd_nxt=5000, rcv_nxt=10), flow_rec(state=2),
                      flow_rec(n_pend=3)], dtype=FLOW)
    fl, _, seg, res = host(metas(rows), flows, np.zeros((4, 2, 2), dtype=np.uint32), 2)
    assert res["why"].tolist() == [STOP_MANY, STOP_NONE, STOP_STATE, STOP_STATE]
    assert res["stop"].tolist() == [1, NONE, 1 + n + 1024, 0] and res["consumed"].tolist() == [0, 1024, 0, 0]
    assert res["n_segs"].tolist() == [n, 1024, 2, 1] and res[1]["acked"] == 1023
    for f in (0, 2, 3):
        assert fl[f].tobytes() == flows[f].tobytes()
    assert not seg[:1 + n].view(np.uint8).any() and (seg["act"][1 + n:1 + n + 1024] == S_CONSUMED).all()
    # not a flow's datagrams: no flow bit, or a flow index past the table
    strays = metas([dict(flow=0, seq=10, place=P_TCP), dict(flow=9, seq=10), dict(flow=0xFFFFFFFF, place=0)])
    fl, _, seg, res = host(strays, flows[:1], None, 0)
    assert res[0]["n_segs"] == 0 and res[0]["why"] == STOP_NONE and not seg.view(np.uint8).any()
    assert fl[0].tobytes() == flows[0].tobytes()


def test_random_batches_agree():
    rng = np.random.default_rng(7)
    for trial in range(30):
        nfl, cap = int(rng.integers(1, 5)), int(rng.integers(0, 4))
        flows = np.array([flow_rec(rcv_nxt=int(rng.integers(0, 2 ** 32)), snd_una=1000, snd_nxt=3000, snd_wl1=0,
                                   delayed_acks=int(rng.integers(0, 5)), ack_timer=int(rng.integers(0, 2)),
                                   rq_len=int(rng.integers(0, 70000))) for _ in range(nfl)], dtype=FLOW)
        rows = []
        for _ in range(int(rng.integers(0, 40))):
            f = int(rng.integers(0, nfl + 1))
            seq = (int(flows[min(f, nfl - 1)]["rcv_nxt"]) + 10 * int(rng.integers(-2, 12))) & 0xFFFFFFFF
            rows.append(dict(flow=f, seq=seq, pay_len=int(rng.choice([0, 10, 10, 20])), ack=int(rng.integers(900, 3100)),
                             window=int(rng.integers(0, 65536)), flags=ACK | (FIN if rng.random() < 0.02 else 0)))
        host(metas(rows), flows, np.zeros((nfl, cap, 2), dtype=np.uint32), cap)
