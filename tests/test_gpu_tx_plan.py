"""TCP send planning (rns_tx_tcp_plan_dev) on the GPU, compared array for array, bytewise, with the
restatement of the reference's loop in tests/tx_plan_helper.py.  Every output is pre-filled with 0xEE
between two guards, so a missing write, a stray one and a template byte that should stay unwritten
all show; the inputs are read back unchanged."""
import numpy as np
import pytest
import torch

from gpu_guard import DEV, Guarded
from rustnetworkstack_amd import _lib, batch
from rustnetworkstack_amd.send import tx_plan_work, tx_tcp_plan, tx_tcp_send
from tx_plan_helper import (FILL, KEYS, PLAN_CAP, RES, chains_of, edge_specs, heads_ref, mixed_specs, mk, ref_of,
                            same_plan)
from rx_flow_helper import FLOW
from tx_segment_helper import head

pytestmark = pytest.mark.gpu
EDGES = edge_specs()
OUT_DTYPES = {"tmpl": np.uint8, "head_len8": np.uint8, "pay_off": np.uint64, "pay_len": np.uint32, "mss": np.uint16,
              "head_off": np.uint64, "seg_first": np.uint32, "blk_flow": np.uint32, "n": np.uint32, "res": RES,
              "flows_out": FLOW}
IN_KEYS = ("flows", "sq_off", "sq_seq", "sq_len", "mss", "tmpl", "head_len8")


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def run_plan(c, add_on_device=None):
    """One rns_tx_tcp_plan_dev call over the host arrays of a case: the outputs as numpy (KEYS), guards
    and inputs checked.  ``add_on_device``: pass ip_id_add as the device dword (default: iff non-zero)."""
    nfl = c["flows"].size
    E, stride, cap = 2 * nfl, int(c["tmpl"].shape[1]), int(c["seg_cap"])
    ins = {k: dev(c[k]) for k in IN_KEYS}
    rex = dev(c["rexmit"]) if c["rexmit"] is not None else None
    add = c["ip_id_add"]
    d_add = dev(np.array([add, 0xEEEEEEEE], dtype=np.uint32)) if (add if add_on_device is None else add_on_device) else None
    assert d_add is not None or add == 0
    sizes = {"tmpl": E * stride, "head_len8": E, "pay_off": 8 * E, "pay_len": 4 * E, "mss": 2 * E, "head_off": 8 * E,
             "seg_first": 4 * (E + 1), "blk_flow": 4 * ((cap + 63) // 64), "n": 8, "res": 16 * nfl, "flows_out": 40 * nfl}
    out = {k: Guarded(v) for k, v in sizes.items()}
    need = tx_plan_work(nfl)
    work = Guarded(need + 8)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    batch._call("rns_tx_tcp_plan_dev", torch.device(DEV), ptr(ins["flows"]), ptr(out["flows_out"].t), nfl, ptr(ins["sq_off"]),
                ptr(ins["sq_seq"]), ptr(ins["sq_len"]), ptr(ins["mss"]), ptr(rex), ptr(ins["tmpl"]), stride,
                ptr(ins["head_len8"]), int(c["ip_id_base"]), ptr(d_add), int(c["head_first_off"]), cap, ptr(out["tmpl"].t),
                ptr(out["head_len8"].t), ptr(out["pay_off"].t), ptr(out["pay_len"].t), ptr(out["mss"].t),
                ptr(out["head_off"].t), out["seg_first"].t.data_ptr(), ptr(out["blk_flow"].t), out["n"].t.data_ptr(),
                ptr(out["res"].t), work.t.data_ptr(), need)
    torch.cuda.synchronize()
    for k in IN_KEYS:
        assert ins[k].cpu().numpy().tobytes() == np.ascontiguousarray(c[k]).tobytes(), k
    if rex is not None:
        assert rex.cpu().numpy().tobytes() == c["rexmit"].tobytes()
    assert work.host(np.uint8)[need:].tolist() == [FILL] * 8          # nothing past the stated need
    got = {k: out[k].host(OUT_DTYPES[k]) for k in KEYS}
    got["tmpl"] = got["tmpl"].reshape(E, stride) if E else got["tmpl"]
    return got


def check(c, **kw):
    want = ref_of(c)
    got = run_plan(c, **kw)
    same_plan(got, want)
    return got, want


@pytest.mark.parametrize("nfl", [1, 2, 63, 64, 65, 255, 256, 257])
def test_flow_counts(nfl):
    stride = (64, 60, 61)[nfl % 3]                                     # rows 16-byte aligned, 4-byte aligned, unaligned
    c = mk(mixed_specs(nfl, 100 + nfl), stride=stride, ip_id_base=0xFFF0, head_first_off=(1 << 32) + 7)
    got, want = check(c)
    if nfl >= 63:
        assert 0 < int(want["n"][1]) < int(want["n"][0])               # IPv4 and IPv6: the id prefix is not the segment prefix
        assert (want["pay_len"] == 0).sum() > nfl // 4                 # empty and stopped flows between busy ones


def test_entries_past_one_block_of_scan_parts():
    nfl = 33000                                                        # E = 66,000 entries: 258 blocks of 256
    c = mk(mixed_specs(nfl, 33, short=True), ip_id_base=0x1234)
    got, want = check(c)
    assert int(want["n"][0]) > 20000 and set(want["res"]["new_segs"].tolist()) == {0, 1}


def test_entries_that_own_many_blocks():
    specs = [dict(unsent=300, mss=100), dict(mss=100, wnd=20000, unsent=130 * 100 - 7, inflight=250, rexmit=1),
             dict(v6=True, unsent=0), dict(v6=True, mss=64, wnd=0x3FFFFFFF, unsent=4097 * 64 - 63, inflight=9, rexmit=1),
             dict(unsent=5000, inflight=1, rexmit=1), dict(mss=9, wnd=0x3FFFFFFF, unsent=9 * 777, v6=True)]
    c = mk(specs, ip_id_base=0xFF80, ip_id_add=0x70)
    got, want = check(c)
    assert want["res"]["new_segs"].tolist() == [3, 130, 0, 4097, 4, 777]
    n = int(want["n"][0])
    assert n == 3 + 1 + 130 + 1 + 4097 + 1 + 4 + 777
    assert (got["blk_flow"] == 3).sum() == 2 and (got["blk_flow"] == 7).sum() >= 64   # an entry's blocks, more than a wave's lanes
    assert (got["blk_flow"][(n + 63) // 64:] == 12).all()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_named_edges(name):
    check(mk(EDGES[name], ip_id_base=0xFFFE, stride=60 if name == "stops" else 64))


def test_rexmit_forms():
    specs = mixed_specs(130, 9)
    c = mk(specs, use_rexmit=False)                                    # NULL
    assert c["rexmit"] is None
    none, _ = check(c)
    c = mk(specs)
    mixed, want = check(c)
    assert 0 < np.count_nonzero(want["res"]["rexmit_bytes"]) < 130
    c["rexmit"] = np.zeros(130, dtype=np.uint8)                        # all zero: as NULL
    zero, _ = check(c)
    same_plan(zero, none)
    assert not np.array_equal(mixed["seg_first"], none["seg_first"])


def test_ip_id_base_and_the_device_dword():
    specs = [dict(unsent=3000), dict(v6=True, unsent=3000), dict(unsent=4000, inflight=10, rexmit=1), dict(unsent=100)]
    got, _ = check(mk(specs, ip_id_base=0xFFFD))                       # wraps inside the batch, no dword
    ids = [int(got["tmpl"][e, 4]) << 8 | int(got["tmpl"][e, 5]) for e in (1, 4, 5, 7)]
    assert ids == [0xFFFD, 0, 1, 4]
    got, _ = check(mk(specs, ip_id_base=0xFFFD, ip_id_add=0x10005))    # the dword, mod 2^16
    assert (int(got["tmpl"][1, 4]) << 8 | int(got["tmpl"][1, 5])) == 2
    check(mk(specs, ip_id_base=0xFFFF), add_on_device=True)            # a dword that holds zero


def test_seg_cap():
    specs = [dict(inflight=3000, wnd=20000, unsent=4 * 1460, rexmit=1), dict(v6=True, inflight=100, wnd=9000, unsent=3000, rexmit=1),
             dict(unsent=0), dict(mss=100, wnd=30000, unsent=5500, inflight=10, rexmit=1), dict(unsent=100)]
    total = int(ref_of(mk(specs))["n"][0])
    assert total == 1 + 4 + 1 + 3 + 1 + 55 + 1
    for cap in (0, 1, 3, 5, 10, 64, 65, total, total - 1, total + 200):
        got, want = check(mk(specs, seg_cap=cap, ip_id_base=0xFFFC))
        assert int(got["n"][0]) <= cap
        if cap < total:
            assert PLAN_CAP in want["res"]["why"].tolist()
        else:
            assert int(got["n"][0]) == total and PLAN_CAP not in want["res"]["why"].tolist()


def test_no_flows():
    got, want = check(mk([], seg_cap=200))
    assert got["seg_first"].tolist() == [0] and got["n"].tolist() == [0, 0] and got["blk_flow"].tolist() == [0] * 4
    check(mk([], seg_cap=0))


def test_wrapper_returns_the_same_plan():
    c = mk(mixed_specs(70, 4), ip_id_base=77, ip_id_add=5)
    want = ref_of(c, fill=0)
    t = {k: dev(c[k]) for k in IN_KEYS}
    p = tx_tcp_plan(t["flows"], t["sq_off"].view(torch.int64), t["sq_seq"].view(torch.int32), t["sq_len"].view(torch.int32),
                    t["mss"].view(torch.uint16), t["tmpl"].view(70, -1), t["head_len8"], rexmit=dev(c["rexmit"]), ip_id_base=77,
                    ip_id_add=dev(np.array([5], dtype=np.uint32)).view(torch.int32), head_first_off=c["head_first_off"],
                    seg_cap=c["seg_cap"])
    torch.cuda.synchronize()
    got = {k: p[k].cpu().numpy().reshape(-1).view(np.uint8).view(OUT_DTYPES[k]) for k in KEYS}
    got["tmpl"] = got["tmpl"].reshape(140, -1)
    live = want["pay_len"] > 0                                          # the rows of empty entries are not written
    got["tmpl"][~live] = 0
    hl = want["head_len8"].astype(int)
    for e in np.flatnonzero(live):
        got["tmpl"][e, hl[e]:] = 0
    same_plan(got, want)
    with pytest.raises(ValueError):
        tx_tcp_plan(t["flows"], t["sq_off"].view(torch.int64)[:5], t["sq_seq"].view(torch.int32), t["sq_len"].view(torch.int32),
                    t["mss"].view(torch.uint16), t["tmpl"].view(70, -1), t["head_len8"], head_first_off=0, seg_cap=4)


# composition: plan -> segment in one stream ------------------------------------------------------------------
def arena_case(specs, **kw):
    """A case whose send buffers lie in an arena (any byte alignment: mk lays them one byte apart from an
    odd offset), the head region behind them, 4-byte aligned."""
    c = mk(specs, **kw)
    end = int((c["sq_off"] + c["sq_len"]).max()) + 1
    c["head_first_off"] = (end + 15) // 16 * 16 + 4
    return c


def test_plan_then_segment(oracle):
    specs = [dict(inflight=2000, wnd=9000, unsent=5000, rexmit=1, a=37), dict(v6=True, mss=536, wnd=3000, unsent=4000, rq_len=300),
             dict(unsent=0, inflight=10), dict(state=4, unsent=800), dict(v6=True, inflight=77, wnd=77 + 1220, unsent=3000, mss=1220,
                                                                         rexmit=1), dict(mss=1, wnd=70, unsent=67), dict(unsent=1461)]
    c = arena_case(specs, ip_id_base=0xFFFA)
    want = ref_of(c)
    total = int(want["n"][0])
    assert total == 1 + 4 + 5 + 1 + 1 + 67 + 2                         # more than one 64-segment block
    cap = total + 70
    c["seg_cap"] = cap
    want = ref_of(c)
    size = c["head_first_off"] + total * 60 + 256
    rng = np.random.default_rng(5)
    arena = rng.integers(0, 256, size, dtype=np.uint8)
    a_exp, st_exp = heads_ref(want, arena)
    d_arena = torch.from_numpy(arena).to(DEV)
    t = {k: dev(c[k]) for k in IN_KEYS}
    p, status = tx_tcp_send(d_arena, t["flows"], t["sq_off"].view(torch.int64), t["sq_seq"].view(torch.int32),
                            t["sq_len"].view(torch.int32), t["mss"].view(torch.uint16), t["tmpl"].view(len(specs), -1),
                            t["head_len8"], rexmit=dev(c["rexmit"]), ip_id_base=0xFFFA, head_first_off=c["head_first_off"],
                            seg_cap=cap)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st.size == cap and np.array_equal(st[:total], st_exp) and (st[total:] == _lib.RNS_TX_MALFORMED).all()
    assert p["n"].cpu().tolist() == [total, int(want["n"][1])]
    got = d_arena.cpu().numpy()
    head_end = c["head_first_off"] + sum(x[3] for x in chains_of(want))
    assert np.array_equal(got[:c["head_first_off"]], arena[:c["head_first_off"]])   # the data is read only
    assert np.array_equal(got[c["head_first_off"]:head_end], a_exp[c["head_first_off"]:head_end])
    assert np.array_equal(got[head_end:], arena[head_end:])            # nothing past the last head
    # the same statuses and bytes from tx_fill_chain on the expanded chains, heads built with zero checksums
    a2 = arena.copy()
    off, ln = [], []
    for e, j, ho, hl, po, n in chains_of(want):
        a2[ho:ho + hl] = np.frombuffer(head(want["tmpl"][e, :hl].tobytes(), j, int(want["mss"][e]), n), dtype=np.uint8)
        off += [ho, po]
        ln += [hl, n]
    off, ln, first = np.array(off, dtype=np.int64), np.array(ln, dtype=np.int32), (2 * np.arange(total + 1)).astype(np.int32)
    d2 = torch.from_numpy(a2).to(DEV)
    st2 = batch.tx_fill_chain(d2, torch.from_numpy(off).to(DEV), torch.from_numpy(ln).to(DEV), torch.from_numpy(first).to(DEV))
    torch.cuda.synchronize()
    assert np.array_equal(st2.cpu().numpy(), st[:total]) and np.array_equal(d2.cpu().numpy(), got)
    a2 = a2.copy()
    assert np.array_equal(oracle.tx_chain_fill(a2, off.view(np.uint64), ln.view(np.uint32), first.view(np.uint32)), st_exp)
    assert np.array_equal(a2, a_exp)                                   # and the compiled oracle agrees with heads_ref
    # with n_seg = the kept total, read from d_n: the first form
    d3 = torch.from_numpy(arena).to(DEV)
    st3 = batch.tx_segment(d3, p["tmpl"], p["head_len8"], p["pay_off"], p["pay_len"], p["mss"], p["head_off"], p["seg_first"],
                           p["blk_flow"], total)
    torch.cuda.synchronize()
    assert np.array_equal(st3.cpu().numpy(), st_exp) and np.array_equal(d3.cpu().numpy(), got)


# loopback: plan -> segment -> (peer) place -> update -> ACK build -> (sender) place -> update -> plan ---------
def plan_on_host(p, want):
    """A wrapper's plan as numpy (KEYS), the bytes the device leaves unwritten taken from ``want``."""
    E = want["pay_len"].size
    got = {k: p[k].cpu().numpy().reshape(-1).view(np.uint8).view(OUT_DTYPES[k]) for k in KEYS}
    got["tmpl"] = got["tmpl"].reshape(E, -1).copy()
    for e in range(E):
        hl = int(want["head_len8"][e]) if want["pay_len"][e] else 0
        got["tmpl"][e, hl:] = want["tmpl"][e, hl:]
    return got


def test_loopback_two_rounds():
    from rustnetworkstack_amd.flow import rx_tcp_flow_update, tx_ack_build
    from rustnetworkstack_amd.place import meta_records, rx_flow_table, rx_tcp_place_pool
    from rx_flow_helper import flow_rec, template
    from rx_place_helper import L4, L6, SENTINEL, key_of, lay_pool
    from tx_plan_helper import rows

    S4, S6 = bytes([10, 1, 2, 3]), bytes.fromhex("20010db8000000000000000000000042")   # the sender's addresses
    srcs, dsts = (S4, S6, S4), (L4, L6, L4)
    iss, piss = [0xFFFFF800, 70000, 1], [5000, 0xFFFFFFF0, 900000]     # the sender's and the peer's sequence numbers
    mss, sq_len, W0, buf = [1460, 536, 1220], [9000, 7000, 5000], 6000, 512
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32)).to(DEV)  # noqa: E731
    i64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64)).to(DEV)  # noqa: E731
    u8 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)  # noqa: E731

    # the sender: its flows, its send buffers (unaligned) in the arena, its templates
    s_flows = np.array([flow_rec(snd_una=iss[f], snd_nxt=iss[f], snd_wnd=3000, rcv_nxt=piss[f], rcv_max=piss[f],
                                 snd_wl1=(piss[f] - 1) & 0xFFFFFFFF) for f in range(3)], dtype=FLOW)
    sq_off = np.array([101, 101 + 9001, 101 + 9001 + 7001], dtype=np.uint64)
    head_first = 21200
    arena = np.random.default_rng(77).integers(0, 256, head_first + 64 * 60 + 64, dtype=np.uint8)
    s_tmpl = rows([template(srcs[f], dsts[f], 5000 + f, 80) for f in range(3)])
    hl = np.array([40, 60, 40], dtype=np.uint8)
    c = dict(flows=s_flows, sq_off=sq_off, sq_seq=np.array(iss, dtype=np.uint32), sq_len=np.array(sq_len, dtype=np.uint32),
             mss=np.array(mss, dtype=np.uint16), tmpl=s_tmpl, head_len8=hl, rexmit=None, ip_id_base=0xFFFE, ip_id_add=0,
             head_first_off=head_first, seg_cap=64)
    d_arena = u8(arena)
    d_in = dict(sq_off=i64(sq_off), sq_seq=i32(iss), sq_len=i32(sq_len), mss=torch.from_numpy(c["mss"]).to(DEV), tmpl=u8(s_tmpl),
                hl=u8(hl))

    def send(flows_t, want, **kw):
        """Plan and segment on the device; the planned datagrams, gathered from the arena."""
        p, st = tx_tcp_send(d_arena, flows_t, d_in["sq_off"], d_in["sq_seq"], d_in["sq_len"], d_in["mss"], d_in["tmpl"],
                            d_in["hl"], ip_id_base=0xFFFE, head_first_off=head_first, seg_cap=64, **kw)
        torch.cuda.synchronize()
        same_plan(plan_on_host(p, want), want)
        n = int(want["n"][0])
        assert (st.cpu().numpy()[:n] & _lib.RNS_TX_L4_FILLED).all() and (st.cpu().numpy()[n:] == _lib.RNS_TX_MALFORMED).all()
        a = d_arena.cpu().numpy()
        return p, [a[ho:ho + h].tobytes() + a[po:po + ln].tobytes() for _, _, ho, h, po, ln in chains_of(want)]

    # the peer: its flows (one segment short of an immediate ACK, W0 bytes of receive window left), its stream
    p_flows = dev(np.array([flow_rec(rcv_nxt=iss[f], rcv_max=iss[f], snd_una=piss[f], snd_nxt=piss[f], delayed_acks=4,
                                     rq_len=0xFFFF - W0, snd_wl1=(iss[f] - 1) & 0xFFFFFFFF) for f in range(3)], dtype=FLOW))
    p_tmpl = rows([template(dsts[f], srcs[f], 80, 5000 + f) for f in range(3)])
    p_table = u8(rx_flow_table([key_of(srcs[f], 5000 + f, 80) for f in range(3)]))
    win_off = np.array([16, 16 + 9008, 16 + 9008 + 7008], dtype=np.uint64)
    d_stream = torch.full((16 + 9008 + 7008 + 5008,), SENTINEL, dtype=torch.uint8, device=DEV)

    def place(pkts, local4, local6, table, next_seq, w_off, w_len, stream):
        pool, idx, blk, len16 = lay_pool(pkts, buf, shuffled=True, seed=len(pkts))
        _, _, d_meta = rx_tcp_place_pool(u8(pool), i32(idx), i32(blk), torch.from_numpy(len16.view(np.int16)).to(DEV), local4,
                                         local6, table, i32(next_seq), i64(w_off), i32(w_len), stream, buf_bytes=buf)
        return d_meta

    def peer_receives(pkts, flows_t):
        d_meta = place(pkts, L4, L6, p_table, iss, win_off, sq_len, d_stream)
        assert (meta_records(d_meta)["place"] == 7).all()             # every planned datagram verified, matched and placed
        fl, _, seg, _ = rx_tcp_flow_update(d_meta.reshape(-1), flows_t, None, pend_cap=0)
        return d_meta, fl, seg

    # round 1: 3000 bytes of window per flow
    want1 = ref_of(c)
    assert want1["res"]["new_bytes"].tolist() == [2920, 2680, 2440]
    plan1, pkts1 = send(dev(s_flows), want1)
    d_meta, p_flows1, seg = peer_receives(pkts1, p_flows)
    out, _, ack_len, n_acks = tx_ack_build(d_meta.reshape(-1), seg.reshape(-1), p_flows1, u8(p_tmpl), u8(hl), 0x4000, ack_cap=16)
    torch.cuda.synchronize()
    n_ack = int(n_acks[0])
    assert n_ack == 3 and int(n_acks[1]) == 2                          # each flow's first segment is acknowledged at once
    acks = [out[k, :int(ack_len[k])].cpu().numpy().tobytes() for k in range(n_ack)]
    # the ACKs come back to the sender: snd_una moves and the window opens
    s_table = u8(rx_flow_table([key_of(dsts[f], 80, 5000 + f) for f in range(3)]))
    d_meta_s = place(acks, S4, S6, s_table, piss, np.zeros(3, dtype=np.uint64), [16, 16, 16],
                     torch.zeros(64, dtype=torch.uint8, device=DEV))
    assert (meta_records(d_meta_s)["place"] == 3).all()
    s_flows2, _, _, _ = rx_tcp_flow_update(d_meta_s.reshape(-1), plan1["flows_out"], None, pend_cap=0)
    torch.cuda.synchronize()
    fl2 = s_flows2.cpu().numpy().view(FLOW)
    first_seg = [1460, 536, 1220]
    assert [int(x) for x in fl2["snd_una"]] == [(iss[f] + first_seg[f]) & 0xFFFFFFFF for f in range(3)]
    assert [int(x) for x in fl2["snd_wnd"]] == [W0 - first_seg[f] for f in range(3)]
    # round 2: the plan reads the flows where the update left them, the ids go on from the ACK build's count
    want2 = ref_of(dict(c, flows=fl2, ip_id_add=int(n_acks[1])))
    for f in range(3):                                                 # exactly what the opened window allows
        room = W0 - first_seg[f] - (int(want1["res"]["new_bytes"][f]) - first_seg[f])
        left = sq_len[f] - int(want1["res"]["new_bytes"][f])
        assert int(want2["res"]["new_bytes"][f]) == (left if left <= room else room // mss[f] * mss[f]) > 0
    plan2, pkts2 = send(s_flows2, want2, ip_id_add=n_acks[1:])
    _, p_flows2, _ = peer_receives(pkts2, p_flows1)
    torch.cuda.synchronize()
    stream, pf = d_stream.cpu().numpy(), p_flows2.cpu().numpy().view(FLOW)
    for f in range(3):
        total = int(want1["res"]["new_bytes"][f]) + int(want2["res"]["new_bytes"][f])
        assert int(pf[f]["rcv_nxt"]) == (iss[f] + total) & 0xFFFFFFFF
        w = stream[int(win_off[f]):int(win_off[f]) + sq_len[f] + 8]
        assert np.array_equal(w[:total], arena[int(sq_off[f]):int(sq_off[f]) + total]) and (w[total:] == SENTINEL).all()
