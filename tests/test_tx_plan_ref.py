"""send.plan_host (the planner's closed form on the host) against tests/tx_plan_helper.plan_ref (the
reference's literal piece-by-piece loop), array for array, and plan_ref's layout against
rns_tx_segment_layout.  No GPU."""
import numpy as np
import pytest

from rustnetworkstack_amd.segment import tx_segment_layout
from rustnetworkstack_amd.send import RES_DTYPE, plan_host
from tx_plan_helper import (FILL, PLAN_BAD, PLAN_CAP, PLAN_NONE, PLAN_STATE, PLAN_TMPL, PLAN_WINDOW, RES, edge_specs, mixed_specs,
                            mk, ref_of, same_plan)

EDGES = edge_specs()


def host_of(c, **kw):
    c = dict(c, **kw)
    return plan_host(c.pop("flows"), c.pop("sq_off"), c.pop("sq_seq"), c.pop("sq_len"), c.pop("mss"), c.pop("tmpl"),
                     c.pop("head_len8"), tmpl_out_fill=FILL, **c)


def layout_matches(p, head_first_off):
    """seg_first / head_off / blk_flow equal rns_tx_segment_layout over the written descriptors."""
    sf, ho, bf, n_seg, head_end = tx_segment_layout(p["pay_len"], p["mss"], p["head_len8"], head_first_off)
    assert n_seg == int(p["n"][0]) and np.array_equal(sf, p["seg_first"]) and np.array_equal(ho, p["head_off"])
    nb = (n_seg + 63) // 64
    assert np.array_equal(bf, p["blk_flow"][:nb]) and (p["blk_flow"][nb:] == p["pay_len"].size).all()
    return head_end


def test_res_dtype_is_the_helpers():
    assert RES_DTYPE == RES and RES_DTYPE.itemsize == 16


@pytest.mark.parametrize("name", sorted(EDGES))
def test_named_edges(name):
    for rex in (True, False):
        c = mk(EDGES[name], ip_id_base=0xFFFE, ip_id_add=3, use_rexmit=rex)
        want = ref_of(c)
        same_plan(host_of(c), want)
        layout_matches(want, c["head_first_off"])


def test_the_edges_are_what_their_names_say():
    why = {k: ref_of(mk(v))["res"] for k, v in EDGES.items()}
    r = why["window exactly full"][0]
    assert (r["new_bytes"], r["new_segs"], r["why"]) == (2920, 2, PLAN_WINDOW)
    assert [int(x) for x in why["one byte short of a piece"]["new_bytes"]] == [0, 1460]
    assert [int(x) for x in why["tail fits, full piece would not"]["new_bytes"]] == [2160, 700, 1460]
    assert [int(x) for x in why["tail fits, full piece would not"]["why"]] == [PLAN_NONE, PLAN_NONE, PLAN_WINDOW]
    assert (why["window zero"]["new_bytes"] == 0).all() and int(why["window zero"]["rexmit_bytes"][1]) == 50
    r = why["window shrunk"][0]
    assert (r["new_bytes"], r["rexmit_bytes"], r["why"]) == (0, 1460, PLAN_WINDOW)
    assert [int(x) for x in why["across 2^32"]["new_bytes"]] == [0x3000, 0x3000, 0x2000]
    assert [int(x) for x in why["mss extremes"]["new_segs"]] == [5, 4, 1]
    assert [int(x) for x in why["stops"]["why"]] == [PLAN_STATE, PLAN_STATE, PLAN_BAD] + [PLAN_TMPL] * 5 + [PLAN_NONE]
    assert [int(x) for x in why["domain bounds"]["why"]] == [PLAN_WINDOW, PLAN_BAD, PLAN_NONE, PLAN_BAD, PLAN_NONE, PLAN_BAD,
                                                             PLAN_NONE, PLAN_BAD, PLAN_NONE, PLAN_BAD, PLAN_BAD]
    rows = ref_of(mk(EDGES["receive queue"]))["tmpl"]
    assert [int(rows[2 * f + 1, 34]) << 8 | int(rows[2 * f + 1, 35]) for f in range(4)] == [0xFFFF, 0, 0xFFFF, 0xFFFF - 0x2345]


def test_a_stopped_flow_is_untouched():
    c = mk(EDGES["stops"])
    p = host_of(c)
    assert np.array_equal(p["flows_out"][:8], c["flows"][:8]) and (p["pay_len"][:16] == 0).all() and (p["pay_off"][:16] == 0).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_random_flows(seed):
    c = mk(mixed_specs(257, seed), ip_id_base=0xFF00 + seed, head_first_off=(1 << 33) + 5)
    want = ref_of(c)
    assert int(want["n"][0]) > 500 and 0 < int(want["n"][1]) < int(want["n"][0])
    assert {PLAN_NONE, PLAN_WINDOW, PLAN_STATE} <= set(int(x) for x in want["res"]["why"])
    same_plan(host_of(c), want)
    layout_matches(want, c["head_first_off"])


def test_seg_cap_inside_and_on_entries():
    specs = [dict(inflight=3000, wnd=20000, unsent=4 * 1460, rexmit=1), dict(v6=True, inflight=100, wnd=9000, unsent=3000, rexmit=1),
             dict(unsent=0), dict(inflight=10, wnd=5000, unsent=100, rexmit=1)]
    full = ref_of(mk(specs))
    assert [int(x) for x in full["seg_first"]] == [0, 1, 5, 6, 9, 9, 9, 10, 11]
    seen = set()
    for cap in range(0, 13):
        c = mk(specs, seg_cap=cap, ip_id_base=0xFFFB)
        want = ref_of(c)
        same_plan(host_of(c), want)
        layout_matches(want, c["head_first_off"])
        n = int(want["n"][0])
        assert n <= cap and n in (0, 1, 5, 6, 9, 10, 11)
        seen.add(n)
        if cap in (3, 7):                                          # inside a new-data entry
            assert PLAN_CAP in [int(x) for x in want["res"]["why"]]
        if cap == 0:                                               # inside (before) a retransmit entry
            assert int(want["res"]["rexmit_bytes"][0]) == 0 and int(want["res"]["why"][0]) == PLAN_CAP
        if cap == 5:                                               # exactly on an entry's end; the next retransmit is dropped
            assert n == 5 and int(want["res"]["rexmit_bytes"][1]) == 0 and int(want["res"]["new_bytes"][0]) == 4 * 1460
    assert seen == {0, 1, 5, 6, 9, 10, 11}


def test_no_flows():
    c = mk([], seg_cap=130)
    want = ref_of(c)
    same_plan(host_of(c), want)
    assert want["seg_first"].tolist() == [0] and want["blk_flow"].tolist() == [0, 0, 0]
