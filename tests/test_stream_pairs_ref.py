"""The batch pairs of tests/stream_pairs_helper.py, checked on the CPU with the host twins alone: what a pair must
have for the replay tests of tests/test_gpu_streams.py to mean anything.  X and Y agree in every by-value argument
and array size (a captured graph fixes exactly those), every output differs between them (a replay that
recomputed nothing, or kept a value of X's, cannot pass), and each reference takes the branches of its family.
These are conditions on the inputs: the builders are written to meet them."""
import numpy as np
import pytest

import stream_pairs_helper as S
from rustnetworkstack_amd import _lib
from udp_demux_helper import TILE

FAMILIES = sorted(S.PAIRS)


@pytest.mark.parametrize("name", FAMILIES)
def test_by_value_arguments_and_sizes_agree(name):
    X, Y = S.PAIRS[name]()
    assert X.args == Y.args and X.args
    for role in ("ins", "io", "want", "slack"):
        a, b = getattr(X, role), getattr(Y, role)
        assert list(a) == list(b), role
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].nbytes == b[k].nbytes, (role, k)
    assert set(X.io) <= set(X.want) and not set(X.ins) & set(X.want)
    for k, m in X.slack.items():
        assert m.dtype == bool and m.size == X.want[k].nbytes, k


@pytest.mark.parametrize("name", FAMILIES)
def test_every_array_differs(name):
    X, Y = S.PAIRS[name]()
    same = lambda a, b: np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()  # noqa: E731
    assert not [k for k in X.want if same(X.want[k], Y.want[k])], "outputs that are the same in X and Y"   # the counters among them
    assert not [k for k in X.ins if same(X.ins[k], Y.ins[k])], "inputs that are the same in X and Y"
    for b in (X, Y):                                                     # and a call that wrote nothing cannot pass either
        assert not [k for k, w in b.want.items() if same(w, b.io[k] if k in b.io else S.poison(w.nbytes))], "outputs nothing is written to"


def test_sizes_have_structure():
    assert S.N > 2 * 256 + 64 and S.N % 64 and S.N > TILE                # scan blocks, a partial 64-item block, two tiles
    X, _ = S.flow_pair()
    assert 70 <= X.args["n_flows"] <= 100
    for b in S.flow_pair() + S.conn_pair():
        n = b.info["n_segs"]
        assert (n == 1).sum() >= 20 and (n > 1).sum() >= 40 and n.max() <= 64   # the lane path and the wave path


@pytest.mark.parametrize("pair", [S.flow_pair, S.conn_pair])
def test_segment_counts_differ_for_half_the_flows(pair):
    X, Y = pair()
    assert (X.info["n_segs"] != Y.info["n_segs"]).sum() * 2 >= S.NFL
    assert X.info["n_segs"].sum() == Y.info["n_segs"].sum()                 # (the datagram count stays)


def test_flow_update_branches():
    for b in S.flow_pair():
        res = b.info["res"]
        assert {int(w) for w in res["why"]} >= {_lib.RNS_STOP_STATE, _lib.RNS_STOP_FLAGS, 0}
        assert res["n_acks"].sum() >= 20 and res["readable"].sum() > 1000 and res["acked"].any() and (res["events"] & _lib.RNS_EV_WND).any()
        assert b.want["flows_out"]["n_pend"].any() or (b.want["pend_out"] != 0).any()     # segments went through the pending list
    X, Y = S.ack_pair()
    assert X.want["n_acks"].tolist() != Y.want["n_acks"].tolist() and 0 < X.want["n_acks"][1] < X.want["n_acks"][0]
    for b in (X, Y):
        k = int(b.want["n_acks"][0])
        assert {0, 40, 60} <= set(b.want["ack_len8"][:k].tolist())             # IPv4, IPv6 and the malformed template


def test_conn_update_branches():
    for b in S.conn_pair():
        res, ctl, out = b.info["res"], b.want["ctl"], b.want["flows_out"]
        assert (res["events"] & _lib.RNS_EV_STATE).sum() >= 10 and (ctl["act"] & _lib.RNS_CTL_SEND).sum() >= 30
        assert (ctl["act"] & _lib.RNS_CTL_RESET).any() and (ctl["act"] & _lib.RNS_CTL_ACK_TIMER).any()
        assert len(set(out["state"].tolist())) >= 4
    X, Y = S.ctl_pair()
    assert X.want["count"].tolist() != Y.want["count"].tolist() and X.want["count"][0] != Y.want["count"][0]
    X, Y = S.close_pair()
    assert 0 < (X.want["ctl"]["act"] != 0).sum() != (Y.want["ctl"]["act"] != 0).sum() > 0


def test_listen_keys_and_later_marks():
    for pair in (S.listen_pair, S.tcp_conn_chain_pair):
        X, Y = pair()
        assert X.info["port_map"] and Y.info["port_map"] and not X.info["port_map"] & Y.info["port_map"]
        assert Y.info["later"] >= 20 and X.info["later"] >= 20
        assert all(int(a) != int(b) for a, b in zip(X.info["count"], Y.info["count"]))   # replies, IPv4 replies, accepts
    X, Y = S.listen_pair()
    for b in (X, Y):
        conn = b.want["conn"]
        assert (conn & _lib.RNS_CONN_RST).any() and (conn & _lib.RNS_CONN_SYN).any() and (conn == 0).any()
        assert {40, 44, 60, 64} <= set(b.want["rep_len8"][:int(b.info["count"][0])].tolist())


def test_nobuf_in_one_batch_only():
    for pair, bit in ((S.echo_pair, _lib.RNS_ECHO_NOBUF), (S.udp_send_pair, _lib.RNS_UDPTX_NOBUF), (S.demux_send_chain_pair, _lib.RNS_UDPTX_NOBUF)):
        X, Y = pair()
        key = "echo" if pair is S.echo_pair else "send"
        assert not (X.want[key] & bit).any() and (Y.want[key] & bit).sum() >= 10
        cx, cy = (b.info["count"] if pair is S.echo_pair else b.info["send_count"] for b in (X, Y))
        assert all(int(a) != int(b) for a, b in zip(cx, cy))               # built, buffers taken, IPv4 ids
        assert int(cy[0]) == X.args["reply_cap" if pair is S.echo_pair else "send_cap"] > int(cx[0]) > 300
    for b in S.echo_pair():
        k = int(b.info["count"][0])
        assert {24, 44} <= set(b.want["tx_head_len8"][:k].tolist()) and b.want["tx_pay_len16"][:k].max() > S.B   # two payload buffers


def test_demux_queue_lengths_differ():
    X, Y = S.demux_pair()
    assert (X.info["queues"] != Y.info["queues"]).all() and X.info["queues"].min() > 0 and Y.info["queues"].min() > 0
    assert all(int(a) != int(b) for a, b in zip(X.info["count"], Y.info["count"]))
    for b in (X, Y):
        udp = b.want["udp"]
        assert ((udp & _lib.RNS_UDP_DGRAM) != 0).sum() > ((udp & _lib.RNS_UDP_SOCK) != 0).sum() > 300 and (udp == 0).sum() >= 40
        assert not (udp & _lib.RNS_UDP_NOROOM).any()


def test_plan_counts_straddle():
    X, Y = S.tcp_send_chain_pair()
    nx, ny = int(X.info["n"][0]), int(Y.info["n"][0])
    lo, hi = sorted((nx, ny))
    assert 200 < lo and lo + 20 <= hi < S.SEG_CAP and X.info["n"][1] != Y.info["n"][1]
    a, b = (X, Y) if nx < ny else (Y, X)
    mal = _lib.RNS_TX_MALFORMED
    assert (a.info["status"][lo:] == mal).all() and not (b.info["status"][lo:hi] == mal).any() and (b.info["status"][hi:] == mal).all()
    assert (a.want["arena"][S.HEAD0 + 60 * hi:] == a.io["arena"][S.HEAD0 + 60 * hi:]).all()   # no byte past the heads
    for p in (X, Y):
        why = set(p.want["p_res"]["why"].tolist())
        assert {_lib.RNS_PLAN_WINDOW, _lib.RNS_PLAN_STATE, 0} <= why and p.want["p_res"]["rexmit_bytes"].any()


def test_transmit_finalize_kinds():
    X, Y = S.tx_fill_pair()
    assert len(set(X.want["status"].tolist())) >= 4 and sorted(X.want["status"].tolist()) == sorted(Y.want["status"].tolist())
