"""The host mirrors of the connection update, the close step and the control-segment build
(conn.conn_update_host, close_host, ctl_heads_host) against the restatement in tests/tcp_conn_helper.py and
the hand-traced lifecycles in tests/golden/tcp_conn_kats.json, on every case the GPU tests run.  No GPU."""
import numpy as np
import pytest

import tcp_conn_helper as H
from rustnetworkstack_amd import _lib, conn
from rustnetworkstack_amd.flow import FLOW_DTYPE
from rustnetworkstack_amd.place import META_DTYPE

KATS = H.load_kats()


def host_update(meta, flows, pend, cap):
    return conn.conn_update_host(np.asarray(meta).view(META_DTYPE), np.asarray(flows).view(FLOW_DTYPE), pend, cap)


def host_close(flows, op):
    out, ctl = conn.close_host(np.asarray(flows).view(FLOW_DTYPE), op)
    return out.view(H.FLOW), ctl.view(H.CTL)


def host_heads(ctl, tmpls, head_len, ip_id_base, **kw):
    tm = np.zeros((len(tmpls), 64), dtype=np.uint8)
    for f, t in enumerate(tmpls):
        tm[f, :len(t)] = np.frombuffer(bytes(t), dtype=np.uint8)
    return conn.ctl_heads_host(np.asarray(ctl).view(conn.CTL_DTYPE), len(tmpls), tm, head_len, ip_id_base, **kw)


def ref_update(meta, flows, pend, cap):
    out, pends, ctl, res, _ = H.conn_ref(meta, flows, pend, cap)
    return out, None, ctl, res


def ref_heads(ctl, tmpls, head_len, ip_id_base):
    heads, v4s = H.ctl_heads_ref(ctl, tmpls, head_len, ip_id_base)
    out, src, len8 = np.zeros(64 * max(len(heads), 1), np.uint8), np.zeros(len(heads), np.uint32), np.zeros(len(heads), np.uint8)
    for k, (i, h) in enumerate(heads):
        src[k] = i
        if h is not None:
            out[64 * k:64 * k + len(h)] = np.frombuffer(h, dtype=np.uint8)
            len8[k] = len(h)
    return out, src, len8, np.array([len(heads), v4s])


def test_constants_and_layout():
    assert (_lib.RNS_TCP_CLOSED, _lib.RNS_TCP_ESTABLISHED, _lib.RNS_TCP_SYN_RECEIVED, _lib.RNS_TCP_CLOSE_WAIT, _lib.RNS_TCP_LAST_ACK,
            _lib.RNS_TCP_FIN_WAIT1, _lib.RNS_TCP_FIN_WAIT2, _lib.RNS_TCP_CLOSING, _lib.RNS_TCP_TIME_WAIT, _lib.RNS_TCP_SYN_SENT,
            _lib.RNS_TCP_LISTEN) == tuple(range(11)) == (H.CLOSED, H.ESTABLISHED, H.SYN_RECEIVED, H.CLOSE_WAIT, H.LAST_ACK,
                                                         H.FIN_WAIT1, H.FIN_WAIT2, H.CLOSING, H.TIME_WAIT, H.SYN_SENT, H.LISTEN)
    assert (_lib.RNS_CTL_CONSUMED, _lib.RNS_CTL_SEND, _lib.RNS_CTL_ACK_TIMER, _lib.RNS_CTL_RESP_TIMER, _lib.RNS_CTL_TIMEWAIT,
            _lib.RNS_CTL_RESET, _lib.RNS_CTL_STATE) == (H.C_CONSUMED, H.C_SEND, H.C_ACK_TIMER, H.C_RESP_TIMER, H.C_TIMEWAIT,
                                                        H.C_RESET, H.C_STATE)
    assert (_lib.RNS_CTL_CONSUMED, _lib.RNS_CTL_SEND, _lib.RNS_CTL_ACK_TIMER) == (_lib.RNS_SEG_CONSUMED, _lib.RNS_SEG_ACK,
                                                                                 _lib.RNS_SEG_TIMER)
    assert (_lib.RNS_EV_STATE, _lib.RNS_STOP_TWICE) == (H.EV_STATE, H.STOP_TWICE) == (2, 7)
    assert conn.CTL_DTYPE == H.CTL and H.FLOW == FLOW_DTYPE


@pytest.mark.parametrize("grouped", (False, True))
@pytest.mark.parametrize("case", KATS["cases"], ids=lambda c: c["name"])
def test_kats_hold_for_the_helper_and_the_host_mirror(case, grouped):
    H.check_kat(KATS, case, ref_update, H.close_ref, ref_heads, grouped)
    H.check_kat(KATS, case, host_update, host_close, host_heads, grouped)


def test_exhaustive_table():
    meta, flows = H.exhaustive_table()
    want = H.conn_ref(meta, flows, None, 0)
    assert set(int(w) for w in want[3]["why"]) == {0, 2, 3, 4, 5, 6, 7}
    H.same_conn(host_update(meta, flows, None, 0), want, 0)


def test_the_wave_path_cases():
    meta, flows, _, _ = H.list_lengths_case()
    H.same_conn(host_update(meta, flows, None, 0), H.conn_ref(meta, flows, None, 0), 0)
    meta, flows, pend, cap = H.order_case()
    H.same_conn(host_update(meta, flows, pend, cap), H.conn_ref(meta, flows, pend, cap), cap)
    meta, flows = H.stops_case()
    want = H.conn_ref(meta, flows, None, 0)
    assert want[3]["why"].tolist() == [H.STOP_TWICE, H.STOP_TWICE, H.STOP_FLAGS, 0]
    H.same_conn(host_update(meta, flows, None, 0), want, 0)
    meta, flows = H.out_of_order_case()
    for cap in (0, 4):
        pend = np.zeros((4, cap, 2), dtype=np.uint32)
        H.same_conn(host_update(meta, flows, pend, cap), H.conn_ref(meta, flows, pend, cap), cap)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_fuzz(seed):
    meta, flows, pend, cap = H.fuzz_batch(seed)
    want = H.conn_ref(meta, flows, pend, cap)
    H.same_conn(host_update(meta, flows, pend, cap), want, cap)


def test_fuzz_generator_covers_the_step():
    assert set(H.fuzz_wants((1, 2, 3))) == {1, 2, 3}                    # (the conditions are asserted inside)


def test_close_every_state_and_op():
    flows = np.array([H.flow_rec(rcv_nxt=900, rcv_max=900 + 9 * (k & 1), snd_nxt=77 + k, rq_len=3 * k, state=k % 12)
                      for k in range(96)], dtype=H.FLOW)
    op = np.array([(k // 24) for k in range(96)], dtype=np.uint8)       # 0, 1, 2, 3: only 1 closes
    want = H.close_ref(flows, op)
    got = host_close(flows, op)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert int((want[1]["act"] != 0).sum()) == 4 and set(want[0]["state"][24:48]) >= {H.FIN_WAIT1, H.LAST_ACK}


@pytest.mark.parametrize("cap", (None, 0, 5, 1000))
@pytest.mark.parametrize("base,add", ((0x10, 0), (0xFFF0, 9), (0xFFFF, 0xFFFF)))
def test_ctl_heads(cap, base, add):
    ctl, tmpl, hl = H.ctl_cases()
    want = H.ctl_heads_ref(ctl, [bytes(t) for t in tmpl], hl, base, add)
    assert len(want[0]) > 60 and any(h is None for _, h in want[0]) and want[1] > 20
    got = conn.ctl_heads_host(ctl.view(conn.CTL_DTYPE), 7, tmpl, hl, base, ip_id_add=add, out_cap=cap)
    H.same_heads(got, want, cap)
