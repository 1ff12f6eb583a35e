"""The pool, TCP and UDP entries on a side stream and under graph replay (tests/stream_replay_helper.py): one test
per entry and one per advertised chain, each an eager run on a side stream, one capture, a replay over another
batch of the same shape and a replay over the first batch with the workspace the second left; and one eager test
of two streams at once.  The batch pairs and their references (the host twins, and the helpers of the families'
own tests) are those of tests/stream_pairs_helper.py, whose conditions tests/test_stream_pairs_ref.py asserts.

Every entry goes through its package wrapper with every output and workspace passed in, but the send planning
(``tx_tcp_plan`` allocates its descriptor arrays itself) and the chain wrappers ``tcp_conn`` and ``tx_tcp_send``:
their tensors come from the graph's pool and the harness keeps them."""
import pytest
import torch

import stream_pairs_helper as S
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import _work_bytes
from rustnetworkstack_amd.conn import conn_work, rx_tcp_conn_update, tcp_conn, tx_tcp_close, tx_tcp_ctl_build
from rustnetworkstack_amd.flow import flow_update_work, rx_tcp_flow_update, tx_ack_build
from rustnetworkstack_amd.icmp import echo_work, rx_icmp_echo_pool
from rustnetworkstack_amd.listen import listen_work, rx_tcp_listen_pool
from rustnetworkstack_amd.place import rx_tcp_place_pool
from rustnetworkstack_amd.pool import rx_verify_pool, tx_fill_pool
from rustnetworkstack_amd.segment import tx_segment
from rustnetworkstack_amd.send import tx_plan_work, tx_tcp_plan, tx_tcp_send
from rustnetworkstack_amd.udp import demux_work, rx_udp_demux_pool, tx_udp_send_pool, udp_send_work
from stream_replay_helper import concurrent, replay

pytestmark = pytest.mark.gpu
L4, L6, B, N, NFL = S.L4, S.L6, S.B, S.N, S.NFL
I64 = torch.int64


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def pool_of(a):
    return a["pool"], a["idx"], a["blk"], a["len16"]


def tx_form(a):
    return dict(tx_blk_first=a["tx_blk_first"], tx_head_len8=a["tx_head_len8"], tx_pay_len16=a["tx_pay_len16"], tx_src=a["tx_src"],
                count=a["count"])


# the calls, each over the arrays of its pair -----------------------------------------------------------------
def run_verify(a):
    rx_verify_pool(*pool_of(a), L4, L6, buf_bytes=B, status=a["status"], l4_sum=a["l4"])


def run_place(a):
    rx_tcp_place_pool(*pool_of(a), L4, L6, a["table"], a["next_seq"], a["win_off"], a["win_len"], a["stream"], buf_bytes=B,
                      status=a["status"], l4_sum=a["l4"], meta=a["meta"])


def run_flow(a):
    rx_tcp_flow_update(a["meta"], a["flows"], a["pend"], pend_cap=S.PEND_CAP, flows_out=a["flows_out"], pend_out=a["pend_out"],
                       seg=a["seg"], res=a["res"], work=a["work"])


def run_ack(a, flows="flows", work="work"):
    tx_ack_build(a["meta"], a["seg"], a[flows], a["tmpl"], a["head_len8"], S.ACK_ID, ack_cap=N, tmpl_stride=64, out=a["out"],
                 ack_src=a["ack_src"], ack_len8=a["ack_len8"], n_acks=a["n_acks"], work=a[work])


def run_conn(a):
    rx_tcp_conn_update(a["meta"], a["flows"], a["pend"], pend_cap=S.PEND_CAP, flows_out=a["flows_out"], pend_out=a["pend_out"],
                       ctl=a["ctl"], res=a["res"], work=a["work"])


def run_ctl(a):
    tx_tcp_ctl_build(a["ctl"], NFL, a["tmpl"], a["head_len8"], S.CTL_ID, out_cap=N, ip_id_add=a["ip_id_add"], tmpl_stride=64,
                     out=a["out"], src=a["src"], len8=a["len8"], count=a["count"], work=a["work"])


def run_close(a):
    tx_tcp_close(a["flows"], a["op"], flows_out=a["flows_out"], ctl=a["ctl"])


def run_listen(a):
    rx_tcp_listen_pool(*pool_of(a), L4, L6, a["meta"], a["listen_tbl"], 2, a["iss"], buf_bytes=B, reply_cap=N,
                       ip_id_base=S.LISTEN_ID, ip_id_add=a["ip_id_add"], out=a["out"], rep_src=a["rep_src"], rep_len8=a["rep_len8"],
                       accept=a["accept"], count=a["count"], conn=a["conn"], work=a["work"].view(I64))


def run_echo(a):
    rx_icmp_echo_pool(*pool_of(a), L4, L6, a["tx_pool"], a["free"], buf_bytes=B, reply_cap=S.ECHO_CAP, ip_id_base=S.ECHO_ID,
                      ip_id_add=a["ip_id_add"], status=a["status"], l4_sum=a["l4"], echo=a["echo"], work=a["work"].view(I64),
                      **tx_form(a))


def run_demux(a, count="count"):
    rx_udp_demux_pool(*pool_of(a), L4, L6, a["port_tbl"], len(S.UDP_PORTS[0]), buf_bytes=B, rec_cap=N, data=a["data"], rec=a["rec"],
                      status=a["status"], l4_sum=a["l4"], udp=a["udp"], pos=a["pos"], q_first=a["q_first"], count=a[count],
                      work=a["work"].view(I64))


def run_udp_send(a, work="work"):
    tx_udp_send_pool(a["data"], a["rec"], a["q_first"], a["sock_port"], L4, L6, a["tx_pool"], a["free"], buf_bytes=B, n_recs=N,
                     send_cap=S.SEND_CAP, ip_id_base=S.UDP_ID, ip_id_add=a["ip_id_add"], send=a["send"], work=a[work].view(I64),
                     **tx_form(a))


def run_tx_fill(a):
    tx_fill_pool(a["pool"], a["idx"], a["blk"], a["head_len8"], a["pay_len16"], buf_bytes=B, status=a["status"])


def plan_args(a):
    return (a["flows"], a["sq_off"], a["sq_seq"], a["sq_len"], a["mss"], a["tmpl"].view(S.PLAN_FLOWS, -1), a["head_len8"]), \
        dict(rexmit=a["rexmit"], ip_id_base=S.PLAN_ID, ip_id_add=a["ip_id_add"], head_first_off=S.HEAD0, seg_cap=S.SEG_CAP,
             work=a["work"], flows_out=a["p_flows_out"])


PLAN_HELD = tuple("p_" + k for k in S.PLAN_KEYS if k != "flows_out")   # what tx_tcp_plan allocates itself


def run_plan(a):
    args, kw = plan_args(a)
    p = tx_tcp_plan(*args, **kw)
    return {k: p[k[2:]] for k in PLAN_HELD}


def run_segment(a):
    tx_segment(a["arena"], a["tmpl"].view(2 * S.PLAN_FLOWS, -1), a["head_len8"], a["pay_off"], a["pay_len"], a["mss"], a["head_off"],
               a["seg_first"], a["blk_flow"], S.SEG_CAP, status=a["status"])


# one replay test per entry ------------------------------------------------------------------------------------
ENTRIES = {
    "rx_verify_pool": (run_verify, lambda: {}),
    "rx_tcp_place_pool": (run_place, lambda: {}),
    "rx_tcp_flow_update": (run_flow, lambda: dict(work=flow_update_work(N, NFL))),
    "tx_ack_build": (run_ack, lambda: dict(work=flow_update_work(N, 0))),
    "rx_tcp_conn_update": (run_conn, lambda: dict(work=conn_work(N, NFL))),
    "tx_tcp_ctl_build": (run_ctl, lambda: dict(work=_work_bytes("rns_tx_tcp_ctl_build_work", N))),
    "tx_tcp_close": (run_close, lambda: {}),
    "rx_tcp_listen_pool": (run_listen, lambda: dict(work=listen_work(N))),
    "rx_icmp_echo_pool": (run_echo, lambda: dict(work=echo_work(N))),
    "rx_udp_demux_pool": (run_demux, lambda: dict(work=demux_work(N, len(S.UDP_PORTS[0])))),
    "tx_udp_send_pool": (run_udp_send, lambda: dict(work=udp_send_work(N))),
    "tx_fill_pool": (run_tx_fill, lambda: {}),
    "tx_tcp_plan": (run_plan, lambda: dict(work=tx_plan_work(S.PLAN_FLOWS))),
    "tx_segment": (run_segment, lambda: {}),
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_on_a_side_stream_and_replayed(name):
    run, works = ENTRIES[name]
    X, Y = S.PAIRS[name]()
    replay(run, X, Y, works(), held=PLAN_HELD if name == "tx_tcp_plan" else ())


# one replay test per advertised chain, each captured as one graph ------------------------------------------------
def test_chain_tcp_conn():
    """conn.tcp_conn: pool verify and placement, listen responder, connection update, control build; the reply
    count is added to the control segments' IPv4 ids on the device."""
    X, Y = S.tcp_conn_chain_pair()

    def run(a):
        r = tcp_conn(*pool_of(a), L4, L6, a["table"], a["next_seq"], a["win_off"], a["win_len"], a["stream"], a["listen_tbl"], 2,
                     a["iss"], a["flows"], a["pend"], a["tmpl"].view(NFL, 64), a["head_len8"], pend_cap=S.PEND_CAP, buf_bytes=B,
                     ip_id_base=S.LISTEN_ID, ip_id_add=a["ip_id_add"])
        lis = r.listen
        return dict(status=r.status, meta=r.meta, l_conn=lis.conn, l_out=lis.out, l_rep_src=lis.rep_src, l_rep_len8=lis.rep_len8,
                    l_accept=lis.accept, l_count=lis.count, flows_out=r.flows, pend_out=r.pend, ctl=r.ctl, res=r.res, out=r.out,
                    src=r.src, len8=r.len8, count=r.count)

    replay(run, X, Y, {}, held=tuple(k for k in X.want if k != "stream"))


def test_chain_tx_tcp_send():
    """send.tx_tcp_send: the plan, then the segmentation with n_seg = seg_cap.  The plans' counts differ, so the
    segments between them are RNS_TX_MALFORMED with no byte written in one batch and real ones in the other."""
    X, Y = S.tcp_send_chain_pair()

    def run(a):
        args, kw = plan_args(a)
        p, status = tx_tcp_send(a["arena"], *args, status=a["status"], **kw)
        assert status is a["status"]
        return {k: p[k[2:]] for k in PLAN_HELD}

    replay(run, X, Y, dict(work=tx_plan_work(S.PLAN_FLOWS)), held=PLAN_HELD)


def test_chain_demux_then_send():
    """rx_udp_demux_pool, then tx_udp_send_pool straight over its records."""
    X, Y = S.demux_send_chain_pair()

    def run(a):
        run_demux(a, count="d_count")
        run_udp_send(a, work="work_send")

    replay(run, X, Y, dict(work=demux_work(N, len(S.UDP_PORTS[0])), work_send=udp_send_work(N)))


def test_chain_place_flow_update_ack_build():
    X, Y = S.place_flow_ack_chain_pair()

    def run(a):
        run_place(a)
        run_flow(a)
        run_ack(a, flows="flows_out", work="work_ack")

    replay(run, X, Y, dict(work=flow_update_work(N, NFL), work_ack=flow_update_work(N, 0)))


# two streams at once ---------------------------------------------------------------------------------------------
def test_two_streams_hold_no_shared_state():
    """Listen on one stream and demux on the other, then echo and connection update, X and Y alternately: every
    round of every job equals its reference, so nothing of one call lives in the library for another to find."""
    job = lambda name: (ENTRIES[name][0],) + S.PAIRS[name]() + (ENTRIES[name][1](),)  # noqa: E731
    concurrent([[job("rx_tcp_listen_pool"), job("rx_icmp_echo_pool")], [job("rx_udp_demux_pool"), job("rx_tcp_conn_update")]])
