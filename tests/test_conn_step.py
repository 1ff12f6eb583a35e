"""The device's step logic without a GPU: conn_step, conn_stop_first and conn_close (rns_k_conn.hpp, RNS_HD: the
functions the walk kernels run) compiled by g++ into the stand-alone program tests/cpp/test_conn_step.cpp, run over
the exhaustive one-segment table plus out-of-order cases and every state's close, and compared with the
restatement in tests/tcp_conn_helper.py.  The program is also built with -fsanitize=address,undefined — again
a stand-alone program — and gives the same results there."""
import os
import subprocess

import numpy as np
import pytest

import tcp_conn_helper as H
from conftest import ROOT

CSRC = os.path.join(ROOT, "rustnetworkstack_amd", "csrc")


def _cases():
    """(op, flow record, meta record or None, pend pairs, pend_cap) per case."""
    meta, flows = H.exhaustive_table()
    cases = [(0, flows[i], meta[i], [], 0) for i in range(len(flows))]
    # out-of-order data against a pending list, in every state, with room and without
    for state in range(12):
        for flags in (H.ACK | H.PSH, H.ACK | H.FIN):
            for cap, pend in ((2, [(1012, 5)]), (2, [(1012, 5), (1030, 4)]), (3, [(1007, 5), (1012, 3), (990, 4)]), (0, [])):
                for seq in (1000, 1020):
                    fl = H.flow_rec(rcv_nxt=1000, rcv_max=1017, snd_una=50, snd_nxt=60, snd_wl1=999, rq_len=70000, n_pend=len(pend),
                                    delayed_acks=4, state=state, ack_timer=1)
                    m = H.metas([dict(seq=seq, ack=61, pay_len=7, flags=flags)])[0]
                    cases.append((0, fl, m, pend, cap))
    fl = H.flow_rec(n_pend=3, state=H.ESTABLISHED)                       # n_pend > pend_cap on input
    cases.append((0, fl, H.metas([dict()])[0], [(5, 5), (20, 5)], 2))
    for state in range(12):                                              # tcp_close in every state, in order or not
        for rmax in (1000, 1009):
            cases.append((1, H.flow_rec(rcv_nxt=1000, rcv_max=rmax, snd_nxt=77, rq_len=11, state=state), None, [], 0))
    return cases


def _expect(case):
    op, fl, m, pend, cap = case
    flows = np.array([fl] * 8, dtype=H.FLOW)                             # the program's flow index is 7
    if op == 1:
        out, ctl = H.close_ref(flows, [0] * 7 + [1])
        return [0] + [int(x) for x in out[7:8].view("<u4")] + [0, 0, 0, H.EV_STATE if ctl[7]["act"] else 0] + \
            [int(x) for x in ctl[7:8].view("<u4")]                       # (the close step keeps no sums: its events are set_state's)
    m = m.copy()
    m["flow"] = 7
    pd = np.zeros((8, cap, 2), dtype=np.uint32)
    for k, e in enumerate(pend[:cap]):
        pd[7, k] = e
    out, pends, ctl, res, _ = H.conn_ref(np.array([m]), flows, pd, cap)
    r = res[7]
    line = [int(r["why"])] + [int(x) for x in out[7:8].view("<u4")]
    line += [int(r["readable"]), int(r["acked"]), int(r["n_acks"]), int(r["events"])] + [int(x) for x in ctl[0:1].view("<u4")]
    if r["why"] == 0:
        line += [int(x) for e in pends[7] for x in e]
    return line


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_conn_step.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("conn_step")
    cases = _cases()
    with open(d / "table.txt", "w") as fh:
        for op, fl, m, pend, cap in cases:
            seg = [0, 0, 0, 0] if m is None else [int(x) for x in np.array([m]).view("<u4")[[1, 2, 4, 5]]]
            pairs = [int(x) for e in pend[:cap] for x in e] + [0] * (2 * (cap - len(pend[:cap])))
            fh.write(" ".join(str(x) for x in [op] + [int(x) for x in np.array([fl]).view("<u4")] + seg + [cap] + pairs) + "\n")
    return d, cases, [_expect(c) for c in cases]


def _run(exe, d, tag):
    res = d / f"results_{tag}.txt"
    r = subprocess.run([exe, str(d / "table.txt"), str(res)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return [[int(x) for x in line.split()] for line in open(res)]


def _compare(got, cases, want):
    assert len(got) == len(want) == len(cases)
    for k, (g, w) in enumerate(zip(got, want)):
        if w[0] != 0:                                                    # a stop: the pending list is not compared
            g = g[:len(w)]
        assert g == w, (k, cases[k][0], cases[k][1], cases[k][2], g, w)


def test_step_program_equals_the_helper(tmp_path, table):
    d, cases, want = table
    assert len(cases) == 3672 + 192 + 1 + 24
    assert {w[0] for w in want} == {0, 2, 3, 4, 5, 6, 7}                 # every stop a single segment can meet
    _compare(_run(_build(tmp_path, "conn_step"), d, "plain"), cases, want)


def test_step_program_under_sanitizers(tmp_path, table):
    d, cases, want = table
    exe = _build(tmp_path, "conn_step_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    _compare(_run(exe, d, "san"), cases, want)
