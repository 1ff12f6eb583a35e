"""echo_host — the ICMP echo responder in numpy, what the GPU tests compare the device with — against
the reference's echo path restated over a NetBuffer model (icmp_echo_helper) on every case the GPU
tests run, and against hand-computed request / reply pairs (tests/golden/icmp_echo_kats.json)."""
import json
import os

import numpy as np
import pytest

import icmp_echo_helper as H
from conftest import ROOT
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.icmp import echo_host

CASES = {B: H.cases(B) for B in (256, 512)}


def both(pkts, B, **kw):
    pool, idx, blk, len16 = H.lay_pool(pkts, B, shuffled=True, seed=3)
    ntx = sum(1 + -(-len(p) // B) for p in pkts) + 4
    free = np.random.default_rng(5).permutation(ntx).astype(np.uint32)
    txa = np.full(ntx * B, 0xA5, dtype=np.uint8)
    txb = txa.copy()
    out = echo_host(pool, idx, blk, len16, H.L4, H.L6, txa, free, buf_bytes=B, **kw)
    ref = H.respond_ref(pkts, B, txb, free, next_id=kw.get("ip_id_base", 0) + kw.get("ip_id_add", 0))
    return out, ref, txa, txb, free


@pytest.mark.parametrize("B", [256, 512])
@pytest.mark.parametrize("name", sorted(CASES[256]))
def test_host_path_equals_the_restatement(name, B):
    pkts = CASES[B][name]
    (st, l4, echo, bf, hl, pl, src, cnt), (ans, sent, srcs, ids), txa, txb, free = both(pkts, B, ip_id_base=0xFFFE, ip_id_add=3)
    assert [bool(e & _lib.RNS_ECHO_BUILT) for e in echo] == ans and src.tolist() == srcs
    assert np.array_equal(txa, txb)                                       # every byte of the transmit pool
    chains = H.expand_replies(free, bf, hl, pl, B)
    assert chains == [nb.frags for nb in sent]                            # the layout, fragment by fragment
    for fr, nb in zip(chains, sent):
        assert fr[0][2] == B and B - fr[0][1] in (24, 44)                 # the head: the last 24 / 44 bytes of its own buffer
        assert all(s == 0 for _, s, _ in fr[1:]) and all(e == B for _, _, e in fr[1:-1])
    assert cnt.tolist() == [len(sent), sum(len(nb.frags) for nb in sent), ids]
    for i, p in enumerate(pkts):                                          # the verify's verdicts
        assert (int(st[i]), int(l4[i])) == H.rx_verify_chain_ref(H.netbuffers(p, B)), i
    assert all(e in (0, _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BUILT) for e in echo)


def test_restatement_pins_the_representations():
    B = 256
    _, (ans, sent, _, _), _, _, _ = both(CASES[B]["sums"], B)
    d = H.reply_datagrams(sent)
    assert all(ans) and [x[22:24] for x in d[0:6:2]] == [b"\xff\xff"] * 3
    for k in (6, 10):
        assert d[k][22:24] == d[k + 1][22:24] == b"\0\0" and d[k + 2][42:44] == d[k + 3][42:44] == b"\0\0"
    _, (ans, sent, _, _), _, _, _ = both(CASES[B]["code"], B)
    assert [x[(41 if x[0] == 0x60 else 21)] for x in H.reply_datagrams(sent)] == [0, 0, 0]


def test_cuts_on_the_host():
    B, pkts = 256, CASES[256]["lengths"]
    pool, idx, blk, len16 = H.lay_pool(pkts, B, shuffled=True, seed=3)
    free = np.arange(200, dtype=np.uint32)
    full = echo_host(pool, idx, blk, len16, H.L4, H.L6, np.zeros(200 * B, np.uint8), free, buf_bytes=B)
    R, F = int(full[7][0]), int(full[7][1])
    assert R == len(pkts)
    for kw, nrep in (({"reply_cap": 0}, 0), ({"reply_cap": 1}, 1), ({"reply_cap": R - 1}, R - 1)):
        tx = np.zeros(200 * B, np.uint8)
        e = echo_host(pool, idx, blk, len16, H.L4, H.L6, tx, free, buf_bytes=B, **kw)
        assert e[7][0] == nrep and (e[2][nrep:] == (_lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_NOBUF)).all()
    tx = np.zeros(200 * B, np.uint8)
    e = echo_host(pool, idx, blk, len16, H.L4, H.L6, tx, free[:F - 1], buf_bytes=B)
    assert e[7][0] == R - 1 and e[2][-1] == (_lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_NOBUF)
    bad = free.copy()
    bad[1] = 100000
    e = echo_host(pool, idx, blk, len16, H.L4, H.L6, tx, bad, buf_bytes=B)
    assert e[2][0] == (_lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BADBUF) or e[2][1] == (_lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BADBUF)
    assert 0 in e[4].tolist() and e[7][0] == R


def test_hand_computed_kats():
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "icmp_echo_kats.json")))["kats"]
    assert [k["name"] for k in kats] == ["v4_ping_56", "v6_ping_56", "v4_ping_empty"]
    for B in (256, 512):
        for k in kats:
            req, want = bytes.fromhex(k["request"]), bytes.fromhex(k["reply"])
            pool, idx, blk, len16 = H.lay_pool([req], B)
            tx = np.zeros(4 * B, dtype=np.uint8)
            e = echo_host(pool, idx, blk, len16, bytes.fromhex(k["local_ipv4"]), bytes.fromhex(k["local_ipv6"]), tx,
                          np.array([2, 0, 1], dtype=np.uint32), buf_bytes=B, ip_id_base=k["ip_id"] or 0)
            assert e[2][0] == _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BUILT, k["name"]
            fr = H.expand_replies([2, 0, 1], e[3], e[4], e[5], B)[0]
            assert b"".join(tx[b * B + s:b * B + t].tobytes() for b, s, t in fr) == want, k["name"]
