"""The TCP listen responder on the host: listen_host (the function the GPU tests compare the device with) equals
the restated reference (tcp_listen_helper.listen_ref) on every case the GPU tests run — classes, every reply
byte, ids, accept records, counts, and every byte it must not write; the reference's oddities pinned one by one;
the caps; and hand-computed datagrams whose checksum fields the oracle filled (tests/golden/tcp_listen_kats.json).
No GPU."""
import json
import os

import numpy as np
import pytest

import rx_place_helper as P
import tcp_listen_helper as H
from oracle import oracle as O
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.listen import (ACCEPT_DTYPE, key_hash, listen_host, listen_slots, listen_work)
from rustnetworkstack_amd.udp import port_table

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tcp_listen_kats.json")
ACK, SYN, RST, FIN, PSH = P.ACK, P.SYN, P.RST, P.FIN, P.PSH


def placed(case, l4=P.L4, l6=P.L6):
    """The case in its pool, shuffled, and the records the placement leaves (the restated one: every window empty)."""
    pool, idx, blk_first, len16 = P.lay_pool(case.pkts, case.buf, shuffled=True, seed=len(case.pkts))
    nfl = len(case.keys)
    z = np.zeros(nfl, dtype=np.int64)
    _, _, meta, _ = P.expected(case.pkts, case.buf, case.keys, z, z, z, np.zeros(1, np.uint8))
    return pool, idx, blk_first, len16, meta


def host(case, layout, cap=None, **kw):
    """listen_host over the case with every output array pre-filled with the sentinel."""
    pool, idx, blk_first, len16, meta = layout
    n = len(case.pkts)
    cap = n if cap is None else cap
    fill = lambda nbytes: np.full(nbytes, H.SENTINEL, np.uint8)  # noqa: E731
    return listen_host(pool, idx, blk_first, len16, P.L4, P.L6, meta, port_table(case.ports) if case.ports else None,
                       len(case.ports), H.iss_of(n), buf_bytes=case.buf, reply_cap=cap, ip_id_base=case.ip_id,
                       ip_id_add=case.ip_id_add, out=fill(64 * cap), rep_src=fill(4 * cap).view(np.uint32), rep_len8=fill(cap),
                       accept=fill(72 * cap).view(ACCEPT_DTYPE), **kw)


def same(r, want):
    conn, out, rep_src, rep_len8, accept, count = want
    assert np.array_equal(r.conn, conn), np.nonzero(r.conn != conn)[0][:10]
    assert np.array_equal(r.count, count), (r.count, count)
    assert np.array_equal(r.rep_src, rep_src) and np.array_equal(r.rep_len8, rep_len8)
    assert np.array_equal(r.out, out), np.nonzero(r.out != out)[0][:10] // 64
    assert r.accept.tobytes() == accept.tobytes()


def cases():
    return {"order": H.order_case(), "options": H.options_case()[0], "families": H.family_case(),
            "unanswered": H.unanswered_case(), "many keys": H.many_keys_case(), "colliding": H.colliding_case(key_hash, listen_slots)}


@pytest.fixture(scope="module")
def laid():
    return {name: (c, placed(c), H.listen_ref(c.pkts, c.buf, c.keys, c.ports, H.iss_of(len(c.pkts)), c.ip_id + c.ip_id_add))
            for name, c in cases().items()}


@pytest.mark.parametrize("name", list(cases()))
def test_host_equals_the_restated_reference(laid, name):
    c, layout, ref = laid[name]
    n = len(c.pkts)
    same(host(c, layout), H.expected(ref, n, n))
    assert len(ref.replies) > 0


def test_the_order_rule(laid):
    c, layout, ref = laid["order"]
    conn = host(c, layout).conn
    U, B = H.C_UNMATCHED, H.C_BUILT
    assert list(conn[:4]) == [U | H.C_RST | B, U | H.C_SYN | B, U | H.C_LATER, U | H.C_LATER]
    assert list(conn[62:66]) == [U | H.C_RST | B, U | H.C_SYN | B, U | H.C_LATER, U | H.C_LATER]
    assert conn[255] == U | H.C_SYN | B and conn[256] == U | H.C_LATER and conn[300] == U | H.C_LATER
    assert conn[257] == U | H.C_SYN | B
    assert (conn[400:420] == U | H.C_RST | B).all() and (conn[420:440] == U | H.C_SYN | B).all() and \
        (conn[440:480] == U | H.C_LATER).all()


def test_options(laid):
    (c, names), (_, layout, ref) = H.options_case(), laid["options"]
    r = host(c, layout)
    mss = {c_["src"] // 2: c_["mss"] for c_ in ref.accepts}
    got = {int(a["src"]) // 2: int(a["mss"]) for a in r.accept[:int(r.count[2])]}
    assert got == mss
    by = dict(zip(names, range(len(names))))
    assert mss[by["none"]] == 0 and mss[by["mss"]] == 1460 and mss[by["nops"]] == 1460      # mss 0 without the option
    assert mss[by["two"]] == 0x0218 and mss[by["eol"]] == 0                                  # the last one wins; EOL ends the walk
    assert mss[by["odd length"]] == 0x0100 and mss[by["other"]] == 1460 and mss[by["full"]] == 1460
    assert mss[by["past the end"]] == 0
    for shape in ("zero length", "length byte past the end", "truncated mss", "mss zero length"):
        j = by[shape]
        assert j not in mss and r.conn[2 * j] == H.C_UNMATCHED | H.C_HOST, shape
        assert r.conn[2 * j + 1] == H.C_UNMATCHED | H.C_LATER, shape                         # it still owns its key
    assert layout[4]["tcp_hdr"][2 * by["full"]] == 60


def one(pkts, ports=(80,), keys=(), buf=128, **kw):
    c = H.Case(list(pkts), list(keys), list(ports), buf)
    return c, host(c, placed(c), **kw)


def tcp_of(r, k):
    """(ip header length, the reply's bytes) of reply k."""
    d = r.out[64 * k:64 * k + int(r.rep_len8[k])].tobytes()
    return (20 if d[0] == 0x45 else 40), d


def test_pinned_oddities():
    a = H.v4(1)
    # an RST is answered with an RST; the RST's ack ignores the payload; SYN|FIN, SYN|RST and SYN|ACK open a connection
    _, r = one([H.seg(a, 1000, 81, 0x10, RST), H.seg(a, 1001, 80, 0x20, ACK | PSH, body=b"x" * 30),
                H.seg(a, 1002, 80, 0x30, SYN | FIN, body=b"yy"), H.seg(a, 1003, 80, 0x40, SYN | RST), H.seg(a, 1004, 80, 0x50, SYN | ACK),
                H.seg(a, 1005, 81, 0x60, SYN)])
    U, B = H.C_UNMATCHED, H.C_BUILT
    assert list(r.conn) == [U | H.C_RST | B, U | H.C_RST | B, U | H.C_SYN | B, U | H.C_SYN | B, U | H.C_SYN | B, U | H.C_RST | B]
    h, d = tcp_of(r, 0)
    assert d[h + 13] == 0x14 and d[h + 4:h + 8] == (1).to_bytes(4, "big") and d[h + 8:h + 12] == (0x11).to_bytes(4, "big")
    h, d = tcp_of(r, 1)
    assert d[h + 8:h + 12] == (0x21).to_bytes(4, "big") and d[h + 14:h + 16] == b"\0\0" and len(d) == 40
    h, d = tcp_of(r, 2)
    assert d[h + 13] == 0x12 and d[h + 8:h + 12] == (0x31).to_bytes(4, "big") and d[h + 20:] == bytes([2, 4, 5, 0xDC]) and len(d) == 44
    assert list(r.count) == [6, 6, 3]
    f = r.accept[0]["flow"]
    assert f["snd_una"] == 0x30 and f["snd_wl1"] == 0x30 and f["rcv_nxt"] == 0x31 and f["rcv_max"] == 0x31   # snd_una = the PEER's seq
    assert f["snd_nxt"] == H.iss_of(1)[0] and f["state"] == _lib.RNS_TCP_SYN_RECEIVED and f["snd_wl2"] == 0x01020304
    assert f["snd_wnd"] == 0x2000 and f["rq_len"] == 0 and f["n_pend"] == 0 and f["delayed_acks"] == 0 and f["ack_timer"] == 0
    assert r.accept[0]["mss"] == 0 and r.accept[0]["listener"] == 0 and r.accept[0]["src"] == 2
    assert [int(x) for x in r.accept["flow"]["snd_nxt"][:3]] == H.iss_of(3)


def test_ids_and_families(laid):
    c, layout, _ = laid["families"]
    r = host(c, layout)
    ids = [int.from_bytes(r.out[64 * k + 4:64 * k + 6].tobytes(), "big") for k in range(int(r.count[0])) if r.out[64 * k] == 0x45]
    first = (c.ip_id + c.ip_id_add) & 0xFFFF
    assert ids == [(first + j) & 0xFFFF for j in range(len(ids))] and len(ids) == r.count[1] and 0xFFFF in ids and 0 in ids
    assert r.count[1] < r.count[0] and set(r.rep_len8[:int(r.count[0])]) == {40, 44, 60, 64}


@pytest.mark.parametrize("name", ["order", "families"])
def test_caps_on_the_host(laid, name):
    c, layout, ref = laid[name]
    n, R = len(c.pkts), len(ref.replies)
    full = host(c, layout)
    for cap in (0, 1, R - 1):
        r = host(c, layout, cap=cap)
        same(r, H.expected(ref, n, cap))
        assert np.array_equal(r.count, full.count)
        nobuf = (r.conn & H.C_NOBUF) != 0
        assert nobuf.sum() == R - cap and np.array_equal(r.conn & 0x4F, full.conn & 0x4F)   # NOBUF SYNs still make LATER
    assert any(full.conn[i] & H.C_SYN for i, _, _ in ref.replies[1:])


def test_no_listener_means_all_rsts(laid):
    c, layout, _ = laid["many keys"]
    c0 = c._replace(ports=[])
    r = host(c0, layout)
    ref = H.listen_ref(c.pkts, c.buf, c.keys, [], [], 0)
    same(r, H.expected(ref, len(c.pkts), len(c.pkts)))
    assert r.count[2] == 0 and ((r.conn == 0) | (r.conn == H.C_UNMATCHED | H.C_RST | H.C_BUILT)).all()


def test_a_record_whose_claims_fail_is_no_segment():
    c = H.Case([H.seg(H.v4(1), 1, 80, 1, SYN), H.seg(H.v6(2), 2, 80, 1, SYN), H.seg(H.v4(3), 3, 80, 1, SYN)], [], [80])
    pool, idx, blk_first, len16, meta = placed(c)
    meta = meta.copy()
    meta["ip_hdr"][0] = 24     # not what the first buffer says
    meta["tcp_hdr"][1] = 64    # past any TCP header
    len16 = len16.copy()
    len16[2] = 30              # shorter than the headers the record claims
    r = host(c, (pool, idx, blk_first, len16, meta))
    assert list(r.conn) == [0, 0, 0] and list(r.count) == [0, 0, 0]


def test_golden_datagrams():
    with open(GOLDEN) as f:
        g = json.load(f)
    l4, l6 = bytes.fromhex(g["local_ipv4"]), bytes.fromhex(g["local_ipv6"])

    def dgram(s):
        src = bytes.fromhex(s["src"])
        dst = l4 if len(src) == 4 else l6
        t = bytearray(20) + bytes.fromhex(s["options"]) + bytes.fromhex(s["payload"])
        t[0:2], t[2:4] = s["sport"].to_bytes(2, "big"), s["dport"].to_bytes(2, "big")
        t[4:8], t[8:12] = s["seq"].to_bytes(4, "big"), s["ack"].to_bytes(4, "big")
        t[12], t[13] = (5 + len(s["options"]) // 8) << 4, s["flags"]
        t[14:16] = s["window"].to_bytes(2, "big")
        t[16:18] = (O.ones_comp_py(O.pseudo_header_py(src, dst, len(t), 6), bytes(t)) ^ 0xFFFF).to_bytes(2, "big")
        return P.ip4(src, dst, 6, bytes(t)) if len(src) == 4 else P.ip6(src, dst, 6, bytes(t))

    pkts = [dgram(s) for s in g["segments"]]
    want = [bytes.fromhex(h) for h in g["datagrams"]]
    for B in (128, 256):
        pool, idx, blk_first, len16 = P.lay_pool(pkts, B, shuffled=True, seed=B)
        # the placement's records, by hand: decoded, no flow
        meta = np.array([(P.NO_FLOW, s["seq"], s["ack"], s["sport"], s["dport"], s["window"], len(s["payload"]) // 2, s["flags"],
                          20 if len(s["src"]) == 8 else 40, 20 + len(s["options"]) // 2, P.P_TCP) for s in g["segments"]], dtype=P.META)
        r = listen_host(pool, idx, blk_first, len16, l4, l6, meta, port_table(g["listen_ports"]), len(g["listen_ports"]), g["iss"],
                        buf_bytes=B, ip_id_base=g["ip_id_base"])
        assert list(r.conn) == g["conn"] and list(r.count) == [4, 2, 2]
        assert [r.out[64 * k:64 * k + int(r.rep_len8[k])].tobytes() for k in range(4)] == want
        for a, w in enumerate(g["accepts"]):
            rec = r.accept[a]
            assert (int(rec["src"]), int(rec["listener"]), int(rec["mss"])) == (w["src"], w["listener"], w["mss"])
            assert int(rec["flow"]["rcv_max"]) == w["rcv_nxt"] and int(rec["flow"]["state"]) == 2
            for fld in ("rcv_nxt", "snd_una", "snd_nxt", "snd_wnd", "snd_wl1", "snd_wl2"):
                assert int(rec["flow"][fld]) == w[fld], fld


def test_work_and_slots():
    assert listen_slots(0) == 64 and listen_slots(33) == 128 and listen_slots(300) == 1024 and listen_slots(2182) == 8192
    assert listen_work(1 << 20) <= 29 << 20
    # the Python twin of the hash against the table builder: a lone key lies in the slot its probe starts at
    from rustnetworkstack_amd.place import rx_flow_table
    for src, sport, dport in ((H.v4(1), 1, 2), (H.v6(77), 40000, 443), (H.v4(513), 65535, 80)):
        tbl = rx_flow_table([(src, sport, dport)]).view(np.uint32).reshape(-1, 8)
        assert list(np.nonzero(tbl[:, 7])[0]) == [key_hash(H.key_dwords(src, sport, dport)) & (len(tbl) - 1)]
