"""send_host — the numpy statement of rns_tx_udp_send_pool_dev that the GPU tests compare with — against the
reference's UDP send path restated in udp_send_helper (udp_send -> udp_output -> ip_output over NetBuffers), on
the cases the GPU tests run; against the receive oracle, an independent path; against hand-laid datagrams filled
by oracle.tx_fill_ref (tests/golden/udp_send_kats.json); and the cuts and layout invariants of the contract.
No GPU."""
import json
import os

import numpy as np
import pytest

import udp_demux_helper as D
import udp_send_helper as H
from oracle import oracle as O
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.udp import REC, demux_host, port_table, send_host, udp_send_work

SEND, BUILT, NOBUF, BADBUF = _lib.RNS_UDPTX_SEND, _lib.RNS_UDPTX_BUILT, _lib.RNS_UDPTX_NOBUF, _lib.RNS_UDPTX_BADBUF
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "udp_send_kats.json")
TXFILL = 0xA5


def host(b, B, *, free=None, extra=3, **kw):
    """(UdpSend, transmit pool, free list) of send_host over batch b, the free list shuffled."""
    ntx = b.tx_needed(B) + extra
    if free is None:
        free = np.random.default_rng(len(b.sends) + B).permutation(ntx).astype(np.uint32)
    tx = np.full(ntx * B, TXFILL, dtype=np.uint8)
    r = send_host(b.data, b.rec, b.q_first, b.ports, H.L4, H.L6, tx, free, buf_bytes=B, **kw)
    return r, tx, free


def datagrams(r, tx, free, B):
    return [b"".join(tx[k * B + s:k * B + e].tobytes() for k, s, e in fr)
            for fr in H.expand_replies(free, r.tx_blk_first, r.tx_head_len8, r.tx_pay_len16, B)]


def check_layout(r, b, B):
    """The contract's own invariants: the built sends are a prefix of the sends, d_tx_src is the built records in
    order, the counts are the datagrams, their buffers and their IPv4 ones."""
    sends = np.nonzero(r.send & SEND)[0]
    built = np.nonzero(r.send & (BUILT | BADBUF))[0]
    assert np.array_equal(built, sends[:len(built)]) and (r.send[sends[len(built):]] == (SEND | NOBUF)).all()
    assert np.array_equal(r.tx_src, built) and r.count[0] == len(built) == len(r.tx_pay_len16) == len(r.tx_head_len8)
    nf = 1 + -(-r.tx_pay_len16.astype(np.int64) // B)
    assert r.count[1] == nf.sum() and r.count[2] == int((b.rec["family"][built] == 4).sum())
    assert np.array_equal(r.tx_blk_first, (np.cumsum(nf) - nf)[::64])
    assert np.array_equal(r.tx_pay_len16, b.rec["len"][built])
    assert set(r.tx_head_len8[(r.send[built] & BUILT) != 0].tolist()) <= {28, 48} and (r.tx_head_len8[(r.send[built] & BADBUF) != 0] == 0).all()


@pytest.mark.parametrize("B", [256, 512])
@pytest.mark.parametrize("name", H.CASE_NAMES)
def test_host_equals_the_reference(name, B):
    b = H.case(name, B)
    r, tx, free = host(b, B, ip_id_base=0xFFFA)
    ref_tx = np.full(tx.size, TXFILL, dtype=np.uint8)
    want, frags, ids = H.send_ref(b.sends, B, ref_tx, free, next_id=0xFFFA)
    assert (r.send == (SEND | BUILT)).all() and r.count.tolist() == [len(want), b.tx_needed(B), ids]
    assert datagrams(r, tx, free, B) == want
    assert H.expand_replies(free, r.tx_blk_first, r.tx_head_len8, r.tx_pay_len16, B) == frags
    assert np.array_equal(tx, ref_tx)
    check_layout(r, b, B)


@pytest.mark.parametrize("name", ["lengths", "sums", "count257"])
def test_built_datagrams_pass_the_receive_oracle(name):
    """What a peer's stack decides for each datagram, the peer's local addresses = the destination: accepted, and
    — the receive path reads no UDP checksum — the checksum verified here over the pseudo-header of what arrived."""
    B = 256
    b = H.case(name, B)
    r, tx, free = host(b, B)
    for d, (port, dest, dport, pay) in zip(datagrams(r, tx, free, B), b.sends):
        st, _ = O.rx_verify_ref(d, dest if len(dest) == 4 else H.R4, dest if len(dest) == 16 else H.R6)
        assert st & O.RX_ACCEPT and st & O.RX_IP_OK
        h = 20 if len(dest) == 4 else 40
        src, dst = (d[12:16], d[16:20]) if h == 20 else (d[8:24], d[24:40])
        assert src == (H.L4 if h == 20 else H.L6) and dst == dest
        seg = d[h:]
        assert seg[:6] == port.to_bytes(2, "big") + dport.to_bytes(2, "big") + len(seg).to_bytes(2, "big") and seg[8:] == pay
        assert O.ones_comp_py(O.pseudo_header_py(src, dst, len(seg), 17), seg) == 0xFFFF


def test_golden_datagrams():
    with open(GOLDEN) as f:
        g = json.load(f)
    l4, l6 = bytes.fromhex(g["local_ipv4"]), bytes.fromhex(g["local_ipv6"])
    socks = [(s["port"], [(bytes.fromhex(d["dest"]), d["dport"], bytes.fromhex(d["payload"])) for d in s["sends"]])
             for s in g["sockets"]]
    b = H.Batch(socks)
    want = [bytes.fromhex(h) for h in g["datagrams"]]
    assert any(d[0] == 0x45 and d[26:28] == b"\0\0" for d in want) and any(d[0] == 0x60 and d[46:48] == b"\0\0" for d in want)
    assert {0, 1} <= {len(p) for _, _, _, p in b.sends} and any(len(p) & 1 and len(p) > 1 for _, _, _, p in b.sends)
    for B in (256, 512):
        ntx = b.tx_needed(B)
        free = np.random.default_rng(B).permutation(ntx).astype(np.uint32)
        tx = np.zeros(ntx * B, dtype=np.uint8)
        r = send_host(b.data, b.rec, b.q_first, b.ports, l4, l6, tx, free, buf_bytes=B, ip_id_base=g["ip_id_base"])
        assert datagrams(r, tx, free, B) == want


@pytest.mark.parametrize("B", [256, 512])
def test_cuts_on_the_host(B):
    b = H.case("lengths", B)
    full, tx_full, free = host(b, B)
    R, F = len(b.sends), b.tx_needed(B)
    last = 1 + -(-len(b.sends[-1][3]) // B)
    for cap in (0, 1, R - 1, R):
        r, tx, _ = host(b, B, send_cap=cap)
        assert r.count[0] == cap and (r.send[:cap] == (SEND | BUILT)).all() and (r.send[cap:] == (SEND | NOBUF)).all()
        check_layout(r, b, B)
        nb = int(r.count[1])
        rows = np.ones(tx.size // B, dtype=bool)
        rows[free[:nb]] = False
        assert (tx.reshape(-1, B)[rows] == TXFILL).all()  # nothing written for what is not built
        assert np.array_equal(tx.reshape(-1, B)[free[:nb]], tx_full.reshape(-1, B)[free[:nb]])
    for nfree, nbuilt in ((F, R), (F - 1, R - 1), (F - last, R - 1), (0, 0)):
        r, _, _ = host(b, B, free=free[:nfree])
        assert r.count[0] == nbuilt and (r.send[nbuilt:] == (SEND | NOBUF)).all()
        check_layout(r, b, B)


def test_a_free_buffer_outside_the_pool():
    B = 256
    b = H.case("lengths", B)
    _, _, free = host(b, B)
    k = sum(1 + -(-len(p) // B) for _, _, _, p in b.sends[:18])  # send 18: IPv4, 2B + 1 bytes, free[k .. k + 4)
    assert len(b.sends[18][3]) == 2 * B + 1 and len(b.sends[18][1]) == 4
    bad = free.copy()
    bad[k + 2] = bad.size + 9
    good, tx_good, _ = host(b, B)
    r, tx, _ = host(b, B, free=bad)
    want = np.full(len(b.sends), SEND | BUILT, dtype=np.uint8)
    want[18] = SEND | BADBUF
    assert np.array_equal(r.send, want) and r.tx_head_len8[18] == 0 and r.count.tolist() == good.count.tolist()
    check_layout(r, b, B)
    rows = tx.reshape(-1, B) != tx_good.reshape(-1, B)
    assert set(np.nonzero(rows.any(axis=1))[0].tolist()) <= set(free[k:k + 4].tolist())  # its own buffers alone are not written
    assert (tx.reshape(-1, B)[free[[k, k + 1, k + 3]]] == TXFILL).all()
    # the later IPv4 datagrams keep their ids: a datagram that is not written takes its id all the same
    assert datagrams(r, tx, bad, B)[19:] == datagrams(good, tx_good, free, B)[19:]


def test_what_is_no_send():
    B = 256
    b = H.case("count65", B)
    rec = b.rec.copy()
    rec["flags"][5] = 0x03                       # decoded, a socket, not queued
    rec["flags"][6] = 0xFF                       # any other bit beside QUEUED does not matter
    rec["family"][9] = 5
    rec["family"][10] = 0
    data = b.data
    end16 = data.size // 16
    rec["off16"][40], rec["len"][40] = end16 - 1, 17         # its last byte is past the end
    rec["off16"][41], rec["len"][41] = end16 - 1, 16         # ends with the array: a send
    rec["off16"][42], rec["len"][42] = end16, 0              # nothing, at the end: a send
    rec["off16"][43], rec["len"][43] = end16 + 1, 0          # nothing, past the end
    rec["off16"][44], rec["len"][44] = 0xFFFFFFFF, 65535     # 64-bit arithmetic
    late = [40, 43, 44]
    q = b.q_first.copy()
    q[-1] = 60                                   # the host passes n_recs = rec_cap: records 60.. are no sends
    ntx = b.tx_needed(B) + 4
    tx = np.full(ntx * B, TXFILL, dtype=np.uint8)
    r = send_host(data, rec, q, b.ports, H.L4, H.L6, tx, np.arange(ntx, dtype=np.uint32), buf_bytes=B)
    no = sorted(set([5, 9, 10] + late + list(range(60, 65))))
    assert np.nonzero(r.send == 0)[0].tolist() == no and (np.delete(r.send, no) == (SEND | BUILT)).all()
    assert r.tx_src.tolist() == [k for k in range(65) if k not in no]
    # a record array zeroed before a cut demux: the unwritten records are no sends
    z = np.zeros(8, dtype=REC)
    z[:3] = b.rec[:3]
    r = send_host(b.data, z, np.array([0, 8], np.uint32), [7], H.L4, H.L6, tx, np.arange(ntx, dtype=np.uint32), buf_bytes=B)
    assert r.send.tolist() == [SEND | BUILT] * 3 + [0] * 5


def test_the_socket_is_the_range_of_q_first():
    B = 256
    b = H.case("socks1024", B)
    r, tx, free = host(b, B)
    got = [int.from_bytes(d[(20 if d[0] == 0x45 else 40):][:2], "big") for d in datagrams(r, tx, free, B)]
    assert got == [p for p, _, _, _ in b.sends] and 800 < len(set(got)) < 1024 - 52   # (the case leaves sockets empty)


@pytest.mark.parametrize("B", [256, 512])
def test_round_trip_from_the_demux(B):
    """demux_host's output fed to send_host as it is: an echo server.  Every datagram comes back with source and
    destination swapped, the same payload, from the socket's port to the sender's."""
    pkts, ports, _, _ = D.case("socks1024" if B == 256 else "two", B)
    rx, idx, blk, len16 = D.lay_pool(pkts, B, shuffled=True, seed=B)
    dm = demux_host(rx, idx, blk, len16, D.L4, D.L6, port_table(ports), len(ports), buf_bytes=B)
    n = int(dm.count[0])
    ntx = int(sum(1 + -(-int(x) // B) for x in dm.rec["len"][:n]))
    free = np.random.default_rng(B).permutation(ntx).astype(np.uint32)
    tx = np.zeros(ntx * B, dtype=np.uint8)
    r = send_host(dm.data, dm.rec, dm.q_first, ports, D.L4, D.L6, tx, free, buf_bytes=B)
    assert r.count[0] == n and (r.send[:n] == (SEND | BUILT)).all() and (r.send[n:] == 0).all()
    for d, k in zip(datagrams(r, tx, free, B), r.tx_src):
        p = pkts[int(dm.rec["src"][k])]
        v6 = (p[0] >> 4) == 6
        h = 40 if v6 else (p[0] & 0xF) * 4
        assert (d[8:24], d[24:40]) == (p[24:40], p[8:24]) if v6 else (d[12:16], d[16:20]) == (p[16:20], p[12:16])
        hd = 40 if v6 else 20
        assert d[hd:hd + 2] == p[h + 2:h + 4] and d[hd + 2:hd + 4] == p[h:h + 2] and d[hd + 8:] == p[h + 8:]


def test_workspace_size():
    assert 0 < udp_send_work(0) <= udp_send_work(1) <= udp_send_work(2 ** 20) <= 8 << 20
    assert udp_send_work(1000) <= udp_send_work(1001)
    with pytest.raises(_lib.ChecksumError):
        udp_send_work(_lib.RNS_CHAIN_MAX_PACKETS + 1)
