"""demux_host — the numpy statement of rns_rx_udp_demux_pool_dev that the GPU tests compare with — against
the reference's UDP receive path restated in udp_demux_helper (ip_input -> udp_input -> udp_recv over
NetBuffers), on every case the GPU tests run, and against hand-written datagrams with their expected
queues (tests/golden/udp_demux_kats.json).  No GPU."""
import json
import os

import numpy as np
import pytest

import udp_demux_helper as H
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.udp import NO_POS, REC, demux_host, demux_work, drain, port_table

DGRAM, SOCK, QUEUED, NOROOM = _lib.RNS_UDP_DGRAM, _lib.RNS_UDP_SOCK, _lib.RNS_UDP_QUEUED, _lib.RNS_UDP_NOROOM
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "udp_demux_kats.json")


def host(pkts, ports, B, **kw):
    rx, idx, blk, len16 = H.lay_pool(pkts, B, shuffled=True, seed=len(pkts) + B)
    return demux_host(rx, idx, blk, len16, H.L4, H.L6, port_table(ports), len(ports), buf_bytes=B, **kw)


def check_layout(r, n_socks):
    """The contract's own invariants: socket-major positions, units in the same order, pos inverted = src."""
    q, udp, pos = r.q_first.astype(np.int64), r.udp, r.pos
    assert q[0] == 0 and (np.diff(q) >= 0).all() and q[n_socks] == r.count[0]
    has = (udp & SOCK) != 0
    assert ((udp[has] & (QUEUED | NOROOM)) != 0).all() and ((udp[~has] & (QUEUED | NOROOM | SOCK)) == 0).all()
    queued = (udp & QUEUED) != 0
    assert (pos[~queued] == NO_POS).all()
    ks = pos[queued].astype(np.int64)
    assert len(set(ks.tolist())) == len(ks)
    rec = r.rec[ks]
    assert np.array_equal(rec["src"], np.nonzero(queued)[0]) and np.array_equal(rec["flags"], udp[queued])
    assert (rec["pad"] == 0).all()
    order = np.argsort(ks)
    units = -(-rec["len"][order].astype(np.int64) // 16)
    off = rec["off16"][order].astype(np.int64)
    if len(off) and not (udp & NOROOM).any():
        assert off[0] == 0 and np.array_equal(off[1:], np.cumsum(units)[:-1]) and off[-1] + units[-1] == r.count[1]
    for s in range(n_socks):
        src = r.rec["src"][q[s]:q[s + 1]] if not (udp & NOROOM).any() else []
        assert list(src) == sorted(src)


@pytest.mark.parametrize("B", [128, 512])
@pytest.mark.parametrize("name", H.CASE_NAMES)
def test_host_equals_the_reference(name, B):
    pkts, ports, st, queues = H.case(name, B)
    r = host(pkts, ports, B)
    assert r.status.tolist() == st
    assert [drain(r, s) for s in range(len(ports))] == queues
    assert not (r.udp & NOROOM).any() and r.count[0] == sum(len(q) for q in queues)
    check_layout(r, len(ports))


def test_host_equals_the_reference_at_the_scan_count():
    pkts, ports, st, queues = H.case("scan", 128)
    r = host(pkts, ports, 128)
    assert r.status.tolist() == st and [drain(r, s) for s in range(len(ports))] == queues
    check_layout(r, len(ports))


def test_what_the_mixed_batch_queues():
    pkts, ports, _, queues = H.case("mixed", 512)
    r = host(pkts, ports, 512)
    # the first datagram and every second one after it are UDP to a bound port; of the others only the
    # unbound ports, the short segments and nothing else are UDP at all
    assert ((r.udp[0::2] & QUEUED) != 0).all() and ((r.udp[1::2] & SOCK) == 0).all()
    assert sum(len(q) for q in queues) == (len(pkts) + 1) // 2
    undelivered = [i for i in range(1, len(pkts), 2) if r.udp[i] == DGRAM]
    assert len(undelivered) == 2  # ports 601 and 599


def test_golden_datagrams():
    with open(GOLDEN) as f:
        g = json.load(f)
    pkts = [bytes.fromhex(h) for h in g["datagrams"]]
    l4, l6 = bytes.fromhex(g["local_ipv4"]), bytes.fromhex(g["local_ipv6"])
    for B in (128, 512):
        rx, idx, blk, len16 = H.lay_pool(pkts, B, shuffled=True, seed=3)
        r = demux_host(rx, idx, blk, len16, l4, l6, port_table(g["ports"]), len(g["ports"]), buf_bytes=B)
        assert r.udp.tolist() == g["udp"]
        for s, port in enumerate(g["ports"]):
            want = [(bytes.fromhex(a), sp, bytes.fromhex(p)) for a, sp, p in g["queues"][str(port)]]
            assert drain(r, s) == want, port


def test_cuts_on_the_host():
    pkts, ports, _, queues = H.case("two", 512)
    full = host(pkts, ports, 512)
    E, U = int(full.count[0]), int(full.count[1])
    order = np.argsort(full.pos[(full.udp & QUEUED) != 0])
    src = np.nonzero(full.udp & QUEUED)[0][order]          # the entries' datagrams by position
    for cap in (0, 1, E - 1, E):
        r = host(pkts, ports, 512, rec_cap=cap)
        assert r.count.tolist() == [E, U] and np.array_equal(r.q_first, full.q_first)
        assert ((r.udp[src[:cap]] & QUEUED) != 0).all() and (r.udp[src[cap:]] == (DGRAM | SOCK | NOROOM)).all()
        assert (r.pos[src[cap:]] == NO_POS).all()
    # data one unit short of the last entry with payload, and of a middle one: what does not fit is cut,
    # zero-length entries and shorter ones behind it are not
    with_units = [k for k in range(E) if full.rec["len"][k] > 0]
    for k in (with_units[-1], with_units[len(with_units) // 2]):
        end = int(full.rec["off16"][k]) + -(-int(full.rec["len"][k]) // 16)
        r = host(pkts, ports, 512, data=np.zeros(16 * (end - 1), dtype=np.uint8))
        assert r.count.tolist() == [E, U]
        for j in range(E):
            fits = 16 * (int(full.rec["off16"][j]) + -(-int(full.rec["len"][j]) // 16)) <= 16 * (end - 1)
            assert bool(r.udp[src[j]] & QUEUED) == fits and bool(r.udp[src[j]] & NOROOM) == (not fits)
        assert r.udp[src[k]] & NOROOM
        # a drained queue ends at its first cut entry
        for s in range(len(ports)):
            d = drain(r, s)
            assert d == queues[s][:len(d)]


def test_no_sockets_and_no_datagrams():
    pkts, _, _, _ = H.case("two", 512)
    r = host(pkts, [], 512)
    assert r.count.tolist() == [0, 0] and r.q_first.tolist() == [0] and set(r.udp.tolist()) == {DGRAM}
    r = demux_host(np.zeros(0, np.uint8), [], [], [], H.L4, H.L6, port_table([7]), 1)
    assert r.count.tolist() == [0, 0] and r.q_first.tolist() == [0, 0] and drain(r, 0) == []


def test_port_table():
    t = port_table([80, 65535, 0])
    assert t.dtype == np.uint16 and t.shape == (65536,)
    assert t[80] == 0 and t[65535] == 1 and t[0] == 2 and (np.delete(t, [0, 80, 65535]) == _lib.RNS_UDP_NO_SOCK).all()
    assert (port_table([]) == _lib.RNS_UDP_NO_SOCK).all()
    with pytest.raises(_lib.ChecksumError):
        port_table([5, 6, 5])                          # udp_open: "Port already in use"
    with pytest.raises(_lib.ChecksumError):
        port_table(list(range(_lib.RNS_UDP_MAX_SOCKS + 1)))
    assert len(port_table(list(range(_lib.RNS_UDP_MAX_SOCKS)))) == 65536


def test_workspace_size():
    assert 0 < demux_work(0, 0) <= demux_work(1, 1) <= demux_work(2 ** 20, 1024) <= 64 << 20
    assert demux_work(1000, 3) <= demux_work(1001, 3) <= demux_work(1001, 4)
    assert REC.itemsize == 32
