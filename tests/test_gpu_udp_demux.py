"""rns_rx_udp_demux_pool_dev on the GPU against demux_host (itself pinned to the reference's restatement by
test_udp_demux_ref.py, on these same cases).  Every array lies between guards prefilled with 0xEE; d_data and
d_rec are prefilled and compared whole, the permitted slack after a payload's end masked; the pool and the
inputs are read back unchanged."""
import socket

import numpy as np
import pytest
import torch

import udp_demux_helper as H
from gpu_guard import DEV, FILL, Guarded
from rustnetworkstack_amd import _lib, batch
from rustnetworkstack_amd.udp import NO_POS, REC, UdpDemux, demux_host, demux_work, drain, port_table, rx_udp_demux_pool, udp_demux

pytestmark = pytest.mark.gpu
DATAFILL, RECFILL = 0xA5, 0x5A
DGRAM, SOCK, QUEUED, NOROOM = _lib.RNS_UDP_DGRAM, _lib.RNS_UDP_SOCK, _lib.RNS_UDP_QUEUED, _lib.RNS_UDP_NOROOM


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def mask_slack(data, ref, r):
    """The bytes an entry may leave unspecified — from its payload's end to the next 16-byte boundary of its
    own range — copied from ref into data."""
    for rec in r.rec[r.pos[(r.udp & QUEUED) != 0]]:
        e = 16 * int(rec["off16"]) + int(rec["len"])
        data[e:(e + 15) & ~15] = ref[e:(e + 15) & ~15]


def run(pkts, ports, B, *, rec_cap=None, data_bytes=None, n_socks=None, datafill=DATAFILL, recfill=RECFILL, with_pos=True,
        tbl=None, drop_frags=0):
    """One call over the datagrams: the outputs as a UdpDemux of numpy arrays, everything compared with demux_host.
    `tbl`: a table other than the ports'; `drop_frags`: that many entries fewer of d_buf_idx than the batch names."""
    rx, idx, blk, len16 = H.lay_pool(pkts, B, shuffled=True, seed=len(pkts) + B)
    idx = idx[:idx.size - drop_frags]
    n, ns = len(pkts), len(ports) if n_socks is None else n_socks
    tbl = port_table(ports) if tbl is None else tbl
    cap = n if rec_cap is None else rec_cap
    nbytes = idx.size * B if data_bytes is None else data_bytes
    d_rx = Guarded(rx.size, rx)
    ins = {"idx": Guarded(4 * idx.size, idx), "blk": Guarded(4 * blk.size, blk), "len16": Guarded(2 * n, len16),
           "tbl": Guarded(2 * 65536, tbl)}
    d_data, d_rec = Guarded(nbytes, fill=datafill), Guarded(32 * cap, fill=recfill)
    sizes = {"status": n, "l4": 2 * n, "udp": n, "pos": 4 * n, "q_first": 4 * (ns + 1), "count": 8}
    out = {k: Guarded(v) for k, v in sizes.items()}
    need = demux_work(n, ns)
    work = Guarded(need + 16)
    ptr = lambda g: g.t.data_ptr() if g is not None and g.n else None  # noqa: E731
    batch._call("rns_rx_udp_demux_pool_dev", torch.device(DEV), d_rx.t.data_ptr(), rx.size, B.bit_length() - 1, ptr(ins["idx"]),
                idx.size, ptr(ins["blk"]), ptr(ins["len16"]), n, H.L4, H.L6, ptr(ins["tbl"]) if ns else None, ns, ptr(d_data),
                nbytes, ptr(d_rec), cap, out["q_first"].t.data_ptr(), out["count"].t.data_ptr(), out["status"].t.data_ptr(),
                out["l4"].t.data_ptr(), out["udp"].t.data_ptr(), ptr(out["pos"]) if with_pos else None, work.t.data_ptr(), need)
    torch.cuda.synchronize()
    work.host()
    # the same on the host, into the same prefill
    data_ref, rec_ref = np.full(nbytes, datafill, dtype=np.uint8), np.full(32 * cap, recfill, dtype=np.uint8).view(REC)
    e = demux_host(rx, idx, blk, len16, H.L4, H.L6, tbl, ns, buf_bytes=B, rec_cap=cap, data=data_ref, rec=rec_ref)
    assert out["count"].host(np.uint32).tolist() == e.count.tolist()
    assert np.array_equal(out["q_first"].host(np.uint32), e.q_first)
    assert np.array_equal(out["status"].host(), e.status) and np.array_equal(out["l4"].host(np.uint16), e.l4_sum)
    got_udp = out["udp"].host()
    assert np.array_equal(got_udp, e.udp), np.nonzero(got_udp != e.udp)[0][:8]
    got_pos = out["pos"].host(np.uint32)
    assert np.array_equal(got_pos, e.pos) if with_pos else (got_pos.view(np.uint8) == FILL).all()
    got_rec = d_rec.host()
    assert np.array_equal(got_rec, rec_ref.view(np.uint8)), np.nonzero(got_rec != rec_ref.view(np.uint8))[0][:8] // 32
    got_data = d_data.host()
    mask_slack(got_data, data_ref, e)
    assert np.array_equal(got_data, data_ref), np.nonzero(got_data != data_ref)[0][:8]
    # the pool and the inputs
    assert np.array_equal(d_rx.host(), rx)
    for k, a in (("idx", idx), ("blk", blk), ("len16", len16), ("tbl", tbl)):
        assert np.array_equal(ins[k].host(a.dtype), a), k
    return UdpDemux(e.status, e.l4_sum, got_udp, e.pos, got_rec.view(REC), e.q_first, e.count, got_data)


@pytest.mark.parametrize("B", [128, 512])
@pytest.mark.parametrize("name", H.CASE_NAMES)
def test_queues_equal_the_reference(name, B):
    """Counts 63 .. 513 around the wave, the scan block and the tile; one socket, two interleaved, 64 within a
    wave, 1024 with empty ones and ones first hit in a late tile; payloads 0 / 1 / 15 / 16 / 17 and ending at a
    buffer's end; 65535-byte datagrams; the mixed batch."""
    pkts, ports, _, queues = H.case(name, B)
    r = run(pkts, ports, B)
    assert [drain(r, s) for s in range(len(ports))] == queues
    assert not (r.udp & NOROOM).any()
    # d_pos, inverted, is the records' src
    queued = np.nonzero(r.udp & QUEUED)[0]
    assert np.array_equal(r.rec["src"][r.pos[queued]], queued) and (r.pos[(r.udp & QUEUED) == 0] == NO_POS).all()


def test_only_udp_to_bound_ports_is_queued():
    pkts, ports, _, queues = H.case("mixed", 512)
    r = run(pkts, ports, 512, with_pos=False)
    assert ((r.udp[0::2] & QUEUED) != 0).all() and ((r.udp[1::2] & SOCK) == 0).all()
    assert int(r.count[0]) == (len(pkts) + 1) // 2 == sum(len(q) for q in queues)


def test_scan_with_more_than_256_parts():
    """1024 sockets over 65 tiles: 66560 counts, 260 parts, so the scan's middle kernel loops twice."""
    pkts, ports, _, queues = H.case("scan", 128)
    r = run(pkts, ports, 128)
    assert int(r.count[0]) == H.SCAN_N and [drain(r, s) for s in (0, 511, 1023)] == [queues[0], queues[511], queues[1023]]


@pytest.mark.parametrize("B", [128, 512])
def test_cuts(B):
    pkts, ports, _, queues = H.case("two", B)
    full = run(pkts, ports, B)
    E, U = int(full.count[0]), int(full.count[1])
    for cap in (0, 1, E - 1, E):
        r = run(pkts, ports, B, rec_cap=cap)
        assert r.count.tolist() == [E, U] and int(((r.udp & QUEUED) != 0).sum()) == cap
        assert int(((r.udp & NOROOM) != 0).sum()) == E - cap
    # data one unit short of the last entry with payload, and of a middle socket's entry
    with_units = [k for k in range(E) if full.rec["len"][k] > 0]
    mid = [k for k in with_units if k < int(full.q_first[1])]
    for k in (with_units[-1], mid[len(mid) // 2]):
        end = int(full.rec["off16"][k]) + -(-int(full.rec["len"][k]) // 16)
        r = run(pkts, ports, B, data_bytes=16 * (end - 1))
        assert r.count.tolist() == [E, U] and r.udp[full.rec["src"][k]] == DGRAM | SOCK | NOROOM
        for s in range(len(ports)):
            d = drain(r, s)
            assert d == queues[s][:len(d)]
    r = run(pkts, ports, B, data_bytes=0, rec_cap=E)  # only the zero-length entries at offset 0 fit
    assert all(full.rec["len"][full.pos[i]] == 0 and full.rec["off16"][full.pos[i]] == 0 for i in np.nonzero(r.udp & QUEUED)[0])


def test_no_sockets():
    pkts, _, _, _ = H.case("two", 512)
    r = run(pkts, [], 512)
    assert r.count.tolist() == [0, 0] and set(r.udp.tolist()) == {DGRAM}


def test_whatever_the_table_and_the_descriptors_hold():
    """Table entries at or past n_socks are unbound ports, whatever they are; datagrams whose buffers lie past
    n_frags are malformed to the verify and queue nothing.  run() finds every guard intact."""
    pkts, ports, _, queues = H.case("two", 512)
    r = run(pkts, ports, 512, n_socks=1)                     # the second socket is past n_socks
    assert drain(r, 0) == queues[0] and int(r.count[0]) == len(queues[0])
    assert int((r.udp == DGRAM).sum()) > len(queues[1])
    tbl = np.random.default_rng(5).integers(0, 2048, 65536).astype(np.uint16)   # half of all ports bound, to any socket
    r = run(pkts, ports, 512, tbl=tbl, n_socks=1024)
    assert 0 < int(r.count[0]) == int(((r.udp & SOCK) != 0).sum())
    r = run(pkts, ports, 512, drop_frags=40)
    assert (r.status[-40:] == _lib.RNS_RX_MALFORMED).all() and (r.udp[-40:] == 0).all() and int(r.count[0]) > 100


def test_no_datagrams():
    cnt, q = Guarded(8), Guarded(4 * 4)
    batch._call("rns_rx_udp_demux_pool_dev", torch.device(DEV), None, 0, 9, None, 0, None, None, 0, H.L4, H.L6, None, 3, None, 0,
                None, 0, q.t.data_ptr(), cnt.t.data_ptr(), None, None, None, None, None, 0)
    torch.cuda.synchronize()
    assert cnt.host(np.uint32).tolist() == [0, 0] and q.host(np.uint32).tolist() == [0, 0, 0, 0]


def test_the_same_bytes_on_every_run():
    """The 1024-socket case twice into differently prefilled outputs: every specified byte is equal."""
    pkts, ports, _, _ = H.case("socks1024", 512)
    a = run(pkts, ports, 512, datafill=0x11, recfill=0x22)
    b = run(pkts, ports, 512, datafill=0xCC, recfill=0xDD)
    assert np.array_equal(a.udp, b.udp) and np.array_equal(a.rec.view(np.uint8), b.rec.view(np.uint8))
    for rec in a.rec[:int(a.count[0])]:
        at = 16 * int(rec["off16"])
        assert np.array_equal(a.data[at:at + int(rec["len"])], b.data[at:at + int(rec["len"])])


def test_wrapper_matches_host():
    B = 512
    pkts, ports, _, queues = H.case("socks1024", B)
    rx, idx, blk, len16 = H.lay_pool(pkts, B, shuffled=True, seed=9)
    dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(DEV)  # noqa: E731
    tbl = port_table(ports)
    r = rx_udp_demux_pool(dv(rx, np.uint8), dv(idx, np.int32), dv(blk, np.int32), dv(len16, np.int16), H.L4, H.L6,
                          dv(tbl, np.int16), len(ports), buf_bytes=B)
    e = demux_host(rx, idx, blk, len16, H.L4, H.L6, tbl, len(ports), buf_bytes=B)
    E = int(e.count[0])
    assert r.count.cpu().numpy().view(np.uint32).tolist() == e.count.tolist()
    assert np.array_equal(r.status.cpu().numpy(), e.status) and np.array_equal(r.udp.cpu().numpy()[:len(pkts)], e.udp)
    assert np.array_equal(r.pos.cpu().numpy().view(np.uint32)[:len(pkts)], e.pos)
    assert np.array_equal(r.q_first.cpu().numpy().view(np.uint32), e.q_first)
    assert np.array_equal(r.rec.cpu().numpy()[:32 * E], e.rec[:E].view(np.uint8))
    assert [drain(r, s) for s in range(len(ports))] == queues


def test_loopback_over_a_socket_pair():
    B = 512
    names = ("mixed", "lengths", "unread")  # 84 datagrams: within any AF_UNIX queue length
    ports = sorted({p for nm in names for p in H.case(nm, B)[1]})
    pkts = [p for nm in names for p in H.case(nm, B)[0] if 0 < len(p) <= 2048]
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    try:
        a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 1 << 20)
        a.setblocking(False)  # a full queue fails the test at once
        for p in pkts:
            a.send(p)
        nrx = 4 * len(pkts) + 8
        pool, free = np.zeros(nrx * B, dtype=np.uint8), np.random.default_rng(1).permutation(nrx).astype(np.uint32)
        n, r = udp_demux(b.fileno(), pool, free, ports, H.L4, H.L6, buf_bytes=B, device=DEV, timeout_ms=1000)
        _, stack = H.demux_ref(pkts, B, ports)
        assert n == len(pkts) and [drain(r, s) for s in range(len(ports))] == H.queues_ref(stack, ports)
        assert int(r.count[0]) == int(((r.udp & QUEUED) != 0).sum()) > 50
    finally:
        a.close()
        b.close()
