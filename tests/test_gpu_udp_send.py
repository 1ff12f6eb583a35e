"""rns_tx_udp_send_pool_dev on the GPU against send_host (itself pinned to the reference's restatement by
test_udp_send_ref.py) and against rns_tx_fill_pool_dev run over the same heads with zeroed checksum fields.
Every output lies between guards prefilled with 0xEE; the transmit pool is prefilled with a pattern and compared
whole, the permitted slack after a payload's end masked; the payloads, the records and every other input are
read back unchanged."""
import socket

import numpy as np
import pytest
import torch

import udp_demux_helper as D
import udp_send_helper as H
from gpu_guard import DEV, FILL, Guarded
from rustnetworkstack_amd import _lib, batch
from rustnetworkstack_amd.udp import REC, port_table, rx_udp_demux_pool, send_host, tx_udp_send_pool, udp_echo, udp_send_work
from tx_pool_helper import mask_slack

pytestmark = pytest.mark.gpu
TXFILL = 0xA5
SEND, BUILT, NOBUF, BADBUF = _lib.RNS_UDPTX_SEND, _lib.RNS_UDPTX_BUILT, _lib.RNS_UDPTX_NOBUF, _lib.RNS_UDPTX_BADBUF


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def run(b, B, *, rec=None, data=None, q_first=None, send_cap=None, n_free=None, bad_at=None, ip_id_base=0, add=0,
        add_on_device=False, fill_check=True, extra=5):
    """One call over the batch (or over its records, payloads or table changed): the outputs as numpy, everything
    compared with send_host."""
    rec = b.rec if rec is None else rec
    data = b.data if data is None else data
    q = b.q_first if q_first is None else q_first
    n = len(rec)
    ntx = b.tx_needed(B) + extra
    free = np.random.default_rng(n + B).permutation(ntx).astype(np.uint32)
    if n_free is not None:
        free = free[:n_free]
    if bad_at is not None:
        free[bad_at] = ntx + 7
    tx0 = np.full(ntx * B, TXFILL, dtype=np.uint8)
    tx0[::7] = np.arange(tx0[::7].size, dtype=np.uint8)  # a pattern: a buffer written to the wrong place shows
    cap = n if send_cap is None else send_cap
    d_tx = Guarded(tx0.size, tx0)
    ins = {"data": Guarded(data.size, data), "rec": Guarded(32 * n, rec), "q": Guarded(4 * q.size, q),
           "ports": Guarded(2 * b.ports.size, b.ports), "free": Guarded(4 * free.size, free)}
    d_add = Guarded(8, np.array([add, 0xEEEEEEEE], dtype=np.uint32)) if add_on_device else None
    assert add_on_device or add == 0
    sizes = {"send": n, "blk_first": 4 * ((cap + 63) // 64), "head_len8": cap, "pay_len16": 2 * cap, "src": 4 * cap, "count": 12}
    out = {k: Guarded(v) for k, v in sizes.items()}
    need = udp_send_work(n)
    work = Guarded(need + 8)
    ptr = lambda g: g.t.data_ptr() if g is not None and g.n else None  # noqa: E731
    keep = torch.empty(16, dtype=torch.uint8, device=DEV)              # a pointer where nothing is read
    batch._call("rns_tx_udp_send_pool_dev", torch.device(DEV), ptr(ins["data"]) or keep.data_ptr(), data.size, ptr(ins["rec"]), n,
                ptr(ins["q"]), ptr(ins["ports"]), b.ports.size, H.L4, H.L6, d_tx.t.data_ptr(), tx0.size, B.bit_length() - 1,
                ptr(ins["free"]), free.size, cap, ip_id_base, ptr(d_add), ptr(out["blk_first"]), ptr(out["head_len8"]),
                ptr(out["pay_len16"]), ptr(out["src"]), out["count"].t.data_ptr(), out["send"].t.data_ptr(), work.t.data_ptr(),
                need)
    torch.cuda.synchronize()
    work.host()
    # the same on the host
    tx_ref = tx0.copy()
    r = send_host(data, rec, q, b.ports, H.L4, H.L6, tx_ref, free, buf_bytes=B, send_cap=cap, ip_id_base=ip_id_base, ip_id_add=add)
    assert out["count"].host(np.uint32).tolist() == r.count.tolist()
    assert np.array_equal(out["send"].host(), r.send)
    for key, ref, dt in (("blk_first", r.tx_blk_first, np.uint32), ("head_len8", r.tx_head_len8, np.uint8),
                         ("pay_len16", r.tx_pay_len16, np.uint16), ("src", r.tx_src, np.uint32)):
        got = out[key].host(dt)
        assert np.array_equal(got[:len(ref)], ref), key
        assert (got[len(ref):].view(np.uint8) == FILL).all(), f"{key}: written past the datagrams"
    # the pool and the inputs
    got_tx = d_tx.host()
    mask_slack(got_tx, tx_ref, free, r.tx_blk_first, r.tx_head_len8, r.tx_pay_len16, B)
    assert np.array_equal(got_tx, tx_ref), np.nonzero(got_tx != tx_ref)[0][:8]
    for k, a in (("data", data), ("rec", rec), ("q", q), ("ports", b.ports), ("free", free)):
        assert np.array_equal(ins[k].host(), np.ascontiguousarray(a).view(np.uint8).reshape(-1)), k
    if d_add is not None:
        assert d_add.host(np.uint32).tolist() == [add, 0xEEEEEEEE]
    # and rns_tx_fill_pool_dev over the same heads with zeroed checksum fields
    nbuilt = int(r.count[0])
    if fill_check and nbuilt:
        z = tx_ref.copy()
        for fr, h in zip(H.expand_replies(free, r.tx_blk_first, r.tx_head_len8, r.tx_pay_len16, B), r.tx_head_len8.tolist()):
            if h:
                at = fr[0][0] * B + B - h
                z[at + h - 2:at + h] = 0
                if h == 28:
                    z[at + 10:at + 12] = 0
        assert not np.array_equal(z, tx_ref)
        d_z = torch.from_numpy(z).to(DEV)
        dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(DEV)  # noqa: E731
        batch.tx_fill_pool(d_z, dv(free[:int(r.count[1])], np.int32), dv(r.tx_blk_first, np.int32), dv(r.tx_head_len8, np.uint8),
                           dv(r.tx_pay_len16, np.int16), buf_bytes=B)
        assert np.array_equal(d_z.cpu().numpy(), tx_ref)
    return r, got_tx, free


def datagrams(r, tx, free, B):
    return [b"".join(tx[k * B + s:k * B + e].tobytes() for k, s, e in fr)
            for fr in H.expand_replies(free, r.tx_blk_first, r.tx_head_len8, r.tx_pay_len16, B)]


@pytest.mark.parametrize("B", [256, 512])
@pytest.mark.parametrize("name", ["lengths", "sums", "one", "socks1024"] + [f"count{n}" for n in H.COUNTS])
def test_every_send_is_built(name, B):
    b = H.case(name, B)
    r, tx, free = run(b, B, ip_id_base=7)
    assert (r.send == (SEND | BUILT)).all() and r.count[0] == len(b.sends)
    d = datagrams(r, tx, free, B)
    for x, (port, dest, dport, pay) in zip(d, b.sends):
        h = 20 if len(dest) == 4 else 40
        assert x[h:h + 4] == port.to_bytes(2, "big") + dport.to_bytes(2, "big") and x[h + 8:] == pay and x[h - len(dest):h] == dest
    if name == "sums":
        assert [x[26:28] if x[0] == 0x45 else x[46:48] for x in d[:6]] == [b"\0\0"] * 6   # a computed 0 is stored as 0


def test_the_length_fields_wrap_as_u16():
    """65507 is the largest payload whose lengths are true; past it 28 + len and 8 + len are taken mod 2^16, as the
    reference's `as u16` takes them, in the header fields and in the pseudo-header alike."""
    B = 256
    b = H.case("big", B)
    r, tx, free = run(b, B)
    assert r.count[0] == 7
    for x, (_, dest, _, pay) in zip(datagrams(r, tx, free, B), b.sends):
        h = 20 if len(dest) == 4 else 40
        assert int.from_bytes(x[h + 4:h + 6], "big") == (8 + len(pay)) & 0xFFFF and x[h + 8:] == pay
        assert int.from_bytes(x[2:4] if h == 20 else x[4:6], "big") == ((28 if h == 20 else 8) + len(pay)) & 0xFFFF


def test_at_the_scan_count():
    """One more record than 256 workgroups of 256: the scan's middle kernel loops twice."""
    b = H.case("scan", 256)
    r, _, _ = run(b, 256, ip_id_base=0xFFF0)
    assert r.count[0] == H.SCAN_N and (r.send == (SEND | BUILT)).all() and r.tx_src.tolist() == list(range(H.SCAN_N))


@pytest.mark.parametrize("on_device", [False, True])
def test_ids_wrap(on_device):
    B = 512
    b = H.case("count257", B)
    r, tx, free = run(b, B, ip_id_base=0xFFFE, add=0x10001 if on_device else 0, add_on_device=on_device)
    ids = [int.from_bytes(d[4:6], "big") for d in datagrams(r, tx, free, B) if d[0] == 0x45]
    base = 0xFFFE + (0x10001 if on_device else 0)
    assert ids == [(base + k) & 0xFFFF for k in range(len(ids))] and 0 in ids and 0 < len(ids) == r.count[2] < r.count[0]


@pytest.mark.parametrize("B", [256, 512])
def test_cuts(B):
    b = H.case("lengths", B)
    R, F = len(b.sends), b.tx_needed(B)
    last = 1 + -(-len(b.sends[-1][3]) // B)
    for cap in (0, 1, R - 1, R):
        r, _, _ = run(b, B, send_cap=cap)
        assert r.count[0] == cap and (r.send[:cap] == (SEND | BUILT)).all() and (r.send[cap:] == (SEND | NOBUF)).all()
    for nfree, nbuilt in ((F, R), (F - 1, R - 1), (F - last, R - 1), (0, 0)):
        r, _, _ = run(b, B, n_free=nfree)
        assert r.count[0] == nbuilt and (r.send[nbuilt:] == (SEND | NOBUF)).all()


@pytest.mark.parametrize("B", [256, 512])
def test_free_buffer_outside_the_pool(B):
    b = H.case("lengths", B)
    k = sum(1 + -(-len(p) // B) for _, _, _, p in b.sends[:18])  # send 18: IPv4, 2B + 1 bytes, free[k .. k + 4)
    r, _, _ = run(b, B, bad_at=k + 2)
    want = np.full(len(b.sends), SEND | BUILT, dtype=np.uint8)
    want[18] = SEND | BADBUF
    assert np.array_equal(r.send, want) and r.tx_head_len8[18] == 0 and r.count[0] == len(b.sends)


def test_what_is_no_send():
    B = 256
    b = H.case("count257", B)
    rec = b.rec.copy()
    rec["flags"][5], rec["flags"][70] = 0x03, 0x08            # not queued
    rec["family"][9], rec["family"][200] = 5, 0
    end16 = b.data.size // 16
    rec["off16"][40], rec["len"][40] = end16 - 1, 17          # its last byte is past the end
    rec["off16"][41], rec["len"][41] = end16 - 1, 16          # ends with the array: a send
    rec["off16"][42], rec["len"][42] = end16, 0               # nothing, at the end: a send
    rec["off16"][43], rec["len"][43] = end16 + 1, 0           # nothing, past the end
    rec["off16"][44], rec["len"][44] = 0xFFFFFFFF, 65535      # 64-bit arithmetic
    q = b.q_first.copy()
    q[-1] = 250                                               # n_recs = rec_cap: records 250.. are no sends
    r, _, _ = run(b, B, rec=rec, q_first=q)
    no = [5, 9, 40, 43, 44, 70, 200] + list(range(250, 257))
    assert np.nonzero(r.send == 0)[0].tolist() == no and (np.delete(r.send, no) == (SEND | BUILT)).all()
    # a payload array whose size is no multiple of 16, its last payload ending with it
    k = int(np.argmax(16 * b.rec["off16"].astype(np.int64) + b.rec["len"]))
    assert b.rec["len"][k] % 16
    r, _, _ = run(b, B, data=b.data[:16 * int(b.rec["off16"][k]) + int(b.rec["len"][k])])
    assert (r.send == (SEND | BUILT)).all()
    r, _, _ = run(b, B, data=b.data[:16 * int(b.rec["off16"][k]) + int(b.rec["len"][k]) - 1])
    assert r.send[k] == 0 and (np.delete(r.send, k) == (SEND | BUILT)).all()
    # a record array zeroed before a cut demux
    z = np.zeros(64, dtype=REC)
    z[:3] = b.rec[:3]
    r, _, _ = run(b, B, rec=z, q_first=np.array([0, 64, 64, 64], dtype=np.uint32))
    assert r.send.tolist() == [SEND | BUILT] * 3 + [0] * 61


def test_two_runs_give_the_same_pool():
    b = H.case("one", 512)
    _, a, _ = run(b, 512, fill_check=False)
    _, c, _ = run(b, 512, fill_check=False)
    assert np.array_equal(a, c)


def test_wrapper_matches_host():
    B, b = 512, H.case("one", 512)
    ntx = b.tx_needed(B)
    free = np.random.default_rng(2).permutation(ntx).astype(np.uint32)
    dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t).reshape(-1)).to(DEV)  # noqa: E731
    d_tx = torch.full((ntx * B,), TXFILL, dtype=torch.uint8, device=DEV)
    s = tx_udp_send_pool(dv(b.data, np.uint8), dv(b.rec, np.uint8), dv(b.q_first, np.int32), dv(b.ports, np.int16), H.L4, H.L6,
                         d_tx, dv(free, np.int32), buf_bytes=B, ip_id_base=3, ip_id_add=dv(np.array([4], np.uint32), np.int32))
    tx_ref = np.full(ntx * B, TXFILL, dtype=np.uint8)
    r = send_host(b.data, b.rec, b.q_first, b.ports, H.L4, H.L6, tx_ref, free, buf_bytes=B, ip_id_base=3, ip_id_add=4)
    cnt = s.count.cpu().numpy().view(np.uint32)
    n = int(cnt[0])
    assert cnt.tolist() == r.count.tolist() and np.array_equal(s.send.cpu().numpy(), r.send)
    assert np.array_equal(s.tx_head_len8.cpu().numpy()[:n], r.tx_head_len8)
    assert np.array_equal(s.tx_src.cpu().numpy().view(np.uint32)[:n], r.tx_src)
    got = d_tx.cpu().numpy()
    mask_slack(got, tx_ref, free, r.tx_blk_first, r.tx_head_len8, r.tx_pay_len16, B)
    assert np.array_equal(got, tx_ref)


@pytest.mark.parametrize("name,B", [("mixed", 256), ("socks1024", 512), ("edges", 256)])
def test_demux_then_send_on_the_device(name, B):
    """The loop closed: rx_udp_demux_pool -> tx_udp_send_pool with nothing read back in between, against the
    restated reference echoing the same datagrams (udp_recv per socket in order, udp_send back to the sender)."""
    pkts, ports, _, queues = D.case(name, B)
    rx, idx, blk, len16 = D.lay_pool(pkts, B, shuffled=True, seed=B)
    dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t).reshape(-1)).to(DEV)  # noqa: E731
    sends = [(p, ip, sport, pay) for p, q in zip(ports, queues) for ip, sport, pay in q]
    ntx = sum(1 + -(-len(s[3]) // B) for s in sends) + 2
    free = np.random.default_rng(len(pkts)).permutation(ntx).astype(np.uint32)
    d_tx = torch.full((ntx * B,), TXFILL, dtype=torch.uint8, device=DEV)
    d_rec = torch.zeros(32 * len(pkts), dtype=torch.uint8, device=DEV)
    dm = rx_udp_demux_pool(dv(rx, np.uint8), dv(idx, np.int32), dv(blk, np.int32), dv(len16, np.int16), D.L4, D.L6,
                           dv(port_table(ports), np.int16), len(ports), buf_bytes=B, rec=d_rec)
    s = tx_udp_send_pool(dm.data, dm.rec, dm.q_first, dv(np.array(ports, dtype=np.uint16), np.int16), D.L4, D.L6, d_tx,
                         dv(free, np.int32), buf_bytes=B, ip_id_base=0xFFFD)
    torch.cuda.synchronize()
    ref_tx = np.full(ntx * B, TXFILL, dtype=np.uint8)
    want, frags, ids = H.send_ref(sends, B, ref_tx, free, next_id=0xFFFD)
    cnt = s.count.cpu().numpy().view(np.uint32)
    n = len(want)
    assert cnt.tolist() == [n, ntx - 2, ids] and (s.send.cpu().numpy()[:n] == (SEND | BUILT)).all() and not s.send.cpu().numpy()[n:].any()
    r = H.expand_replies(free, s.tx_blk_first.cpu().numpy().view(np.uint32), s.tx_head_len8.cpu().numpy()[:n],
                         s.tx_pay_len16.view(torch.int16).cpu().numpy().view(np.uint16)[:n], B)
    assert r == frags
    tx = d_tx.cpu().numpy()
    assert [b"".join(tx[k * B + a:k * B + e].tobytes() for k, a, e in fr) for fr in r] == want


def test_no_records():
    cnt = Guarded(12)
    batch._call("rns_tx_udp_send_pool_dev", torch.device(DEV), None, 0, None, 0, None, None, 0, H.L4, H.L6, None, 0, 9, None, 0, 0, 0,
                None, None, None, None, None, cnt.t.data_ptr(), None, None, 0)
    torch.cuda.synchronize()
    assert cnt.host(np.uint32).tolist() == [0, 0, 0]


def test_echo_over_a_socket_pair():
    """udp_echo end to end, the transmit pool too small for one pass: what the device leaves (RNS_UDPTX_NOBUF) the
    host path sends, and every datagram the reference would answer comes back."""
    B = 512
    pkts, ports, _, queues = D.case("two", B)
    sends = [(p, ip, sport, pay) for p, q in zip(ports, queues) for ip, sport, pay in q]
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    c, d = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    try:
        for s in (a, c):
            s.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 1 << 20)
        a.setblocking(False)  # a full queue fails the test at once
        d.setblocking(False)
        for p in pkts:
            a.send(p)
        nf = [1 + -(-len(s[3]) // B) for s in sends]
        nrx, ntx = 4 * len(pkts) + 8, sum(nf) - 60
        dev_want = int(np.searchsorted(np.cumsum(nf), ntx, side="right"))  # the sends whose buffers the free list holds
        rx_pool, rx_free = np.zeros(nrx * B, dtype=np.uint8), np.random.default_rng(1).permutation(nrx).astype(np.uint32)
        tx_pool, tx_free = np.zeros(ntx * B, dtype=np.uint8), np.random.default_rng(2).permutation(ntx).astype(np.uint32)
        n, sent, udp, (entries, on_dev, on_host) = udp_echo(b.fileno(), c.fileno(), rx_pool, rx_free, tx_pool, tx_free, ports, D.L4,
                                                            D.L6, buf_bytes=B, ip_id_base=0x1234, device=DEV, timeout_ms=1000)
        assert n == len(pkts) and entries == len(sends) == sent == on_dev + on_host and on_dev == dev_want < len(sends)
        got = [d.recv(4096) for _ in range(sent)]
        want, _, _ = H.send_ref(sends, B, np.zeros((2 * len(sends)) * B, dtype=np.uint8), np.arange(2 * len(sends)), next_id=0x1234)
        assert got == want
    finally:
        for s in (a, b, c, d):
            s.close()
