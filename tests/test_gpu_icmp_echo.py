"""rns_rx_icmp_echo_pool_dev on the GPU against echo_host (itself pinned to the reference's restatement
by test_icmp_echo_ref.py) and against rns_tx_fill_pool_dev run over the same heads with zeroed checksum
fields.  Every output lies between guards prefilled with 0xEE; the transmit pool is prefilled and
compared whole, the permitted slack after a payload's end masked; the receive pool and the inputs are
read back unchanged."""
import socket

import numpy as np
import pytest
import torch

import icmp_echo_helper as H
from gpu_guard import DEV, FILL, Guarded
from rustnetworkstack_amd import _lib, batch
from rustnetworkstack_amd.icmp import echo_host, echo_respond, echo_work, rx_icmp_echo_pool
from tx_pool_helper import mask_slack

pytestmark = pytest.mark.gpu
TXFILL = 0xA5
BUILT, NOBUF, BADBUF, REQ = _lib.RNS_ECHO_BUILT, _lib.RNS_ECHO_NOBUF, _lib.RNS_ECHO_BADBUF, _lib.RNS_ECHO_REQUEST
_CASES = {}


def cases(B):
    if B not in _CASES:
        _CASES[B] = H.cases(B)
    return _CASES[B]


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def tx_needed(pkts, B):
    return sum(1 + -(-len(p) // B) for p in pkts)


def run(pkts, B, *, reply_cap=None, n_free=None, bad_at=None, ip_id_base=0, add=0, add_on_device=False, same_pool=False,
        fill_check=True):
    """One call over the datagrams: the outputs as numpy, everything compared with echo_host."""
    rx, idx, blk, len16 = H.lay_pool(pkts, B, shuffled=True, seed=len(pkts) + B)
    n, nrx = len(pkts), rx.size // B
    ntx = tx_needed(pkts, B) + 5
    free = np.random.default_rng(n).permutation(ntx).astype(np.uint32)
    if n_free is not None:
        free = free[:n_free]
    if bad_at is not None:
        free[bad_at] = ntx + 7
    tx0 = np.full(ntx * B, TXFILL, dtype=np.uint8)
    if same_pool:
        tx0, free = np.concatenate([rx, tx0]), free + np.uint32(nrx)
    cap = n if reply_cap is None else reply_cap
    # the device call
    d_tx = Guarded(tx0.size, tx0)
    d_rx = d_tx if same_pool else Guarded(rx.size, rx)
    ins = {"idx": Guarded(4 * idx.size, idx), "blk": Guarded(4 * blk.size, blk), "len16": Guarded(2 * n, len16),
           "free": Guarded(4 * free.size, free)}
    d_add = Guarded(8, np.array([add, 0xEEEEEEEE], dtype=np.uint32)) if add_on_device else None
    assert add_on_device or add == 0
    sizes = {"status": n, "l4": 2 * n, "echo": n, "blk_first": 4 * ((cap + 63) // 64), "head_len8": cap, "pay_len16": 2 * cap,
             "src": 4 * cap, "count": 12}
    out = {k: Guarded(v) for k, v in sizes.items()}
    need = echo_work(n)
    work = Guarded(need + 8)
    ptr = lambda g: g.t.data_ptr() if g is not None and g.n else None  # noqa: E731
    rx_bytes = nrx * B if same_pool else rx.size
    batch._call("rns_rx_icmp_echo_pool_dev", torch.device(DEV), d_rx.t.data_ptr(), rx_bytes, B.bit_length() - 1, ptr(ins["idx"]),
                idx.size, ptr(ins["blk"]), ptr(ins["len16"]), n, H.L4, H.L6, d_tx.t.data_ptr(), tx0.size, ptr(ins["free"]),
                free.size, cap, ip_id_base, ptr(d_add), ptr(out["blk_first"]), ptr(out["head_len8"]), ptr(out["pay_len16"]),
                ptr(out["src"]), out["count"].t.data_ptr(), out["status"].t.data_ptr(), out["l4"].t.data_ptr(),
                out["echo"].t.data_ptr(), work.t.data_ptr(), need)
    torch.cuda.synchronize()
    work.host()
    # the same on the host
    tx_ref = tx0.copy()
    e = echo_host(tx_ref[:nrx * B] if same_pool else rx, idx, blk, len16, H.L4, H.L6, tx_ref, free, buf_bytes=B,
                  reply_cap=cap, ip_id_base=ip_id_base, ip_id_add=add)
    st, l4, echo, bf, hl, pl, src, cnt = e
    got_cnt = out["count"].host(np.uint32)
    assert got_cnt.tolist() == cnt.tolist()
    nrep = int(cnt[0])
    assert np.array_equal(out["status"].host(), st) and np.array_equal(out["l4"].host(np.uint16), l4)
    assert np.array_equal(out["echo"].host(), echo)
    for key, ref, dt in (("blk_first", bf, np.uint32), ("head_len8", hl, np.uint8), ("pay_len16", pl, np.uint16),
                         ("src", src, np.uint32)):
        got = out[key].host(dt)
        assert np.array_equal(got[:len(ref)], ref), key
        assert (got[len(ref):].view(np.uint8) == FILL).all(), f"{key}: written past the replies"
    # the pools and the inputs
    got_tx = d_tx.host()
    mask_slack(got_tx, tx_ref, free, bf, hl, pl, B)
    assert np.array_equal(got_tx, tx_ref), np.nonzero(got_tx != tx_ref)[0][:8]
    if not same_pool:
        assert np.array_equal(d_rx.host(), rx)
    for k, a in (("idx", idx), ("blk", blk), ("len16", len16), ("free", free)):
        assert np.array_equal(ins[k].host(a.dtype), a), k
    if d_add is not None:
        assert d_add.host(np.uint32).tolist() == [add, 0xEEEEEEEE]
    # and rns_tx_fill_pool_dev over the same heads with zeroed checksum fields
    if fill_check and nrep:
        z = tx_ref.copy()
        for fr, h in zip(H.expand_replies(free, bf, hl, pl, B), hl.tolist()):
            if h:
                at = fr[0][0] * B + B - h
                z[at + h - 2:at + h] = 0
                if h == 24:
                    z[at + 10:at + 12] = 0
        d_z = torch.from_numpy(z).to(DEV)
        dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(DEV)  # noqa: E731
        batch.tx_fill_pool(d_z, dv(free[:int(cnt[1])], np.int32), dv(bf, np.int32), dv(hl, np.uint8), dv(pl, np.int16),
                           buf_bytes=B)
        assert np.array_equal(d_z.cpu().numpy(), tx_ref)
    return {"echo": echo, "count": cnt, "tx": got_tx, "free": free, "blk_first": bf, "head_len8": hl, "pay_len16": pl,
            "src": src}


def replies(r, B):
    rows = r["tx"]
    return [b"".join(rows[k * B + s:k * B + e].tobytes() for k, s, e in fr)
            for fr in H.expand_replies(r["free"], r["blk_first"], r["head_len8"], r["pay_len16"], B)]


@pytest.mark.parametrize("B", [256, 512])
@pytest.mark.parametrize("name", ["lengths", "ihl", "big", "code"])
def test_every_request_is_answered(name, B):
    pkts = cases(B)[name]
    r = run(pkts, B, ip_id_base=7)
    assert (r["echo"] == (REQ | BUILT)).all() and r["count"][0] == len(pkts)
    for p, d in zip(pkts, replies(r, B)):
        v6 = (p[0] >> 4) == 6
        h = 40 if v6 else (p[0] & 0xF) * 4
        assert d[(40 if v6 else 20):][:2] == bytes([129 if v6 else 0, 0])      # the code is not echoed
        assert d[(44 if v6 else 24):] == p[h + 4:]                             # IPv4 options are dropped
        assert (d[8:24] == H.L6 and d[24:40] == p[8:24]) if v6 else (d[12:16] == H.L4 and d[16:20] == p[12:16])


@pytest.mark.parametrize("B", [256, 512])
def test_checksum_representations(B):
    pkts = cases(B)["sums"]
    r = run(pkts, B)
    d = replies(r, B)
    assert r["count"][0] == len(pkts)
    assert [x[22:24] for x in d[0:6:2]] == [b"\xff\xff"] * 3       # IPv4, all-zero payloads: stored 0xffff
    for k in (6, 10):                                              # words summing to 0xffff: stored 0x0000
        assert d[k][22:24] == d[k + 1][22:24] == b"\0\0" and d[k + 2][42:44] == d[k + 3][42:44] == b"\0\0"
        assert len(d[k + 1]) & 1 and len(d[k + 3]) & 1             # the odd-length twins


@pytest.mark.parametrize("B", [256, 512])
def test_what_is_not_answered(B):
    pkts = cases(B)["rejects"]
    r = run(pkts, B)
    assert (r["echo"][0::2] == (REQ | BUILT)).all() and (r["echo"][1::2] == 0).all()
    assert r["src"].tolist() == list(range(0, len(pkts), 2))


@pytest.mark.parametrize("B", [256, 512])
@pytest.mark.parametrize("on_device", [False, True])
def test_mixed_batch_ids_wrap(B, on_device):
    pkts = cases(B)["mixed"]
    r = run(pkts, B, ip_id_base=0xFFFE, add=0x10001 if on_device else 0, add_on_device=on_device)
    assert r["count"][0] > 64 and len(r["blk_first"]) >= 2 and 0 < r["count"][2] < r["count"][0]
    ids = [int.from_bytes(d[4:6], "big") for d in replies(r, B) if d[0] == 0x45]
    base = 0xFFFE + (0x10001 if on_device else 0)
    assert ids == [(base + k) & 0xFFFF for k in range(len(ids))] and 0 in ids and len(ids) == r["count"][2]


def test_wrapper_matches_host():
    B, pkts = 512, cases(512)["mixed"]
    rx, idx, blk, len16 = H.lay_pool(pkts, B, shuffled=True, seed=9)
    ntx = tx_needed(pkts, B)
    free = np.random.default_rng(2).permutation(ntx).astype(np.uint32)
    dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(DEV)  # noqa: E731
    d_tx = torch.full((ntx * B,), TXFILL, dtype=torch.uint8, device=DEV)
    out = rx_icmp_echo_pool(dv(rx, np.uint8), dv(idx, np.int32), dv(blk, np.int32), dv(len16, np.int16), H.L4, H.L6, d_tx,
                            dv(free, np.int32), buf_bytes=B, ip_id_base=3, ip_id_add=dv(np.array([4], np.uint32), np.int32))
    tx_ref = np.full(ntx * B, TXFILL, dtype=np.uint8)
    e = echo_host(rx, idx, blk, len16, H.L4, H.L6, tx_ref, free, buf_bytes=B, ip_id_base=3, ip_id_add=4)
    cnt = out[7].cpu().numpy().view(np.uint32)
    assert cnt.tolist() == e[7].tolist()
    nrep = int(cnt[0])
    assert np.array_equal(out[0].cpu().numpy(), e[0]) and np.array_equal(out[2].cpu().numpy()[:len(pkts)], e[2])
    assert np.array_equal(out[4].cpu().numpy()[:nrep], e[4]) and np.array_equal(out[6].cpu().numpy().view(np.uint32)[:nrep], e[6])
    got = d_tx.cpu().numpy()
    mask_slack(got, tx_ref, free, e[3], e[4], e[5], B)
    assert np.array_equal(got, tx_ref)


@pytest.mark.parametrize("B", [256, 512])
def test_cuts(B):
    pkts = cases(B)["lengths"]
    R, F = len(pkts), tx_needed([p[(44 if p[0] >> 4 == 6 else 24):] for p in pkts], B)
    last = 1 + -(-(len(pkts[-1]) - 44) // B)
    for cap in (0, 1, R, R - 1):
        r = run(pkts, B, reply_cap=cap)
        assert r["count"][0] == cap and (r["echo"][:cap] == (REQ | BUILT)).all() and (r["echo"][cap:] == (REQ | NOBUF)).all()
    for nfree, nrep in ((F, R), (F - 1, R - 1), (F - last, R - 1), (0, 0)):
        r = run(pkts, B, n_free=nfree)
        assert r["count"][0] == nrep and (r["echo"][nrep:] == (REQ | NOBUF)).all()


@pytest.mark.parametrize("B", [256, 512])
def test_free_buffer_outside_the_pool(B):
    pkts = cases(B)["lengths"]
    # reply 22 (IPv4, 2B + 1 payload bytes) holds free[k .. k + 4): its second payload buffer is outside
    k = tx_needed([p[(44 if p[0] >> 4 == 6 else 24):] for p in pkts[:22]], B)
    r = run(pkts, B, bad_at=k + 2)
    want = np.full(len(pkts), REQ | BUILT, dtype=np.uint8)
    want[22] = REQ | BADBUF
    assert np.array_equal(r["echo"], want) and r["head_len8"][22] == 0 and r["count"][0] == len(pkts)


@pytest.mark.parametrize("B", [256, 512])
def test_both_pools_in_one(B):
    r = run(cases(B)["ihl"], B, same_pool=True, fill_check=False)
    assert (r["echo"] == (REQ | BUILT)).all()


@pytest.mark.parametrize("n", [255, 256, 257, 65537])
def test_scan_block_boundaries(n):
    """The scan under the responder at its block boundaries: n 84-byte pings, IPv4 and IPv6 alternating (the
    scan's components differ), one workgroup short by one, one, one more, and one more than 256 workgroups
    (the middle kernel's loop runs twice).  run() compares every output with echo_host; at the three small
    counts the replies are also the restated reference's (respond_ref is a Python object per buffer: at
    65537 it would take most of a minute, and echo_host is pinned to it by test_icmp_echo_ref.py)."""
    B = 256
    kinds = [H.ping4(H.body(k, 60)) if k % 2 == 0 else H.ping6(H.body(k, 40)) for k in range(16)]
    assert all(len(p) == 84 for p in kinds)
    pkts = [kinds[i % 16] for i in range(n)]
    r = run(pkts, B, ip_id_base=0xFFF0)
    assert (r["echo"] == (REQ | BUILT)).all() and r["count"].tolist() == [n, 2 * n, (n + 1) // 2]
    assert r["src"].tolist() == list(range(n))
    if n <= 257:
        ntx = tx_needed(pkts, B) + 5
        ans, ref, _, _ = H.respond_ref(pkts, B, np.full(ntx * B, TXFILL, dtype=np.uint8), r["free"], next_id=0xFFF0)
        assert all(ans) and replies(r, B) == H.reply_datagrams(ref)


def test_no_datagrams():
    cnt = Guarded(12)
    batch._call("rns_rx_icmp_echo_pool_dev", torch.device(DEV), None, 0, 9, None, 0, None, None, 0, H.L4, H.L6, None, 0, None, 0,
                0, 0, None, None, None, None, None, cnt.t.data_ptr(), None, None, None, None, 0)
    torch.cuda.synchronize()
    assert cnt.host(np.uint32).tolist() == [0, 0, 0]


def test_loopback_over_a_socket_pair():
    B = 512
    pkts = [p for p in cases(B)["rejects"] + cases(B)["lengths"] if 0 < len(p) <= 2048]
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    c, d = socket.socketpair(socket.AF_UNIX, socket.SOCK_DGRAM)
    try:
        for s in (a, c):
            s.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 1 << 20)
        a.setblocking(False)  # a full queue fails the test at once
        d.setblocking(False)
        for p in pkts:
            a.send(p)
        nrx, ntx = 4 * len(pkts) + 8, tx_needed(pkts, B) + 3
        rx_pool, rx_free = np.zeros(nrx * B, dtype=np.uint8), np.random.default_rng(1).permutation(nrx).astype(np.uint32)
        tx_pool, tx_free = np.zeros(ntx * B, dtype=np.uint8), np.random.default_rng(2).permutation(ntx).astype(np.uint32)
        n, sent, echo, cnt = echo_respond(b.fileno(), c.fileno(), rx_pool, rx_free, tx_pool, tx_free, H.L4, H.L6, buf_bytes=B,
                                          ip_id_base=0x1234, device=DEV, timeout_ms=1000)
        ans, ref, _, _ = H.respond_ref(pkts, B, np.zeros(ntx * B, dtype=np.uint8), tx_free, next_id=0x1234)
        want = H.reply_datagrams(ref)
        assert n == len(pkts) and sent == len(want) == cnt[0] and [bool(x & BUILT) for x in echo] == ans
        assert [d.recv(4096) for _ in want] == want
    finally:
        for s in (a, b, c, d):
            s.close()
