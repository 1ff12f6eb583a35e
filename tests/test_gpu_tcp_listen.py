"""rns_rx_tcp_listen_pool_dev on the GPU against listen_host (itself pinned to the reference's restatement by
test_tcp_listen_ref.py, on these same cases), over the records the real placement leaves on the device.  Every
array lies between guards prefilled with 0xEE; every output array is prefilled with a sentinel and compared whole,
so "not written" is checked byte for byte; the pool and the inputs are read back unchanged."""
import numpy as np
import pytest
import torch

import rx_place_helper as P
import tcp_listen_helper as H
from gpu_guard import DEV, Guarded
from rustnetworkstack_amd import _lib, batch
from rustnetworkstack_amd.flow import FLOW_DTYPE
from rustnetworkstack_amd.listen import (ACCEPT_DTYPE, accept_merge, key_hash, listen_host, listen_slots, listen_work, tcp_listen)
from rustnetworkstack_amd.place import meta_records, rx_flow_table, rx_tcp_place_pool
from rustnetworkstack_amd.udp import port_table

pytestmark = pytest.mark.gpu
SENT = H.SENTINEL
U, B_ = H.C_UNMATCHED, H.C_BUILT


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def place(case, layout):
    """The real placement over the case (every known flow's window empty): the meta records, on the device."""
    pool, idx, blk, len16 = layout
    nfl = len(case.keys)
    _, _, d_meta = rx_tcp_place_pool(torch.from_numpy(pool).to(DEV), i32(idx), i32(blk), torch.from_numpy(len16.view(np.int16)).to(DEV),
                                     P.L4, P.L6, torch.from_numpy(rx_flow_table(case.keys)).to(DEV), i32(np.zeros(nfl)),
                                     torch.zeros(nfl, dtype=torch.int64, device=DEV), i32(np.zeros(nfl)),
                                     torch.zeros(16, dtype=torch.uint8, device=DEV), buf_bytes=case.buf)
    return meta_records(d_meta)


def run(case, *, cap=None, ports=None, null_arrays=False):
    """One call over the case after the real placement: the raw output arrays, everything compared with listen_host."""
    layout = P.lay_pool(case.pkts, case.buf, shuffled=True, seed=len(case.pkts) + case.buf)
    pool, idx, blk, len16 = layout
    meta = place(case, layout)
    n = len(case.pkts)
    ports = case.ports if ports is None else ports
    nl = len(ports)
    cap = n if cap is None else cap
    iss = np.array(H.iss_of(n), dtype=np.uint32)
    ins = {"pool": Guarded(pool.size, pool), "idx": Guarded(4 * idx.size, idx), "blk": Guarded(4 * blk.size, blk),
           "len16": Guarded(2 * n, len16), "meta": Guarded(24 * n, meta), "tbl": Guarded(2 * 65536, port_table(ports)),
           "iss": Guarded(4 * n, iss), "add": Guarded(4, np.array([case.ip_id_add], dtype=np.uint32))}
    before = {k: g.host().copy() for k, g in ins.items()}
    sizes = {"out": 64 * cap, "rep_src": 4 * cap, "rep_len8": cap, "accept": 72 * cap, "count": 12, "conn": n}
    out = {k: Guarded(v, fill=SENT) for k, v in sizes.items()}
    need = listen_work(n)
    work = Guarded(need + 16)
    ptr = lambda g: g.t.data_ptr() if g.n else None  # noqa: E731
    arr = (lambda g: None) if null_arrays else ptr
    assert not null_arrays or cap == 0
    batch._call("rns_rx_tcp_listen_pool_dev", torch.device(DEV), ins["pool"].t.data_ptr(), pool.size, case.buf.bit_length() - 1,
                ptr(ins["idx"]), idx.size, ptr(ins["blk"]), ptr(ins["len16"]), n, P.L4, P.L6, ptr(ins["meta"]),
                ptr(ins["tbl"]) if nl else None, nl, None if null_arrays else ptr(ins["iss"]), case.ip_id, ptr(ins["add"]),
                arr(out["out"]), cap, arr(out["rep_src"]), arr(out["rep_len8"]), arr(out["accept"]), ptr(out["count"]),
                ptr(out["conn"]), work.t.data_ptr(), need)
    torch.cuda.synchronize()
    work.host()
    for k, g in ins.items():
        assert np.array_equal(g.host(), before[k]), f"{k} was written"
    fill = lambda nbytes: np.full(nbytes, SENT, np.uint8)  # noqa: E731
    e = listen_host(pool, idx, blk, len16, P.L4, P.L6, meta, port_table(ports) if nl else None, nl, iss, buf_bytes=case.buf,
                    reply_cap=cap, ip_id_base=case.ip_id, ip_id_add=case.ip_id_add, out=fill(64 * cap),
                    rep_src=fill(4 * cap).view(np.uint32), rep_len8=fill(cap), accept=fill(72 * cap).view(ACCEPT_DTYPE))
    got = {k: g.host() for k, g in out.items()}
    assert got["count"].view(np.uint32).tolist() == e.count.tolist()
    assert np.array_equal(got["conn"], e.conn), np.nonzero(got["conn"] != e.conn)[0][:8]
    assert np.array_equal(got["rep_src"].view(np.uint32), e.rep_src) and np.array_equal(got["rep_len8"], e.rep_len8)
    assert np.array_equal(got["out"], e.out), np.nonzero(got["out"] != e.out)[0][:8] // 64
    assert got["accept"].tobytes() == e.accept.tobytes()
    return got, e


CASES = {"order": H.order_case, "options": lambda: H.options_case()[0], "families": H.family_case, "unanswered": H.unanswered_case}


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_host_twin(name):
    got, e = run(CASES[name]())
    assert e.count[0] > 0 and got["conn"].any()


def test_the_order_rule():
    got, _ = run(H.order_case())
    conn = got["conn"]
    assert list(conn[:4]) == [U | H.C_RST | B_, U | H.C_SYN | B_, U | H.C_LATER, U | H.C_LATER]
    assert list(conn[62:66]) == [U | H.C_RST | B_, U | H.C_SYN | B_, U | H.C_LATER, U | H.C_LATER]   # a 64-datagram block's edge
    assert conn[255] == U | H.C_SYN | B_ and conn[256] == U | H.C_LATER and conn[300] == U | H.C_LATER  # a scan block's edge
    assert (conn[400:420] == U | H.C_RST | B_).all() and (conn[420:440] == U | H.C_SYN | B_).all() and \
        (conn[440:480] == U | H.C_LATER).all()


@pytest.mark.parametrize("which", ["many keys", "colliding"])
def test_probing_gives_the_same_bytes_on_every_run(which):
    case = H.many_keys_case() if which == "many keys" else H.colliding_case(key_hash, listen_slots)
    a, e = run(case)
    b, _ = run(case)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert e.count[2] >= 40 and ((e.conn & H.C_LATER) != 0).sum() >= 20


def test_option_shapes():
    case, names = H.options_case()
    got, e = run(case)
    by = dict(zip(names, range(len(names))))
    for shape in ("zero length", "length byte past the end", "truncated mss", "mss zero length"):
        assert got["conn"][2 * by[shape]] == U | H.C_HOST and got["conn"][2 * by[shape] + 1] == U | H.C_LATER, shape
    acc = got["accept"].view(ACCEPT_DTYPE)[:int(e.count[2])]
    mss = {int(a["src"]) // 2: int(a["mss"]) for a in acc}
    assert (mss[by["none"]], mss[by["mss"]], mss[by["nops"]], mss[by["two"]], mss[by["eol"]], mss[by["full"]]) == \
        (0, 1460, 1460, 0x0218, 0, 1460)


def test_ids_across_the_wrap():
    case = H.family_case()
    got, e = run(case)
    R = int(e.count[0])
    out = got["out"].reshape(-1, 64)[:R]
    ids = [int(o[4]) << 8 | int(o[5]) for o in out if o[0] == 0x45]
    first = (case.ip_id + case.ip_id_add) & 0xFFFF
    assert ids == [(first + j) & 0xFFFF for j in range(len(ids))] and 0xFFFF in ids and 0 in ids and len(ids) == e.count[1] < R
    assert set(got["rep_len8"][:R].tolist()) == {40, 44, 60, 64}      # IPv6 replies take no id: 60 00 00 00 is their first dword
    assert all(o[:4].tolist() == [0x60, 0, 0, 0] for o in out if o[0] != 0x45)


@pytest.mark.parametrize("cap", [0, 1, -1])
def test_caps(cap):
    case = H.order_case()
    _, full = run(case)
    R = int(full.count[0])
    cap = R - 1 if cap < 0 else cap
    got, e = run(case, cap=cap, null_arrays=cap == 0)
    assert e.count.tolist() == full.count.tolist() and ((got["conn"] & H.C_NOBUF) != 0).sum() == R - cap
    assert np.array_equal(got["conn"] & 0x4F, full.conn & 0x4F)        # NOBUF SYNs still make later segments LATER


def test_no_listener_means_all_rsts():
    got, e = run(H.unanswered_case(), ports=[])
    assert e.count[2] == 0 and e.count[0] > 0
    assert ((got["conn"] == 0) | (got["conn"] == U | H.C_RST | B_)).all()


def test_after_the_real_placement_and_into_the_next_batch():
    case = H.order_case()
    pool, idx, blk, len16 = P.lay_pool(case.pkts, case.buf, shuffled=True, seed=9)
    n, nfl = len(case.pkts), len(case.keys)
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(DEV)  # noqa: E731
    d_pool = dev(pool, np.uint8)
    iss = np.array(H.iss_of(n), dtype=np.uint32)
    st, meta, r = tcp_listen(d_pool, i32(idx), i32(blk), dev(len16, np.int16), P.L4, P.L6, dev(rx_flow_table(case.keys), np.uint8),
                             i32(np.zeros(nfl)), torch.zeros(nfl, dtype=torch.int64, device=DEV), i32(np.zeros(nfl)),
                             torch.zeros(16, dtype=torch.uint8, device=DEV), dev(port_table(case.ports), np.int16), len(case.ports),
                             i32(iss), buf_bytes=case.buf, ip_id_base=5)
    e = listen_host(pool, idx, blk, len16, P.L4, P.L6, meta_records(meta), port_table(case.ports), len(case.ports), iss,
                    buf_bytes=case.buf, ip_id_base=5)
    R, A = int(e.count[0]), int(e.count[2])
    assert r.count.cpu().numpy().view(np.uint32).tolist() == e.count.tolist() and np.array_equal(r.conn.cpu().numpy()[:n], e.conn)
    out = r.out.cpu().numpy()[:64 * R]
    lens = r.rep_len8.cpu().numpy()[:R].astype(np.int64)
    assert np.array_equal(lens, e.rep_len8[:R])
    for k in range(R):
        assert np.array_equal(out[64 * k:64 * k + lens[k]], e.out[64 * k:64 * k + lens[k]]), k
    # the slots, their checksum fields zeroed, through the transmit finalize: the same bytes
    z = out.copy().reshape(-1, 64)
    for k in range(R):
        h = 20 if z[k, 0] == 0x45 else 40
        z[k, h + 16:h + 18] = 0
        if h == 20:
            z[k, 10:12] = 0
    d_z = dev(z.reshape(-1), np.uint8)
    stx = batch.tx_fill(d_z, torch.arange(R, dtype=torch.int64, device=DEV) * 64, dev(lens.astype(np.int32), np.int32))
    assert ((stx.cpu().numpy() & _lib.RNS_TX_L4_FILLED) != 0).all()
    zz = d_z.cpu().numpy().reshape(-1, 64)
    for k in range(R):
        assert np.array_equal(zz[k, :lens[k]], out[64 * k:64 * k + lens[k]]), k
    # the accepted connections join the flows: the next batch's segments of the new keys match in the placement
    acc = r.accept.cpu().numpy()[:72 * A].view(ACCEPT_DTYPE)
    assert acc.tobytes() == e.accept[:A].tobytes()
    keys, flows, next_seq, win_off, win_len = accept_merge(acc, case.keys, np.zeros(nfl, dtype=FLOW_DTYPE), np.zeros(nfl),
                                                           np.zeros(nfl), np.zeros(nfl))
    assert len(keys) == nfl + A and (flows["state"][nfl:] == _lib.RNS_TCP_SYN_RECEIVED).all()
    nxt = []
    for a in acc:
        src = bytes(a["key"]["ip"][:4 if a["key"]["family"] == 4 else 16])
        nxt.append(H.seg(src, int(a["key"]["sport"]), int(a["key"]["dport"]), int(a["flow"]["rcv_nxt"]), P.ACK,
                         ack=int(a["flow"]["snd_nxt"]) + 1))
    nxt.append(H.seg(H.v4(999), 1, 80, 1, P.ACK))                      # a stranger stays unmatched
    pool2, idx2, blk2, len2 = P.lay_pool(nxt, case.buf, shuffled=True, seed=3)
    _, _, meta2 = rx_tcp_place_pool(dev(pool2, np.uint8), i32(idx2), i32(blk2), dev(len2, np.int16), P.L4, P.L6,
                                    dev(rx_flow_table(keys), np.uint8), i32(next_seq), dev(win_off.astype(np.int64), np.int64),
                                    i32(win_len), torch.zeros(16, dtype=torch.uint8, device=DEV), buf_bytes=case.buf)
    m2 = meta_records(meta2)
    assert (m2["place"][:A] & P.P_FLOW).all() and m2["flow"][:A].tolist() == list(range(nfl, nfl + A))
    assert m2["place"][A] == P.P_TCP and m2["flow"][A] == P.NO_FLOW
