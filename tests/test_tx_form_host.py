"""``pool._TxFormHost`` against the two allocation loops it replaced.

``icmp.echo_host`` and ``udp.send_host`` are what the GPU tests compare the device with, and both are now written
over one host allocator.  ``_old_echo_host`` and ``_old_send_host`` below are their bodies from before that change,
kept here so that a mistake made in the shared allocator cannot pass by being made on both sides: the new functions
must return identical arrays and leave identical transmit pool bytes.  CPU only.
"""
import numpy as np
import pytest

import icmp_echo_helper as E
import udp_send_helper as U
from oracle import oracle as O
from test_rx_oracle import L4, L6

from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import _local_addrs
from rustnetworkstack_amd.icmp import echo_host
from rustnetworkstack_amd.pool import _be_sum, _buf_log2, _fold, _host_datagrams, _np
from rustnetworkstack_amd.udp import REC, UdpSend, send_host


def _old_echo_host(rx_pool: np.ndarray, buf_idx, blk_first, len16, local_ipv4: bytes, local_ipv6: bytes, tx_pool: np.ndarray,
              free, *, buf_bytes: int = 512, reply_cap: int | None = None, ip_id_base: int = 0, ip_id_add: int = 0):
    """``icmp.echo_host`` as it was before ``pool._TxFormHost``."""
    B = int(buf_bytes)
    log2 = _buf_log2(B, 256)
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    free = np.asarray(free, dtype=np.uint32).astype(np.int64)
    n, n_free = len(len16), len(free)
    cap = n if reply_cap is None else int(reply_cap)
    tx_bufs = tx_pool.size >> log2
    status, l4_sum, echo = np.zeros(n, np.uint8), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    heads, pays, srcs, firsts = [], [], [], []
    R = F = V = 0
    full = False
    for i, T, d, st, l4, h, v6 in _host_datagrams(rx_pool, buf_idx, blk_first, len16, ip4, ip6, B, log2):
        status[i], l4_sum[i] = st, l4
        if not (st & _lib.RNS_RX_ACCEPT) or T - h < 4 or (d[6] if v6 else d[9]) != (58 if v6 else 1) or \
                d[h] != (128 if v6 else 8):
            continue
        pay = d[h + 4:]
        nfr = 1 + -(-len(pay) // B)
        R, F = R + 1, F + nfr
        if full or R > cap or F > n_free:
            full = True  # (both counts are monotone: every later request is past them too)
            echo[i] = _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_NOBUF
            continue
        bufs = free[F - nfr:F]
        if (R - 1) % 64 == 0:
            firsts.append(F - nfr)
        pays.append(len(pay))
        srcs.append(i)
        if (bufs >= tx_bufs).any():
            echo[i] = _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BADBUF
            heads.append(0)
            V += 0 if v6 else 1
            continue
        echo[i] = _lib.RNS_ECHO_REQUEST | _lib.RNS_ECHO_BUILT
        if v6:
            peer = d[8:24]
            icmp = bytearray([129, 0, 0, 0])
            seed = _fold(_be_sum(ip6) + _be_sum(peer) + 4 + len(pay) + 58)
            ip = bytes([0x60, 0, 0, 0]) + (4 + len(pay)).to_bytes(2, "big") + bytes([58, 64]) + ip6 + peer
        else:
            peer = d[12:16]
            icmp = bytearray(4)
            seed = 0
            ipb = bytearray([0x45, 0]) + ((24 + len(pay)) & 0xFFFF).to_bytes(2, "big") + \
                ((int(ip_id_base) + int(ip_id_add) + V) & 0xFFFF).to_bytes(2, "big") + bytes([0, 0, 64, 1, 0, 0]) + ip4 + peer
            ipb[10:12] = (_fold(_be_sum(ipb)) ^ 0xFFFF).to_bytes(2, "big")
            ip = bytes(ipb)
            V += 1
        icmp[2:4] = (_fold(seed + _be_sum(icmp) + _be_sum(pay)) ^ 0xFFFF).to_bytes(2, "big")
        head = ip + bytes(icmp)
        heads.append(len(head))
        at = (int(bufs[0]) << log2) + B - len(head)
        tx_pool[at:at + len(head)] = np.frombuffer(head, dtype=np.uint8)
        for j in range(nfr - 1):
            part = pay[j * B:(j + 1) * B]
            at = int(bufs[1 + j]) << log2
            tx_pool[at:at + len(part)] = np.frombuffer(part, dtype=np.uint8)
    # the counts: the answered requests are a prefix of the requests
    nrep = len(pays)
    nbuf = int(sum(1 + -(-p // B) for p in pays))
    return (status, l4_sum, echo, np.array(firsts, dtype=np.uint32), np.array(heads, dtype=np.uint8),
            np.array(pays, dtype=np.uint16), np.array(srcs, dtype=np.uint32), np.array([nrep, nbuf, V], dtype=np.uint32))


def _old_send_host(data: np.ndarray, rec, q_first, sock_port, local_ipv4: bytes, local_ipv6: bytes, tx_pool: np.ndarray, free, *,
              buf_bytes: int = 512, n_recs: int | None = None, send_cap: int | None = None, ip_id_base: int = 0,
              ip_id_add: int = 0) -> UdpSend:
    """``udp.send_host`` as it was before ``pool._TxFormHost``."""
    B = int(buf_bytes)
    log2 = _buf_log2(B, 256)
    ip4, ip6 = _local_addrs(local_ipv4, local_ipv6)
    rec = _np(rec, np.uint8)
    rec = rec[:rec.size // 32 * 32].view(REC)
    q = np.asarray(q_first, dtype=np.uint32).astype(np.int64)
    ports = np.asarray(sock_port).astype(np.uint16)
    n_socks = len(ports)
    if not 1 <= n_socks <= _lib.RNS_UDP_MAX_SOCKS or len(q) < n_socks + 1:
        raise ValueError(f"sock_port needs 1..{_lib.RNS_UDP_MAX_SOCKS} ports and q_first one entry more")
    free = np.asarray(free, dtype=np.uint32).astype(np.int64)
    n, n_free = len(rec) if n_recs is None else int(n_recs), len(free)
    cap = n if send_cap is None else int(send_cap)
    tx_bufs = tx_pool.size >> log2
    send = np.zeros(n, np.uint8)
    heads, pays, srcs, firsts = [], [], [], []
    R = F = V = 0
    full = False
    for k in range(min(n, int(q[n_socks]))):
        r = rec[k]
        fam, ln, at = int(r["family"]), int(r["len"]), 16 * int(r["off16"])
        if not int(r["flags"]) & _lib.RNS_UDP_QUEUED or fam not in (4, 6) or at + ln > data.size:
            continue
        s = max(int(np.searchsorted(q[:n_socks], k, side="right")) - 1, 0)
        pay = data[at:at + ln].tobytes()
        nfr = 1 + -(-ln // B)
        R, F = R + 1, F + nfr
        if full or R > cap or F > n_free:
            full = True  # (both counts are monotone: every later send is past them too)
            send[k] = _lib.RNS_UDPTX_SEND | _lib.RNS_UDPTX_NOBUF
            continue
        bufs = free[F - nfr:F]
        if (R - 1) % 64 == 0:
            firsts.append(F - nfr)
        pays.append(ln)
        srcs.append(k)
        if (bufs >= tx_bufs).any():
            send[k] = _lib.RNS_UDPTX_SEND | _lib.RNS_UDPTX_BADBUF
            heads.append(0)
            V += 1 if fam == 4 else 0
            continue
        send[k] = _lib.RNS_UDPTX_SEND | _lib.RNS_UDPTX_BUILT
        ulen = (8 + ln) & 0xFFFF  # udp.rs:152 `as u16`
        dst = r["ip"][:4 if fam == 4 else 16].tobytes()
        src = ip4 if fam == 4 else ip6
        udp = bytearray(int(ports[s]).to_bytes(2, "big") + int(r["sport"]).to_bytes(2, "big") + ulen.to_bytes(2, "big") + b"\0\0")
        udp[6:8] = (_fold(_be_sum(src) + _be_sum(dst) + 17 + ulen + _be_sum(udp) + _be_sum(pay)) ^ 0xFFFF).to_bytes(2, "big")
        if fam == 6:
            ip = bytes([0x60, 0, 0, 0]) + ulen.to_bytes(2, "big") + bytes([17, 64]) + ip6 + dst
        else:
            ipb = bytearray([0x45, 0]) + ((28 + ln) & 0xFFFF).to_bytes(2, "big") + \
                ((int(ip_id_base) + int(ip_id_add) + V) & 0xFFFF).to_bytes(2, "big") + bytes([0, 0, 64, 17, 0, 0]) + ip4 + dst
            ipb[10:12] = (_fold(_be_sum(ipb)) ^ 0xFFFF).to_bytes(2, "big")
            ip = bytes(ipb)
            V += 1
        head = ip + bytes(udp)
        heads.append(len(head))
        at = (int(bufs[0]) << log2) + B - len(head)
        tx_pool[at:at + len(head)] = np.frombuffer(head, dtype=np.uint8)
        for j in range(nfr - 1):
            part = pay[j * B:(j + 1) * B]
            at = int(bufs[1 + j]) << log2
            tx_pool[at:at + len(part)] = np.frombuffer(part, dtype=np.uint8)
    nbuf = int(sum(1 + -(-p // B) for p in pays))
    return UdpSend(send, np.array(firsts, dtype=np.uint32), np.array(heads, dtype=np.uint8), np.array(pays, dtype=np.uint16),
                   np.array(srcs, dtype=np.uint32), np.array([len(pays), nbuf, V], dtype=np.uint32))


# ---------------------------------------------------------------------------
# the shapes: the helpers' batches, a transmit pool with a permuted free list, and the cuts
# ---------------------------------------------------------------------------
BS = (256, 512)
CAPS = (0, 1, 63, 64, 65, None)  # None: all


def tx_pool_for(need, B, spare=3):
    """A transmit pool of need + spare buffers filled with a pattern, and a free list that is no identity."""
    nbuf = need + spare
    pool = O.splitmix64_bytes(0x7F00 + B, nbuf * B).copy()
    free = ((np.arange(nbuf, dtype=np.int64) * 7 + 3) % nbuf if nbuf % 7 else np.arange(nbuf)[::-1]).astype(np.uint32)
    assert len(set(free.tolist())) == nbuf
    return pool, free


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all()


_ECHO = {}


def echo_batch(B):
    """Every echo case of the helper in one batch, laid into a receive pool — built once per B."""
    if B not in _ECHO:
        c = E.cases(B)
        pkts = [p for name in ("lengths", "ihl", "sums", "code", "rejects", "mixed") for p in c[name]]
        pool, buf_idx, blk_first, len16 = E.lay_pool(pkts, B)[:4]
        need = sum(1 + -(-max(len(p) - 24, 0) // B) for p in pkts)
        _ECHO[B] = (np.asarray(pool), buf_idx, blk_first, len16, need, len(pkts))
    return _ECHO[B]


def run_echo(B, free, tx, **kw):
    rx, buf_idx, blk_first, len16, _, _ = echo_batch(B)
    t_old, t_new = tx.copy(), tx.copy()
    old = _old_echo_host(rx, buf_idx, blk_first, len16, L4, L6, t_old, free, buf_bytes=B, **kw)
    new = echo_host(rx, buf_idx, blk_first, len16, L4, L6, t_new, free, buf_bytes=B, **kw)
    same(old, new)
    assert (t_old == t_new).all()
    return new


def run_send(b, B, free, tx, **kw):
    t_old, t_new = tx.copy(), tx.copy()
    old = _old_send_host(b.data, b.rec, b.q_first, b.ports, L4, L6, t_old, free, buf_bytes=B, **kw)
    new = send_host(b.data, b.rec, b.q_first, b.ports, L4, L6, t_new, free, buf_bytes=B, **kw)
    assert type(new) is UdpSend
    same(old, new)
    assert (t_old == t_new).all()
    return new


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("cap", CAPS)
def test_echo_caps(B, cap):
    need = echo_batch(B)[4]
    tx, free = tx_pool_for(need, B)
    out = run_echo(B, free, tx, reply_cap=cap, ip_id_base=0xFFF0, ip_id_add=7)  # (the ids wrap past 0xffff)
    nreq = int((out[2] & _lib.RNS_ECHO_REQUEST != 0).sum())
    assert nreq > 65 and int(out[7][0]) == (nreq if cap is None else min(cap, nreq))
    if cap is None:
        assert int(out[7][2]) > 0x10  # IPv4 replies enough to wrap


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", ["lengths", "sums", "one", "count65"])
@pytest.mark.parametrize("cap", CAPS)
def test_send_caps(name, B, cap):
    b = U.case(name, B)
    tx, free = tx_pool_for(b.tx_needed(B), B)
    out = run_send(b, B, free, tx, send_cap=cap, ip_id_base=0xFFFE, ip_id_add=0xFFFF)
    assert int(out.count[0]) == (len(b.sends) if cap is None else min(cap, len(b.sends)))


@pytest.mark.parametrize("B", BS)
def test_send_big_wraps(B):
    """Lengths whose 28 + len and 8 + len wrap as u16."""
    b = U.case("big", B)
    tx, free = tx_pool_for(b.tx_needed(B), B)
    assert int(run_send(b, B, free, tx).count[0]) == len(b.sends)


def first_multi(pay_lens, B):
    """The first item with two payload buffers or more, and the buffers of the items before it."""
    before = 0
    for k, n in enumerate(pay_lens):
        nfr = 1 + -(-n // B)
        if nfr >= 3:
            return k, before, nfr
        before += nfr
    raise AssertionError("no multi-buffer item")


@pytest.mark.parametrize("B", BS)
def test_free_list_one_short(B):
    """The free list ends one buffer short of a multi-buffer item: it and everything after it is NOBUF."""
    need = echo_batch(B)[4]
    tx, free = tx_pool_for(need, B)
    full = run_echo(B, free, tx)
    k, before, nfr = first_multi([int(p) for p in full[5]], B)
    out = run_echo(B, free[:before + nfr - 1], tx)
    assert int(out[7][0]) == k and int(out[7][1]) == before

    b = U.case("lengths", B)
    tx, free = tx_pool_for(b.tx_needed(B), B)
    k, before, nfr = first_multi([len(s[3]) for s in b.sends], B)
    out = run_send(b, B, free[:before + nfr - 1], tx)
    assert int(out.count[0]) == k and int(out.count[1]) == before
    assert (out.send[k:] & _lib.RNS_UDPTX_NOBUF != 0).all()


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("where", ["first", "last"])
def test_bad_free_index(B, where):
    """One free index outside the transmit pool, at the list's position 0 and at the last position taken."""
    need = echo_batch(B)[4]
    tx, free = tx_pool_for(need, B, spare=0)
    taken = int(run_echo(B, free, tx)[7][1])
    bad = free.copy()
    bad[0 if where == "first" else taken - 1] = len(free) + 5
    out = run_echo(B, bad, tx)
    assert int((out[2] & _lib.RNS_ECHO_BADBUF != 0).sum()) == 1 and int((out[4] == 0).sum()) == 1

    b = U.case("one", B)
    tx, free = tx_pool_for(b.tx_needed(B), B, spare=0)
    bad = free.copy()
    bad[0 if where == "first" else len(free) - 1] = 0xFFFFFFFF
    out = run_send(b, B, bad, tx, ip_id_base=0xFFFF)
    assert int((out.send & _lib.RNS_UDPTX_BADBUF != 0).sum()) == 1
    assert int((out.tx_head_len8 == 0).sum()) == 1 and int(out.count[0]) == len(b.sends)
