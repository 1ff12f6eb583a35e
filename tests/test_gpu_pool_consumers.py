"""The three consumers of the pool receive verify on one batch: rx_verify_pool alone, the TCP placement, the
ICMP echo responder and the UDP demux leave byte-identical status and l4_sum, and each consumer's outputs
equal its reference (rx_place_helper.expected; echo_host, itself compared with respond_ref here; demux_host,
its queues compared with demux_ref's here).

The batch: 70 datagrams (a full 64-block and a partial one) in shuffled 256-byte buffers, TCP to known flows
and an unknown one, UDP to bound ports and an unbound one, echo requests, each as IPv4 with IHL 5 and 15 and
as IPv6, total lengths one byte below, at and above a buffer boundary, and one malformed datagram.  The last
datagram ends in the pool's last buffer, and the pool is cut 5 bytes short of a whole buffer, so the last
16-byte source chunk is not whole inside the pool.  The test sees results only: it cannot tell which loads
were issued there."""
import numpy as np
import pytest
import torch

import icmp_echo_helper as EH
import test_gpu_icmp_echo as TE
import test_gpu_udp_demux as TU
import udp_demux_helper as UH
from oracle import oracle as O
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.icmp import echo_host, rx_icmp_echo_pool
from rustnetworkstack_amd.place import meta_records, rx_flow_table, rx_tcp_place_pool
from rustnetworkstack_amd.pool import rx_verify_pool
from rustnetworkstack_amd.udp import REC, UdpDemux, demux_host, drain, port_table, rx_udp_demux_pool
from rx_place_helper import L4, L6, R4, R6, SENTINEL, body_bytes, expected, key_of, lay_pool, segment

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 256
TOTALS = (B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 100, 3 * B + 2)  # datagram lengths
PORTS = [53, 5353]
KEYS = [key_of(R4, 1234, 80), key_of(R6, 1234, 80)]
NEXT_SEQ, WIN_OFF, WIN_LEN = [0x1000, 0xFFFFFF00], [5, 0x8003], [0x7FF0, 0x7FF0]
STREAM_BYTES = 0x10000
TXFILL, DATAFILL, RECFILL = 0xA5, 0xA5, 0x5A


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    if not torch.cuda.is_available() or _lib.load().rns_device_count() == 0:
        pytest.fail("gpu tests need a GPU (the HIP path has no CPU fallback)")


def dev(a, view):
    return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(DEV)


def datagrams(last_kind, last_frag):
    """The batch: datagram k's kind, family and length all vary with k; the last one is `last_kind` with
    `last_frag` bytes in its third buffer."""
    pos = [0, 0]  # the next free byte of each flow's window

    def one(kind, fam, total, tag):
        ip = (20, 60, 40)[fam]
        src, ihl = (R6 if fam == 2 else R4), (15 if fam == 1 else 5)
        if kind == "tcp":
            f, n, known = (1 if fam == 2 else 0), total - ip - 20, tag % 7 != 6
            if known:
                pos[f] += 1 + tag % 16  # a gap of sentinel bytes: the destination's alignment varies
            p = segment(src, 1234 if known else 999, 80, NEXT_SEQ[f] + pos[f], body_bytes(tag, n), ihl=ihl)
            pos[f] += n if known else 0
        elif kind == "udp":
            pay = UH.body(tag, total - ip - 8)
            dport = (53, 5353, 9)[tag % 3]
            p = UH.udp6(4000 + tag, dport, pay) if fam == 2 else UH.udp4(4000 + tag, dport, pay, ihl=ihl)
        else:
            pay = EH.body(tag, total - ip - 4)
            p = EH.ping6(pay) if fam == 2 else EH.ping4(pay, ihl=ihl)
        assert len(p) == total
        return p

    pkts = [one(("tcp", "udp", "ping")[k % 3], (k // 3) % 3, TOTALS[(k // 9) % 8], k) for k in range(68)]
    pkts.insert(33, bytes([0x75]) + UH.body(7, 47))  # version 7: malformed
    pkts.append(one(last_kind, 0, 2 * B + last_frag, 99))
    assert len(pkts) == 70 and max(pos) + 16 <= min(WIN_LEN)
    return pkts


def lay_at_the_tail(pkts):
    """lay_pool's shuffled form with no spare buffer, the last datagram's last fragment moved into the pool's
    last buffer and the pool cut 5 bytes short."""
    pool, idx, blk, len16 = lay_pool(pkts, B, shuffled=True, seed=7, spare=0)
    rows = pool.reshape(-1, B)
    q = int(np.flatnonzero(idx == rows.shape[0] - 1)[0])
    rows[[idx[q], idx[-1]]] = rows[[idx[-1], idx[q]]]
    idx[q], idx[-1] = idx[-1], idx[q]
    assert int(len16[-1]) % B <= B - 5
    return pool[:-5].copy(), idx, blk, len16


class Case:
    """One batch, its references (computed once) and the verify's own results on the device."""

    def __init__(self, last_kind, last_frag, oracle):
        self.pkts = pkts = datagrams(last_kind, last_frag)
        self.pool, self.idx, self.blk, self.len16 = pool, idx, blk, len16 = lay_at_the_tail(pkts)
        self.n, self.nf = n, nf = len(pkts), idx.size
        assert pool.size == nf * B - 5 and idx[-1] == nf - 1
        # the placement's reference
        self.stream0 = np.full(STREAM_BYTES, SENTINEL, dtype=np.uint8)
        self.place = expected(pkts, B, KEYS, NEXT_SEQ, WIN_OFF, WIN_LEN, self.stream0, ones_comp=oracle.compute_ones_comp)
        # the responder's: echo_host, and the reference's echo path restated over the same transmit pool
        ntx = TE.tx_needed(pkts, B) + 5
        self.free = np.random.default_rng(n).permutation(ntx).astype(np.uint32)
        self.tx0 = np.full(ntx * B, TXFILL, dtype=np.uint8)
        self.tx_ref, tx_restated = self.tx0.copy(), self.tx0.copy()
        self.echo = echo_host(pool, idx, blk, len16, L4, L6, self.tx_ref, self.free, buf_bytes=B)
        answered, _, srcs, _ = EH.respond_ref(pkts, B, tx_restated, self.free)
        assert np.array_equal(self.tx_ref, tx_restated) and self.echo[6].tolist() == srcs
        assert [bool(e & _lib.RNS_ECHO_BUILT) for e in self.echo[2]] == answered and sum(answered) >= 20
        # the demux's: demux_host, and the reference's queues
        self.tbl = port_table(PORTS)
        self.data_ref = np.full(nf * B, DATAFILL, dtype=np.uint8)
        self.rec_ref = np.full(32 * n, RECFILL, dtype=np.uint8).view(REC)
        self.demux = demux_host(pool, idx, blk, len16, L4, L6, self.tbl, len(PORTS), buf_bytes=B, data=self.data_ref,
                                rec=self.rec_ref)
        self.queues = UH.queues_ref(UH.demux_ref(pkts, B, PORTS)[1], PORTS)
        assert [drain(self.demux, s) for s in range(len(PORTS))] == self.queues and sum(map(len, self.queues)) >= 12
        # no datagram of the batch is dropped for the pool's size: one verdict, and only the malformed one is
        self.status, self.l4 = self.place[0], self.place[1]
        for st, l4 in ((self.echo[0], self.echo[1]), (self.demux.status, self.demux.l4_sum)):
            assert np.array_equal(st, self.status) and np.array_equal(l4, self.l4)
        assert (np.flatnonzero(self.status & O.RX_MALFORMED) == [33]).all() and self.status[-1] & O.RX_ACCEPT
        # the device's inputs, and the verify alone
        self.d_pool = torch.from_numpy(pool).to(DEV)
        self.d_in = (dev(idx, np.int32), dev(blk, np.int32), dev(len16, np.int16))
        st, l4 = rx_verify_pool(self.d_pool, *self.d_in, L4, L6, buf_bytes=B, l4_sum=self.new_l4())
        self.verify = self.host(st, l4)

    def new_l4(self):
        return torch.full((self.n,), 0x5555, dtype=torch.uint16, device=DEV)

    @staticmethod
    def host(st, l4):
        torch.cuda.synchronize()
        return st.cpu().numpy().tobytes(), l4.view(torch.int16).cpu().numpy().view(np.uint16).tobytes()

    def same_verdicts(self, st, l4):
        """Byte-identical to the verify alone, which equals the reference."""
        assert self.verify == (self.status.tobytes(), self.l4.tobytes())
        assert self.host(st, l4) == self.verify
        assert np.array_equal(self.d_pool.cpu().numpy(), self.pool), "the pool changed"


_CASES = {}


@pytest.fixture(params=[("tcp", 251), ("udp", 249), ("ping", 251)], ids=lambda p: f"{p[0]}{p[1]}")
def case(request, oracle):
    if request.param not in _CASES:
        _CASES[request.param] = Case(*request.param, oracle)
    return _CASES[request.param]


def test_placement(case):
    d_stream = torch.from_numpy(case.stream0).to(DEV)
    meta = torch.full((case.n, 24), 0xEE, dtype=torch.uint8, device=DEV)
    st, l4, m = rx_tcp_place_pool(case.d_pool, *case.d_in, L4, L6, torch.from_numpy(rx_flow_table(KEYS)).to(DEV),
                                  dev(np.asarray(NEXT_SEQ, dtype=np.uint32), np.int32),
                                  dev(np.asarray(WIN_OFF, dtype=np.uint64), np.int64),
                                  dev(np.asarray(WIN_LEN, dtype=np.uint32), np.int32), d_stream, buf_bytes=B,
                                  l4_sum=case.new_l4(), meta=meta)
    case.same_verdicts(st, l4)
    want_meta, want_stream = case.place[2], case.place[3]
    got = meta_records(m)
    bad = np.flatnonzero(got != want_meta)
    assert bad.size == 0, [(int(i), got[i], want_meta[i]) for i in bad[:6]]
    got_stream = d_stream.cpu().numpy()
    assert np.array_equal(got_stream, want_stream), np.flatnonzero(got_stream != want_stream)[:8]
    assert int(((want_meta["place"] & 4) != 0).sum()) >= 18  # RNS_PLACE_DONE: both flows' segments were copied


def test_echo(case):
    d_tx = torch.from_numpy(case.tx0).to(DEV)
    out = rx_icmp_echo_pool(case.d_pool, *case.d_in, L4, L6, d_tx, dev(case.free, np.int32), buf_bytes=B,
                            l4_sum=case.new_l4())
    case.same_verdicts(out[0], out[1])
    _, _, echo, bf, hl, pl, src, cnt = case.echo
    got_cnt = out[7].cpu().numpy().view(np.uint32)
    assert got_cnt.tolist() == cnt.tolist()
    assert np.array_equal(out[2].cpu().numpy()[:case.n], echo)
    for got, ref, dt in ((out[3], bf, np.uint32), (out[4], hl, np.uint8), (out[6], src, np.uint32)):
        assert np.array_equal(got.cpu().numpy().view(dt)[:len(ref)], ref)
    assert np.array_equal(out[5].view(torch.int16).cpu().numpy().view(np.uint16)[:len(pl)], pl)
    got_tx = d_tx.cpu().numpy()
    TE.mask_slack(got_tx, case.tx_ref, case.free, bf, hl, pl, B)
    assert np.array_equal(got_tx, case.tx_ref), np.flatnonzero(got_tx != case.tx_ref)[:8]


def test_demux(case):
    e = case.demux
    d_data = torch.full((case.nf * B,), DATAFILL, dtype=torch.uint8, device=DEV)
    d_rec = torch.full((32 * case.n,), RECFILL, dtype=torch.uint8, device=DEV)
    r = rx_udp_demux_pool(case.d_pool, *case.d_in, L4, L6, dev(case.tbl, np.int16), len(PORTS), buf_bytes=B, data=d_data,
                          rec=d_rec, l4_sum=case.new_l4())
    case.same_verdicts(r.status, r.l4_sum)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    assert u32(r.count).tolist() == e.count.tolist() and np.array_equal(u32(r.q_first), e.q_first)
    assert np.array_equal(r.udp.cpu().numpy()[:case.n], e.udp) and np.array_equal(u32(r.pos)[:case.n], e.pos)
    got_rec, got_data = d_rec.cpu().numpy(), d_data.cpu().numpy()
    assert np.array_equal(got_rec, case.rec_ref.view(np.uint8)), np.flatnonzero(got_rec != case.rec_ref.view(np.uint8))[:8] // 32
    TU.mask_slack(got_data, case.data_ref, e)
    assert np.array_equal(got_data, case.data_ref), np.flatnonzero(got_data != case.data_ref)[:8]
    got = UdpDemux(e.status, e.l4_sum, e.udp, e.pos, got_rec.view(REC), e.q_first, e.count, got_data)
    assert [drain(got, s) for s in range(len(PORTS))] == case.queues
