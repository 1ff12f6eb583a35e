"""The reassembler side of TCP receive placement, without a GPU: the restated TCPReassembler
(rx_place_helper.RefReassembler, over byte strings) and place.Reassembler (over (seq, len) pairs, the
data already in place) both reproduce the reference's unit tests (tests/golden/reassembler_kats.json,
read off tcp.rs:1055-1323), and for random segment sets the bytes the reference would deliver are
the window bytes the placement rule puts below the reassembler's advance."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from rustnetworkstack_amd import batch
from rustnetworkstack_amd.place import META_DTYPE, Reassembler
from rx_place_helper import META, R4, R6, SENTINEL, RefReassembler, body_bytes, expected, key_of, segment

with open(os.path.join(GOLDEN, "reassembler_kats.json")) as _f:
    KATS = json.load(_f)["kats"]


def test_kats_cover_the_reference_tests():
    assert len(KATS) == 9 and len({k["name"] for k in KATS}) == 9
    assert META_DTYPE == META and batch.META_DTYPE is META_DTYPE and batch.Reassembler is Reassembler


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_reassemblers_reproduce_the_reference(kat):
    ref, mine = RefReassembler(), Reassembler()
    ref.set_next_expect(kat["next_expect"])
    mine.set_next_expect(kat["next_expect"])
    for c in kat["calls"]:
        got = ref.add_packet(bytes([c["fill"]]) * c["len"], c["seq"])
        assert ref.get_next_expect() == c["next_expect"] and len(ref.out_of_order) == c["pending"]
        assert (len(got) if got is not None else 0) == c["delivered"]
        assert mine.add(c["seq"], c["len"]) == c["delivered"]
        assert mine.get_next_expect() == c["next_expect"] and len(mine.out_of_order) == c["pending"]


def test_ooo_delivery_is_in_sequence_order():
    """test_reassemble_ooo's byte checks: the delivered buffer is packet 1 then packet 2."""
    r = RefReassembler()
    r.set_next_expect(1000)
    assert r.add_packet(bytes([2]) * 100, 1100) is None
    assert r.add_packet(bytes([1]) * 100, 1000) == bytes([1]) * 100 + bytes([2]) * 100


@pytest.mark.parametrize("seed", range(6))
def test_placed_window_holds_what_the_reference_delivers(seed):
    """Random non-overlapping in-window segments of a few flows in random order: the expected window
    bytes [0, advance) are the reference reassembler's delivered bytes, and advance is
    Reassembler.feed's total."""
    rng = np.random.default_rng(seed)
    nfl = int(rng.integers(2, 5))
    srcs = [R4, R6, bytes([10, 0, 0, 7]), bytes(range(16))]
    keys = [key_of(srcs[f], 4000 + f, 80) for f in range(nfl)]
    next_seq = [int(x) for x in rng.integers(0, 2 ** 32, nfl)]
    next_seq[0] = 0xFFFFFF00                                        # one flow across the wrap
    win_len, pkts, sent = [], [], []
    for f in range(nfl):
        lens = rng.integers(1, 300, int(rng.integers(3, 11)))      # at most 40 segments in all
        drop = set(rng.choice(len(lens), int(rng.integers(0, 3)), replace=False).tolist()) - {0}
        off = 0
        for j, ln in enumerate(lens):
            if j not in drop:                                       # a hole stops the advance
                body = body_bytes(1000 * seed + 50 * f + j, int(ln))
                pkts.append((f, (next_seq[f] + off) & 0xFFFFFFFF, body))
                sent.append(segment(srcs[f], 4000 + f, 80, next_seq[f] + off, body))
            off += int(ln)
        win_len.append(off + 7)
    assert len(pkts) <= 40
    order = rng.permutation(len(pkts))
    pkts, sent = [pkts[i] for i in order], [sent[i] for i in order]
    win_off = np.concatenate([[3], 3 + np.cumsum(win_len)[:-1]]).astype(np.int64)
    total = int(win_off[-1]) + win_len[-1] + 5
    st, _, meta, stream = expected(sent, 512, keys, next_seq, win_off, win_len, np.full(total, SENTINEL, dtype=np.uint8))
    assert (meta["place"] == 7).all()
    for f in range(nfl):
        ref, mine = RefReassembler(), Reassembler(next_seq[f])
        ref.set_next_expect(next_seq[f])
        delivered = b""
        for g, seq, body in pkts:
            if g == f:
                got = ref.add_packet(body, seq)
                delivered += got if got is not None else b""
        advance = mine.feed(meta, f)
        assert advance == len(delivered) > 0
        assert mine.get_next_expect() == ref.get_next_expect() == (next_seq[f] + advance) & 0xFFFFFFFF
        w = stream[int(win_off[f]):int(win_off[f]) + win_len[f]]
        assert w[:advance].tobytes() == delivered
        assert (w[-7:] == SENTINEL).all()
    assert (stream[:3] == SENTINEL).all() and (stream[-5:] == SENTINEL).all()
