"""The datagrams tx_segment_helper builds are what the reference's receive path accepts: the
helper restates tcp_write's segment loop (tcp.rs:256-285) and the head fields tcp_output and
ip_output write (tcp.rs:938-976, ip.rs:140-177), the oracle fills the checksums, and
rx_verify_ref, with the destination as the local address, must accept every segment; the payloads
concatenate to the send's data; seq and id advance as the form states."""
import struct

import pytest

from oracle import oracle as O
from tx_segment_helper import DST4, DST6, Flow, data_bytes, datagrams, expected, lay, template

OK = O.RX_IP_OK | O.RX_L4_OK | O.RX_ACCEPT


def cases():
    out = []
    for v6 in (False, True):
        for opts in (0, 12, 32):
            for mss, n in ((1460, 44 * 1460 + 7), (537, 2 * 537), (1, 5), (17, 16), (1459, 1460)):
                out.append((v6, opts, mss, n))
    return out


@pytest.mark.parametrize("v6,opts,mss,n", cases())
def test_reference_accepts_the_segments(oracle, v6, opts, mss, n):
    seq0, id0 = 0xFFFFFF00, 0xFFFE                             # both wrap within the flow
    t = template(v6=v6, opts=opts, seq=seq0, ident=id0)
    data = data_bytes(mss * 31 + n, n)
    L = lay([Flow(t, data, mss, align=(mss + n) % 16)], head_align=1 + opts % 3)
    arena, st, ch = expected(oracle, L)
    want_st = 0x02 if v6 else 0x03
    assert st.tolist() == [want_st] * L.n_seg and L.n_seg == -(-n // mss)
    dgs = datagrams(arena, ch)
    iphdr, hl = (40 if v6 else 20), len(t)
    got = b""
    for j, d in enumerate(dgs):
        assert O.rx_verify_ref(d, DST4, DST6, oracle.compute_ones_comp)[0] == OK, j
        pay = d[hl:]
        assert 1 <= len(pay) <= mss and (len(pay) == mss or j == len(dgs) - 1)
        got += pay
        assert struct.unpack(">I", d[iphdr + 4:iphdr + 8])[0] == (seq0 + j * mss) & 0xFFFFFFFF
        assert d[iphdr + 13] == 0x18                            # ACK | PSH on every piece (tcp.rs:279)
        if v6:
            assert struct.unpack(">H", d[4:6])[0] == len(d) - 40
        else:
            assert struct.unpack(">H", d[2:4])[0] == len(d)
            assert struct.unpack(">H", d[4:6])[0] == (id0 + j) & 0xFFFF
        # everything else is the template's
        same = bytearray(d[:hl])
        for lo, hi in ([(4, 6)] if v6 else [(2, 6), (10, 12)]) + [(iphdr + 4, iphdr + 8), (iphdr + 16, iphdr + 18)]:
            same[lo:hi] = t[lo:hi]
        assert bytes(same) == t
    assert got == data
