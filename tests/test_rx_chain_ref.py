"""The chain reference of the rx-chain tests (tests/rx_chain_helper.py) anchored to the pinned
oracle: where the per-fragment fold cannot differ from the flat one — the first fragment holds
the IP header and every non-final trimmed fragment is even — it equals oracle.rx_verify_ref on
the concatenation; a fixed odd split differs from the flat value, which shows that the
per-fragment fold (util.rs:112-119, each fragment zero-padded on its own) is what it computes."""
import numpy as np

from oracle import oracle as O
from rx_chain_helper import (hdr_len, ipv4_long, make_datagrams, netbuffers, rx_verify_chain_ref, split_even,
                             trim_head)
from test_rx_oracle import L4, L6, R4, R6, ipv4, ipv6, tcp_seg


def test_even_splits_equal_the_flat_oracle():
    pkts = make_datagrams(14 * 44, 0xC4A1)
    w = O.splitmix64_words(0xC4A2, 4096)
    kinds = set()
    for i, p in enumerate(pkts):
        want = O.rx_verify_ref(p, L4, L6)
        kinds.add(want[0])
        chain = split_even(p, max(hdr_len(p), 16), w[i:])
        assert b"".join(chain) == p
        assert rx_verify_chain_ref(chain, L4, L6) == want, (i, p[:24].hex(), [len(f) for f in chain])
        assert rx_verify_chain_ref(netbuffers(p), L4, L6) == want, (i, p[:24].hex())
    assert len(kinds) >= 7  # every kind of verdict is exercised


def test_the_c_oracle_gives_the_same(oracle):
    w = O.splitmix64_words(0xC4A3, 512)
    for i, p in enumerate(make_datagrams(14 * 6, 0xC4A4)):
        chain = split_even(p, max(hdr_len(p), 16), w[i:])
        assert rx_verify_chain_ref(chain, L4, L6, ones_comp=oracle.compute_ones_comp) == \
            rx_verify_chain_ref(chain, L4, L6)


def test_an_odd_split_differs_from_the_flat_value():
    """[20-byte header + 3 bytes | rest]: the 3-byte trimmed head is zero-padded on its own
    (util.rs:97-99), so the segment's words pair differently than in the flat datagram."""
    p = ipv4(6, tcp_seg(R4, L4, bytes(range(1, 64))))
    flat = O.rx_verify_ref(p, L4, L6)
    assert flat == (O.RX_IP_OK | O.RX_L4_OK | O.RX_ACCEPT, 0)
    st, l4 = rx_verify_chain_ref([p[:23], p[23:]], L4, L6)
    seg = [p[20:23], p[23:]]
    want = O.buffer_ones_comp_py(O.pseudo_header_py(R4, L4, len(p) - 20, 6), seg) ^ 0xFFFF
    assert l4 == want and l4 != flat[1]
    assert st == O.RX_IP_OK  # the header verifies, the per-fragment L4 sum does not


def test_trim_head_as_the_reference():
    assert trim_head([b"abcd", b"ef"], 4) == [b"ef"]            # a head of exactly `size` disappears
    assert trim_head([b"abcd", b"ef"], 5) == [b"f"]             # whole fragments go, the next start advances
    assert trim_head([b"abcd", b"ef"], 3) == [b"d", b"ef"]
    assert trim_head([b"abcd", b"ef"], 6) == []
    assert trim_head([b"abcd", b"ef"], 0) == [b"abcd", b"ef"]


def test_head_conditions_are_on_the_first_fragment():
    v4 = ipv4(6, tcp_seg(R4, L4, b"x" * 40))
    assert rx_verify_chain_ref([v4[:15], v4[15:]])[0] == O.RX_MALFORMED          # header[12..16]
    assert rx_verify_chain_ref([v4[:16], v4[16:]])[0] == O.RX_MALFORMED          # header[..20]
    assert rx_verify_chain_ref([v4[:20], v4[20:]]) == O.rx_verify_ref(v4, L4, L6)
    v6 = ipv6(6, tcp_seg(R6, L6, b"y" * 41))
    assert rx_verify_chain_ref([v6[:23], v6[23:]])[0] == O.RX_MALFORMED          # header[8..24]
    for len0 in (24, 26, 38, 40, 42):  # the header may run over fragments; even cuts keep the flat value
        assert rx_verify_chain_ref([v6[:len0], v6[len0:]]) == O.rx_verify_ref(v6, L4, L6)
    assert rx_verify_chain_ref([v6[:24], v6[24:39]])[0] == O.RX_MALFORMED        # T = 39: trim_head asserts
    st, l4 = rx_verify_chain_ref([v6[:24], v6[24:40]])                           # T = 40: an empty segment
    assert l4 == O.pseudo_header_py(R6, L6, 0, 6) ^ 0xFFFF and st == O.RX_IP_OK
    assert rx_verify_chain_ref([])[0] == O.RX_MALFORMED
    assert rx_verify_chain_ref([b"", v4])[0] == O.RX_MALFORMED
    assert rx_verify_chain_ref([v4[:20], b"", v4[20:]]) == O.rx_verify_ref(v4, L4, L6)  # (parity unpinned)


def test_lengths_are_the_chain_total():
    """The pseudo-header carries T - hdr (as u16 under IPv4, tcp.rs:845 / util.rs:196)."""
    body = np.arange(70000, dtype=np.uint32).astype(np.uint8).tobytes()
    p = ipv4_long(6, tcp_seg(R4, L4, body))
    assert len(p) - 20 > 65535
    assert rx_verify_chain_ref(netbuffers(p), L4, L6) == O.rx_verify_ref(p, L4, L6)
