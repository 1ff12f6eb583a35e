"""TCP receive placement (rns_rx_tcp_place_pool_dev) without a GPU: the symbols, the argument checks
(all before the device is touched), the GPU-less error, the CPU-tensor refusal, and the flow table's
host-side builder (rns_rx_flow_table_build) against a pure-Python probe of the layout the header
documents."""
import ctypes

import numpy as np
import pytest

from abi_helper import FAKE
from rustnetworkstack_amd import _lib, batch, place

PTRS = ("pool", "idx", "blk", "len16", "ip4", "ip6", "tbl", "nseq", "woff", "wlen", "stream", "status", "meta")
IP4, IP6 = bytes(4), bytes(16)


def call(lib, buf_log2=9, n_frags=1, n=1, tbl_bytes=2048, n_flows=1, l4=None, **kw):
    p = {k: kw.get(k, FAKE) for k in PTRS}
    p["ip4"], p["ip6"] = kw.get("ip4", IP4), kw.get("ip6", IP6)
    return lib.rns_rx_tcp_place_pool_dev(p["pool"], 1 << 20, buf_log2, p["idx"], n_frags, p["blk"], p["len16"], n,
                                         p["ip4"], p["ip6"], p["tbl"], tbl_bytes, p["nseq"], p["woff"], p["wlen"],
                                         n_flows, p["stream"], 4096, p["status"], l4, p["meta"], None)


def test_symbols_are_bound_and_declared():
    lib = _lib.load()
    for name, argc in (("rns_rx_tcp_place_pool_dev", 22), ("rns_rx_flow_table_build", 5)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    for name in ("rx_tcp_place_pool", "rx_flow_table", "Reassembler", "META_DTYPE"):
        assert getattr(batch, name) is getattr(place, name)
    assert place.META_DTYPE.itemsize == 24 and place.KEY_DTYPE.itemsize == 24
    assert (_lib.RNS_RX_NO_FLOW, _lib.RNS_PLACE_TCP, _lib.RNS_PLACE_FLOW, _lib.RNS_PLACE_DONE,
            _lib.RNS_PLACE_OUTSIDE) == (0xFFFFFFFF, 1, 2, 4, 8)


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    assert call(lib, n=0) == _lib.RNS_OK
    assert call(lib, n=0, **{k: None for k in PTRS}) == _lib.RNS_OK
    for name in PTRS:
        if name != "idx":
            assert call(lib, **{name: None}) == _lib.RNS_E_INVALID, name
    assert call(lib, idx=None) == _lib.RNS_E_INVALID                 # a NULL d_buf_idx with n_frags > 0
    for log2 in (0, 6, 16, 31):                                      # the verify's 6 is too small here
        assert call(lib, buf_log2=log2) == _lib.RNS_E_INVALID, log2
    assert call(lib, pool=ctypes.c_void_p(4096 + 8)) == _lib.RNS_E_INVALID   # not 16-byte aligned
    assert call(lib, meta=ctypes.c_void_p(4096 + 2)) == _lib.RNS_E_INVALID
    assert call(lib, tbl=ctypes.c_void_p(4096 + 1)) == _lib.RNS_E_INVALID
    assert call(lib, tbl_bytes=2047) == _lib.RNS_E_INVALID           # below the need for one flow
    assert call(lib, n_flows=33, tbl_bytes=2048) == _lib.RNS_E_INVALID      # 33 flows need 128 slots
    assert call(lib, n=_lib.RNS_CHAIN_MAX_PACKETS + 1) == _lib.RNS_E_INVALID


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    for log2 in (7, 15):
        assert call(lib, buf_log2=log2, l4=FAKE) == _lib.RNS_E_NODEVICE
    assert call(lib, idx=None, n_frags=0) == _lib.RNS_E_NODEVICE
    assert call(lib, tbl=None, tbl_bytes=0, n_flows=0) == _lib.RNS_E_NODEVICE  # no flows: the table is not wanted
    assert call(lib, n=_lib.RNS_CHAIN_MAX_PACKETS, n_flows=32) == _lib.RNS_E_NODEVICE


def test_python_wrapper_refuses_cpu_tensors():
    import torch
    z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="no CPU fallback"):
        place.rx_tcp_place_pool(z(1024, torch.uint8), z(1, torch.int32), z(1, torch.int32), z(1, torch.int16), IP4, IP6,
                                z(2048, torch.uint8), z(1, torch.int32), z(1, torch.int64), z(1, torch.int32),
                                z(64, torch.uint8))


# --- the flow table -----------------------------------------------------------------------------
def keys_for(n, seed=1):
    """n distinct keys: IPv4 and IPv6 sources, and runs that differ in one field only."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        k = len(out) % 4
        ip = bytes(rng.integers(0, 256, 4 if k < 2 else 16, dtype=np.uint8))
        base = (ip, int(rng.integers(0, 65536)), int(rng.integers(0, 65536)))
        for cand in (base, (base[0], base[1] ^ 1, base[2]), (base[0], base[1], base[2] ^ 1),
                     (base[0] + bytes(12), base[1], base[2]) if len(ip) == 4 else base):
            if cand not in seen and len(out) < n:
                seen.add(cand)
                out.append(cand)
    return out


def key_words(ip, sport, dport):
    raw = bytes(ip) + bytes(16 - len(ip))
    return [int.from_bytes(raw[4 * i:4 * i + 4], "little") for i in range(4)] + [sport | dport << 16,
                                                                                  4 if len(ip) == 4 else 6]


def probe(tbl, n_flows, ip, sport, dport):
    """The documented layout, probed in Python: the key's flow index or None."""
    w = np.frombuffer(tbl.tobytes(), dtype="<u4").reshape(-1, 8)
    slots = w.shape[0]
    assert slots >= 64 and slots & (slots - 1) == 0 and slots >= 2 * n_flows
    k = key_words(ip, sport, dport)
    h = 0x9E3779B9
    for x in k:
        h = ((h ^ x) * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 15
    s = h & (slots - 1)
    for _ in range(slots):
        if w[s, 7] == 0:
            return None
        if w[s, 7] == 1 and w[s, :6].tolist() == k and w[s, 6] < n_flows:
            return int(w[s, 6])
        s = (s + 1) & (slots - 1)
    return None


@pytest.mark.parametrize("n", [0, 1, 32, 33, 65, 5000])
def test_table_finds_every_key_and_no_other(n):
    lib = _lib.load()
    keys = keys_for(n, seed=n)
    arr = place._keys(keys)
    need = ctypes.c_uint64(7)
    assert lib.rns_rx_flow_table_build(arr.ctypes.data, n, None, 0, ctypes.byref(need)) == _lib.RNS_OK  # the size query
    slots = 64
    while slots < 2 * n:
        slots *= 2
    assert need.value == 32 * slots
    guard = 64
    buf = np.full(need.value + guard, 0xC3, dtype=np.uint8)
    assert lib.rns_rx_flow_table_build(arr.ctypes.data, n, buf.ctypes.data, need.value, ctypes.byref(need)) == _lib.RNS_OK
    assert (buf[need.value:] == 0xC3).all(), "written past the table"
    tbl = buf[:need.value]
    assert np.array_equal(tbl, place.rx_flow_table(keys))            # the wrapper
    for f, k in enumerate(keys):
        assert probe(tbl, n, *k) == f
    rng = np.random.default_rng(99)
    have, absent = set(keys), 0
    while absent < 1000:
        ip = bytes(rng.integers(0, 256, 4 if absent % 2 else 16, dtype=np.uint8))
        k = (ip, int(rng.integers(0, 65536)), int(rng.integers(0, 65536)))
        if k in have:
            continue
        assert probe(tbl, n, *k) is None
        absent += 1
    if n >= 2:                                                       # key order changes slots, not what is found
        perm = np.random.default_rng(5).permutation(n)
        tbl2 = place.rx_flow_table([keys[i] for i in perm])
        for new, old in enumerate(perm):
            assert probe(tbl2, n, *keys[old]) == new
        assert probe(tbl, n - 1, *keys[n - 1]) is None               # a stored flow >= n_flows is no match


def test_table_rejects():
    lib = _lib.load()
    need = ctypes.c_uint64(0)
    buf = np.zeros(4096, dtype=np.uint8)

    def build(arr, n=None, tbl_bytes=4096, need_ref=True):
        return lib.rns_rx_flow_table_build(arr.ctypes.data, arr.size if n is None else n, buf.ctypes.data, tbl_bytes,
                                           ctypes.byref(need) if need_ref else None)

    good = place._keys([(bytes([1, 2, 3, 4]), 5, 6), (bytes(range(16)), 5, 6)])
    assert build(good) == _lib.RNS_OK and need.value == 2048
    assert build(good, need_ref=False) == _lib.RNS_E_INVALID         # a NULL need_bytes
    assert build(good, tbl_bytes=2047) == _lib.RNS_E_INVALID         # below the need
    assert lib.rns_rx_flow_table_build(None, 2, buf.ctypes.data, 4096, ctypes.byref(need)) == _lib.RNS_E_INVALID
    dup = place._keys([(bytes([1, 2, 3, 4]), 5, 6), (bytes([9, 9, 9, 9]), 1, 1), (bytes([1, 2, 3, 4]), 5, 6)])
    assert build(dup) == _lib.RNS_E_INVALID
    for field, value in (("family", 5), ("family", 0), ("pad", [0, 0, 1]), ("pad", [1, 0, 0])):
        bad = good.copy()
        bad[field][1] = value
        assert build(bad) == _lib.RNS_E_INVALID, (field, value)
    bad = good.copy()
    bad["ip"][0, 15] = 1                                             # family 4 with bytes past ip[4]
    assert build(bad) == _lib.RNS_E_INVALID
    same4, same6 = bytes([1, 2, 3, 4]), bytes([1, 2, 3, 4]) + bytes(12)
    both = place._keys([(same4, 5, 6), (same6, 5, 6)])               # equal bytes, another family: two keys
    assert build(both) == _lib.RNS_OK
    with pytest.raises(_lib.ChecksumError):
        place.rx_flow_table([(same4, 5, 6), (same4, 5, 6)])
    with pytest.raises(ValueError):
        place.rx_flow_table([(bytes(5), 5, 6)])
    with pytest.raises(ValueError):
        place.rx_flow_table([(same4, 70000, 6)])
