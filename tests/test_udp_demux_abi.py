"""The UDP receive demux (rns_rx_udp_demux_pool_dev) without a GPU: the symbols, the argument checks (all
before the device is touched), the GPU-less error, the CPU-tensor refusal, the record's layout in the
header and the workspace's size."""
import ctypes

import pytest
import torch

from abi_helper import FAKE, assert_header_compiles, assert_header_defines
from rustnetworkstack_amd import _lib, batch, udp

PTRS = ("pool", "idx", "blk", "len16", "ip4", "ip6", "tbl", "data", "rec", "q_first", "count", "status", "l4", "udp", "pos",
        "work")
OPTIONAL = ("l4", "pos")
IP4, IP6 = bytes(4), bytes(16)


def call(lib, buf_log2=9, n_frags=1, n=1, n_socks=2, data_bytes=1 << 20, cap=1, work_bytes=1 << 20, **kw):
    p = {k: kw.get(k, FAKE) for k in PTRS}
    p["ip4"], p["ip6"] = kw.get("ip4", IP4), kw.get("ip6", IP6)
    return lib.rns_rx_udp_demux_pool_dev(p["pool"], 1 << 20, buf_log2, p["idx"], n_frags, p["blk"], p["len16"], n, p["ip4"],
                                         p["ip6"], p["tbl"], n_socks, p["data"], data_bytes, p["rec"], cap, p["q_first"],
                                         p["count"], p["status"], p["l4"], p["udp"], p["pos"], p["work"], work_bytes, None)


def work(n, s):
    need = ctypes.c_uint64(0)
    assert _lib.load().rns_rx_udp_demux_work(n, s, ctypes.byref(need)) == _lib.RNS_OK
    return need.value


def test_symbols_are_bound_and_declared():
    lib = _lib.load()
    for name, argc in (("rns_rx_udp_demux_pool_dev", 25), ("rns_rx_udp_demux_work", 3), ("rns_rx_udp_port_table_build", 3)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    for name in ("rx_udp_demux_pool", "demux_host", "demux_work", "drain", "port_table", "udp_demux"):
        assert getattr(batch, name) is getattr(udp, name)
    assert_header_defines(["RNS_UDP_MAX_SOCKS"])
    assert (_lib.RNS_UDP_DGRAM, _lib.RNS_UDP_SOCK, _lib.RNS_UDP_QUEUED, _lib.RNS_UDP_NOROOM) == (1, 2, 4, 8)
    assert _lib.RNS_UDP_NO_SOCK == 0xFFFF >= _lib.RNS_UDP_MAX_SOCKS


def test_the_record_is_32_bytes_in_c():
    assert_header_compiles("#include <stddef.h>\n"
                           "_Static_assert(sizeof(rns_udp_rec) == 32 && offsetof(rns_udp_rec, src) == 16 && "
                           "offsetof(rns_udp_rec, off16) == 20 && offsetof(rns_udp_rec, sport) == 24 && "
                           "offsetof(rns_udp_rec, len) == 26 && offsetof(rns_udp_rec, family) == 28 && "
                           "offsetof(rns_udp_rec, flags) == 29, \"rns_udp_rec\");\n"
                           "_Static_assert(RNS_UDP_NO_SOCK == 0xffffu && RNS_UDP_DGRAM == 1 && RNS_UDP_SOCK == 2 && "
                           "RNS_UDP_QUEUED == 4 && RNS_UDP_NOROOM == 8, \"flags\");\n")
    assert [udp.REC.fields[k][1] for k in ("src", "off16", "sport", "len", "family", "flags")] == [16, 20, 24, 26, 28, 29]


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    for name in PTRS:
        if name not in OPTIONAL:
            assert call(lib, **{name: None}) == _lib.RNS_E_INVALID, name
    assert call(lib, n_socks=_lib.RNS_UDP_MAX_SOCKS + 1) == _lib.RNS_E_INVALID
    assert call(lib, n=0, n_socks=_lib.RNS_UDP_MAX_SOCKS + 1) == _lib.RNS_E_INVALID
    for log2 in (0, 6, 16, 31):
        assert call(lib, buf_log2=log2) == _lib.RNS_E_INVALID, log2
    for name in ("pool", "data", "rec", "work"):                         # 16-byte alignment
        assert call(lib, **{name: ctypes.c_void_p(4096 + 8)}) == _lib.RNS_E_INVALID, name
    assert call(lib, n=300, work_bytes=work(300, 2) - 1) == _lib.RNS_E_INVALID
    assert call(lib, n=300, n_socks=1000, work_bytes=work(300, 2)) == _lib.RNS_E_INVALID
    assert call(lib, n=_lib.RNS_CHAIN_MAX_PACKETS + 1, work_bytes=1 << 60) == _lib.RNS_E_INVALID
    assert call(lib, buf_log2=9, n_frags=1 << 27) == _lib.RNS_E_INVALID  # n_frags << buf_log2 == 2^36
    assert call(lib, buf_log2=15, n_frags=1 << 21) == _lib.RNS_E_INVALID
    assert call(lib, n=0, count=None) == _lib.RNS_E_INVALID              # n_pkts == 0 zeroes d_count and d_q_first
    assert call(lib, n=0, q_first=None) == _lib.RNS_E_INVALID


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    assert call(lib, n=0) == _lib.RNS_E_NODEVICE                         # the zeroing needs the device
    assert call(lib, n=300, work_bytes=work(300, 2)) == _lib.RNS_E_NODEVICE
    assert call(lib, n_socks=0, tbl=None, l4=None, pos=None) == _lib.RNS_E_NODEVICE
    assert call(lib, data_bytes=0, data=None, cap=0, rec=None) == _lib.RNS_E_NODEVICE
    assert call(lib, buf_log2=9, n_frags=(1 << 27) - 1) == _lib.RNS_E_NODEVICE
    for log2 in (7, 15):
        assert call(lib, buf_log2=log2) == _lib.RNS_E_NODEVICE


def test_work_is_monotone_and_bounded():
    sizes = [work(n, 1024) for n in (0, 1, 511, 512, 513, 4096, 1 << 20)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] <= 64 << 20
    assert [work(1 << 16, s) for s in (0, 1, 2, 1024)] == sorted(work(1 << 16, s) for s in (0, 1, 2, 1024))
    assert udp.demux_work(513, 7) == work(513, 7)
    need = ctypes.c_uint64(0)
    lib = _lib.load()
    assert lib.rns_rx_udp_demux_work(1, 1, None) == _lib.RNS_E_INVALID
    assert lib.rns_rx_udp_demux_work(_lib.RNS_CHAIN_MAX_PACKETS + 1, 1, ctypes.byref(need)) == _lib.RNS_E_INVALID
    assert lib.rns_rx_udp_demux_work(1, _lib.RNS_UDP_MAX_SOCKS + 1, ctypes.byref(need)) == _lib.RNS_E_INVALID


def test_port_table_arguments():
    lib = _lib.load()
    tbl = (ctypes.c_uint16 * 65536)()
    ports = (ctypes.c_uint16 * 3)(7, 9, 7)
    assert lib.rns_rx_udp_port_table_build(ports, 2, tbl) == _lib.RNS_OK and tbl[7] == 0 and tbl[9] == 1 and tbl[8] == 0xFFFF
    assert lib.rns_rx_udp_port_table_build(ports, 3, tbl) == _lib.RNS_E_INVALID       # a duplicate port
    assert lib.rns_rx_udp_port_table_build(ports, 2, None) == _lib.RNS_E_INVALID
    assert lib.rns_rx_udp_port_table_build(None, 2, tbl) == _lib.RNS_E_INVALID
    assert lib.rns_rx_udp_port_table_build(None, 0, tbl) == _lib.RNS_OK and tbl[7] == 0xFFFF
    assert lib.rns_rx_udp_port_table_build(ports, _lib.RNS_UDP_MAX_SOCKS + 1, tbl) == _lib.RNS_E_INVALID


def test_wrapper_refuses_cpu_tensors():
    z = lambda n, t: torch.zeros(n, dtype=t)  # noqa: E731
    with pytest.raises(ValueError, match="GPU"):
        udp.rx_udp_demux_pool(z(1024, torch.uint8), z(2, torch.int32), z(1, torch.int32), z(1, torch.int16), IP4, IP6,
                              z(65536, torch.int16), 1)
