"""The TCP listen responder (rns_rx_tcp_listen_pool_dev) without a GPU: the symbols, the argument checks (all
before the device is touched), the GPU-less error, the CPU-tensor refusal, the flags and the record in the header
and the workspace's size."""
import ctypes

import pytest
import torch

from abi_helper import FAKE, assert_header_compiles
from rustnetworkstack_amd import _lib, batch, listen

PTRS = ("pool", "buf_idx", "blk_first", "len16", "ip4", "ip6", "meta", "listen", "iss", "add", "out", "rep_src", "rep_len8",
        "accept", "count", "conn", "work")
OPTIONAL = ("add",)
IP4, IP6 = bytes(4), bytes(16)


def call(lib, n=1, n_frags=1, buf_log2=9, n_listen=2, cap=1, work_bytes=1 << 20, **kw):
    p = {k: kw.get(k, FAKE) for k in PTRS}
    p["ip4"], p["ip6"] = kw.get("ip4", IP4), kw.get("ip6", IP6)
    return lib.rns_rx_tcp_listen_pool_dev(p["pool"], 1 << 20, buf_log2, p["buf_idx"], n_frags, p["blk_first"], p["len16"], n,
                                          p["ip4"], p["ip6"], p["meta"], p["listen"], n_listen, p["iss"], 7, p["add"], p["out"],
                                          cap, p["rep_src"], p["rep_len8"], p["accept"], p["count"], p["conn"], p["work"],
                                          work_bytes, None)


def work(n):
    need = ctypes.c_uint64(0)
    assert _lib.load().rns_rx_tcp_listen_work(n, ctypes.byref(need)) == _lib.RNS_OK
    return need.value


def test_symbols_are_bound_and_declared():
    lib = _lib.load()
    for name, argc in (("rns_rx_tcp_listen_pool_dev", 26), ("rns_rx_tcp_listen_work", 2)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    for name in ("rx_tcp_listen_pool", "listen_host", "listen_work", "tcp_listen", "accept_merge", "TcpListen"):
        assert getattr(batch, name) is getattr(listen, name)
    assert (_lib.RNS_CONN_UNMATCHED, _lib.RNS_CONN_SYN, _lib.RNS_CONN_LATER, _lib.RNS_CONN_RST, _lib.RNS_CONN_BUILT,
            _lib.RNS_CONN_NOBUF, _lib.RNS_CONN_HOST, _lib.RNS_TCP_SYN_RECEIVED) == (1, 2, 4, 8, 16, 32, 64, 2)
    assert listen.ACCEPT_DTYPE.itemsize == 72
    assert_header_compiles("_Static_assert(RNS_CONN_UNMATCHED == 1 && RNS_CONN_SYN == 2 && RNS_CONN_LATER == 4 && RNS_CONN_RST == 8 && "
                           "RNS_CONN_BUILT == 16 && RNS_CONN_NOBUF == 32 && RNS_CONN_HOST == 64 && RNS_TCP_SYN_RECEIVED == 2 && "
                           "sizeof(rns_tcp_accept) == 72, \"flags and record\");\n")


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    for name in PTRS:
        if name not in OPTIONAL:
            assert call(lib, **{name: None}) == _lib.RNS_E_INVALID, name
    assert call(lib, n_listen=_lib.RNS_UDP_MAX_SOCKS + 1) == _lib.RNS_E_INVALID
    for log2 in (0, 6, 16, 31):
        assert call(lib, buf_log2=log2) == _lib.RNS_E_INVALID, log2
    assert call(lib, pool=ctypes.c_void_p(4096 + 8)) == _lib.RNS_E_INVALID        # 16-byte alignment
    for name in ("meta", "accept", "out", "count"):                               # 4-byte alignment
        assert call(lib, **{name: ctypes.c_void_p(4096 + 2)}) == _lib.RNS_E_INVALID, name
    assert call(lib, work=ctypes.c_void_p(4096 + 4)) == _lib.RNS_E_INVALID        # 8-byte alignment
    assert call(lib, n=300, work_bytes=work(300) - 1) == _lib.RNS_E_INVALID
    assert call(lib, n=_lib.RNS_CHAIN_MAX_PACKETS + 1, work_bytes=1 << 60) == _lib.RNS_E_INVALID
    assert call(lib, n=0, count=None) == _lib.RNS_E_INVALID                       # n_pkts == 0 zeroes d_count


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    assert call(lib, n=0) == _lib.RNS_E_NODEVICE                                  # the zeroing needs the device
    assert call(lib, n=0, pool=None, meta=None, work=None, conn=None, listen=None, n_listen=0) == _lib.RNS_E_NODEVICE
    assert call(lib, n=300, work_bytes=work(300)) == _lib.RNS_E_NODEVICE
    assert call(lib, add=None) == _lib.RNS_E_NODEVICE                             # the optional one
    assert call(lib, cap=0, out=None, rep_src=None, rep_len8=None, accept=None, iss=None) == _lib.RNS_E_NODEVICE
    assert call(lib, n_listen=0, listen=None) == _lib.RNS_E_NODEVICE
    assert call(lib, n_frags=0, buf_idx=None) == _lib.RNS_E_NODEVICE
    assert call(lib, work=ctypes.c_void_p(4096 + 8)) == _lib.RNS_E_NODEVICE
    for log2, nl in ((7, 1), (15, _lib.RNS_UDP_MAX_SOCKS)):
        assert call(lib, buf_log2=log2, n_listen=nl) == _lib.RNS_E_NODEVICE


def test_work_is_monotone():
    sizes = [work(n) for n in (0, 1, 32, 33, 255, 256, 257, 65536, 65537, 1 << 20)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] <= 29 << 20
    assert listen.listen_work(513) == work(513)
    assert work(300) >= 16 * 3 + 12 * listen.listen_slots(300) + 4 * 300
    need = ctypes.c_uint64(0)
    lib = _lib.load()
    assert lib.rns_rx_tcp_listen_work(1, None) == _lib.RNS_E_INVALID
    assert lib.rns_rx_tcp_listen_work(_lib.RNS_CHAIN_MAX_PACKETS + 1, ctypes.byref(need)) == _lib.RNS_E_INVALID


def test_wrapper_refuses_cpu_tensors():
    z = lambda n, t: torch.zeros(n, dtype=t)  # noqa: E731
    with pytest.raises(ValueError, match="GPU"):
        listen.rx_tcp_listen_pool(z(1024, torch.uint8), z(2, torch.int32), z(1, torch.int32), z(1, torch.int16), IP4, IP6,
                                  z(24, torch.uint8), z(65536, torch.int16), 1, z(1, torch.int32))
