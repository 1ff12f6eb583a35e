"""The UDP send build (rns_tx_udp_send_pool_dev) without a GPU: the symbols, the argument checks (all before
the device is touched), the GPU-less error, the CPU-tensor refusal, the flags in the header and the workspace's
size."""
import ctypes

import pytest
import torch

from abi_helper import FAKE, assert_header_compiles
from rustnetworkstack_amd import _lib, batch, udp

PTRS = ("data", "rec", "q_first", "ports", "ip4", "ip6", "pool", "free", "add", "blk_first", "head_len8", "pay_len16", "src",
        "count", "send", "work")
OPTIONAL = ("add", "src")
IP4, IP6 = bytes(4), bytes(16)


def call(lib, n=1, n_socks=2, buf_log2=9, n_free=4, cap=1, work_bytes=1 << 20, **kw):
    p = {k: kw.get(k, FAKE) for k in PTRS}
    p["ip4"], p["ip6"] = kw.get("ip4", IP4), kw.get("ip6", IP6)
    return lib.rns_tx_udp_send_pool_dev(p["data"], 1 << 20, p["rec"], n, p["q_first"], p["ports"], n_socks, p["ip4"], p["ip6"],
                                        p["pool"], 1 << 20, buf_log2, p["free"], n_free, cap, 7, p["add"], p["blk_first"],
                                        p["head_len8"], p["pay_len16"], p["src"], p["count"], p["send"], p["work"], work_bytes,
                                        None)


def work(n):
    need = ctypes.c_uint64(0)
    assert _lib.load().rns_tx_udp_send_work(n, ctypes.byref(need)) == _lib.RNS_OK
    return need.value


def test_symbols_are_bound_and_declared():
    lib = _lib.load()
    for name, argc in (("rns_tx_udp_send_pool_dev", 26), ("rns_tx_udp_send_work", 2)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    for name in ("tx_udp_send_pool", "send_host", "udp_send_work", "udp_echo", "UdpSend"):
        assert getattr(batch, name) is getattr(udp, name)
    assert (_lib.RNS_UDPTX_SEND, _lib.RNS_UDPTX_BUILT, _lib.RNS_UDPTX_NOBUF, _lib.RNS_UDPTX_BADBUF) == (1, 2, 4, 8)
    assert_header_compiles("_Static_assert(RNS_UDPTX_SEND == 1 && RNS_UDPTX_BUILT == 2 && RNS_UDPTX_NOBUF == 4 && "
                           "RNS_UDPTX_BADBUF == 8, \"flags\");\n")


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    for name in PTRS:
        if name not in OPTIONAL:
            assert call(lib, **{name: None}) == _lib.RNS_E_INVALID, name
    for ns in (0, _lib.RNS_UDP_MAX_SOCKS + 1):
        assert call(lib, n_socks=ns) == _lib.RNS_E_INVALID, ns
    for log2 in (0, 7, 16, 31):
        assert call(lib, buf_log2=log2) == _lib.RNS_E_INVALID, log2
    for name in ("data", "rec", "pool"):                                  # 16-byte alignment
        assert call(lib, **{name: ctypes.c_void_p(4096 + 8)}) == _lib.RNS_E_INVALID, name
    assert call(lib, work=ctypes.c_void_p(4096 + 4)) == _lib.RNS_E_INVALID   # 8-byte alignment
    assert call(lib, n=300, work_bytes=work(300) - 1) == _lib.RNS_E_INVALID
    assert call(lib, n=_lib.RNS_CHAIN_MAX_PACKETS + 1, work_bytes=1 << 60) == _lib.RNS_E_INVALID
    assert call(lib, n=0, count=None) == _lib.RNS_E_INVALID               # n_recs == 0 zeroes d_count


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    assert call(lib, n=0) == _lib.RNS_E_NODEVICE                          # the zeroing needs the device
    assert call(lib, n=0, n_socks=0, data=None, rec=None, pool=None, work=None, send=None) == _lib.RNS_E_NODEVICE
    assert call(lib, n=300, work_bytes=work(300)) == _lib.RNS_E_NODEVICE
    assert call(lib, add=None, src=None) == _lib.RNS_E_NODEVICE           # the optional ones
    assert call(lib, cap=0, blk_first=None, head_len8=None, pay_len16=None) == _lib.RNS_E_NODEVICE
    assert call(lib, n_free=0, free=None) == _lib.RNS_E_NODEVICE
    assert call(lib, work=ctypes.c_void_p(4096 + 8)) == _lib.RNS_E_NODEVICE
    for log2, ns in ((8, 1), (15, _lib.RNS_UDP_MAX_SOCKS)):
        assert call(lib, buf_log2=log2, n_socks=ns) == _lib.RNS_E_NODEVICE


def test_work_is_monotone():
    sizes = [work(n) for n in (0, 1, 255, 256, 257, 65536, 65537, 1 << 20)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] <= 8 << 20
    assert udp.udp_send_work(513) == work(513)
    need = ctypes.c_uint64(0)
    lib = _lib.load()
    assert lib.rns_tx_udp_send_work(1, None) == _lib.RNS_E_INVALID
    assert lib.rns_tx_udp_send_work(_lib.RNS_CHAIN_MAX_PACKETS + 1, ctypes.byref(need)) == _lib.RNS_E_INVALID


def test_wrapper_refuses_cpu_tensors():
    z = lambda n, t: torch.zeros(n, dtype=t)  # noqa: E731
    with pytest.raises(ValueError, match="GPU"):
        udp.tx_udp_send_pool(z(1024, torch.uint8), z(64, torch.uint8), z(2, torch.int32), z(1, torch.int16), IP4, IP6,
                             z(1024, torch.uint8), z(2, torch.int32))
