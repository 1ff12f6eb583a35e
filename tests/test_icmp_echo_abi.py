"""The ICMP echo responder (rns_rx_icmp_echo_pool_dev) without a GPU: the symbols, the argument checks
(all before the device is touched), the GPU-less error, the CPU-tensor refusal and the workspace's size."""
import ctypes

import numpy as np
import pytest
import torch

from abi_helper import FAKE
from rustnetworkstack_amd import _lib, batch, icmp

PTRS = ("rx", "idx", "blk", "len16", "ip4", "ip6", "tx", "free", "add", "tbf", "thl", "tpl", "src", "count", "status", "l4",
        "echo", "work")
OPTIONAL = ("add", "src", "l4")
IP4, IP6 = bytes(4), bytes(16)


def call(lib, buf_log2=9, n_frags=1, n=1, n_free=4, cap=1, work_bytes=1 << 20, **kw):
    p = {k: kw.get(k, FAKE) for k in PTRS}
    p["ip4"], p["ip6"] = kw.get("ip4", IP4), kw.get("ip6", IP6)
    return lib.rns_rx_icmp_echo_pool_dev(p["rx"], 1 << 20, buf_log2, p["idx"], n_frags, p["blk"], p["len16"], n, p["ip4"],
                                         p["ip6"], p["tx"], 1 << 20, p["free"], n_free, cap, 0, p["add"], p["tbf"], p["thl"],
                                         p["tpl"], p["src"], p["count"], p["status"], p["l4"], p["echo"], p["work"],
                                         work_bytes, None)


def work(n):
    need = ctypes.c_uint64(0)
    assert _lib.load().rns_rx_icmp_echo_work(n, ctypes.byref(need)) == _lib.RNS_OK
    return need.value


def test_symbols_are_bound_and_declared():
    lib = _lib.load()
    for name, argc in (("rns_rx_icmp_echo_pool_dev", 28), ("rns_rx_icmp_echo_work", 2)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    for name in ("rx_icmp_echo_pool", "echo_host", "echo_respond", "echo_work"):
        assert getattr(batch, name) is getattr(icmp, name)
    assert (_lib.RNS_ECHO_REQUEST, _lib.RNS_ECHO_BUILT, _lib.RNS_ECHO_NOBUF, _lib.RNS_ECHO_BADBUF) == (1, 2, 4, 8)


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    for name in PTRS:
        want = _lib.RNS_E_INVALID
        if name in OPTIONAL:
            continue
        assert call(lib, **{name: None}) == want, name
    assert call(lib, free=None, n_free=4) == _lib.RNS_E_INVALID          # a NULL d_free with n_free > 0
    for name in ("tbf", "thl", "tpl"):                                   # the outputs may be NULL iff reply_cap == 0
        assert call(lib, cap=5, **{name: None}) == _lib.RNS_E_INVALID
    for log2 in (0, 7, 16, 31):
        assert call(lib, buf_log2=log2) == _lib.RNS_E_INVALID, log2
    assert call(lib, rx=ctypes.c_void_p(4096 + 8)) == _lib.RNS_E_INVALID     # a pool that is not 16-byte aligned
    assert call(lib, tx=ctypes.c_void_p(4096 + 8)) == _lib.RNS_E_INVALID
    assert call(lib, work=ctypes.c_void_p(4096 + 4)) == _lib.RNS_E_INVALID
    assert call(lib, n=300, work_bytes=work(300) - 1) == _lib.RNS_E_INVALID
    assert call(lib, n=_lib.RNS_CHAIN_MAX_PACKETS + 1) == _lib.RNS_E_INVALID
    assert call(lib, n=0, count=None) == _lib.RNS_E_INVALID              # n_pkts == 0 zeroes d_count


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    assert call(lib, n=300, work_bytes=work(300)) == _lib.RNS_E_NODEVICE
    assert call(lib, cap=0, tbf=None, thl=None, tpl=None, src=None) == _lib.RNS_E_NODEVICE
    assert call(lib, n_free=0, free=None, n_frags=0, idx=None, add=None, l4=None) == _lib.RNS_E_NODEVICE
    for log2 in (8, 15):
        assert call(lib, buf_log2=log2) == _lib.RNS_E_NODEVICE


def test_work_is_monotone_and_non_zero():
    sizes = [work(n) for n in (0, 1, 63, 64, 255, 256, 257, 4096, 1 << 20, _lib.RNS_CHAIN_MAX_PACKETS)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert [icmp.echo_work(n) for n in (0, 257)] == [sizes[0], sizes[6]]
    need = ctypes.c_uint64(0)
    lib = _lib.load()
    assert lib.rns_rx_icmp_echo_work(1, None) == _lib.RNS_E_INVALID
    assert lib.rns_rx_icmp_echo_work(_lib.RNS_CHAIN_MAX_PACKETS + 1, ctypes.byref(need)) == _lib.RNS_E_INVALID


def test_wrapper_refuses_cpu_tensors():
    z = lambda n, t: torch.zeros(n, dtype=t)  # noqa: E731
    with pytest.raises(ValueError, match="GPU"):
        icmp.rx_icmp_echo_pool(z(1024, torch.uint8), z(2, torch.int32), z(1, torch.int32), z(1, torch.int16), IP4, IP6,
                               z(1024, torch.uint8), z(2, torch.int32))
    assert np.dtype(np.uint8).itemsize == 1
