"""The TCP flow update and the ACK build (rns_rx_tcp_flow_update_dev, rns_tx_ack_build_dev) without a
GPU: the symbols, the constants and record sizes, the argument checks (all before the device is
touched), the GPU-less error, the workspace helper and the CPU-tensor refusal."""
import ctypes

import pytest

from abi_helper import BIG, FAKE, ODD, assert_header_compiles, assert_header_defines
from rustnetworkstack_amd import _lib, flow

UPD = ("meta", "flow_in", "pend_in", "flow_out", "pend_out", "seg", "res", "work")
ACKP = ("meta", "seg", "flow", "tmpl", "hl8", "work", "out", "src", "len8", "nacks")


def update(lib, n=3, nfl=2, cap=4, work_bytes=BIG, **kw):
    p = {k: kw.get(k, FAKE) for k in UPD}
    return lib.rns_rx_tcp_flow_update_dev(p["meta"], n, nfl, p["flow_in"], p["pend_in"], cap, p["flow_out"], p["pend_out"],
                                          p["seg"], p["res"], p["work"], work_bytes, None)


def build(lib, n=3, nfl=2, stride=64, cap=4, work_bytes=BIG, **kw):
    p = {k: kw.get(k, FAKE) for k in ACKP}
    return lib.rns_tx_ack_build_dev(p["meta"], p["seg"], n, p["flow"], nfl, p["tmpl"], stride, p["hl8"], 0xFFFE, p["work"],
                                    work_bytes, p["out"], cap, p["src"], p["len8"], p["nacks"], None)


def need(lib, n, nfl):
    b = ctypes.c_uint64(0)
    assert lib.rns_rx_tcp_flow_update_work(n, nfl, ctypes.byref(b)) == _lib.RNS_OK
    return b.value


def test_symbols_constants_and_sizes():
    lib = _lib.load()
    for name, argc in (("rns_rx_tcp_flow_update_dev", 13), ("rns_rx_tcp_flow_update_work", 3), ("rns_tx_ack_build_dev", 17)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    assert (flow.FLOW_DTYPE.itemsize, flow.SEG_DTYPE.itemsize, flow.RES_DTYPE.itemsize) == (40, 8, 24)
    assert_header_defines(("RNS_TCP_ESTABLISHED", "RNS_FLOW_MAX_SEGS", "RNS_SEG_CONSUMED", "RNS_SEG_ACK", "RNS_SEG_TIMER",
                           "RNS_EV_WND", "RNS_STOP_NONE", "RNS_STOP_MANY", "RNS_STOP_STATE", "RNS_STOP_FLAGS", "RNS_STOP_OPTIONS",
                           "RNS_STOP_OUTSIDE", "RNS_STOP_PEND"))
    assert_header_compiles("_Static_assert(sizeof(rns_tcp_flow) == 40 && sizeof(rns_rx_tcp_seg) == 8 && "
                           "sizeof(rns_tcp_flow_res) == 24, \"\");\nint main(void){ return 0; }\n")


def test_update_argument_checks_come_before_the_device():
    lib = _lib.load()
    assert update(lib, n=0, nfl=0, **{k: None for k in UPD}) == _lib.RNS_OK
    for name in UPD:
        assert update(lib, **{name: None}) == _lib.RNS_E_INVALID, name
        assert update(lib, **{name: ODD}) == _lib.RNS_E_INVALID, name
    assert update(lib, work=ctypes.c_void_p(4096 + 4)) == _lib.RNS_E_INVALID     # the workspace: 8-byte aligned
    assert update(lib, work_bytes=need(lib, 3, 2) - 1) == _lib.RNS_E_INVALID
    assert update(lib, work_bytes=0) == _lib.RNS_E_INVALID
    assert update(lib, n=_lib.RNS_CHAIN_MAX_PACKETS + 1) == _lib.RNS_E_INVALID
    assert update(lib, nfl=2 ** 31) == _lib.RNS_E_INVALID
    assert update(lib, n=0, meta=None, seg=None, flow_in=None) == _lib.RNS_E_INVALID   # flows still get their records
    assert update(lib, nfl=0, meta=None) == _lib.RNS_E_INVALID


def test_build_argument_checks_come_before_the_device():
    lib = _lib.load()
    for name in ACKP:
        assert build(lib, **{name: None}) == _lib.RNS_E_INVALID, name
    for name in ("meta", "seg", "flow", "out", "src", "nacks", "work"):
        assert build(lib, **{name: ODD}) == _lib.RNS_E_INVALID, name
    assert build(lib, stride=0) == _lib.RNS_E_INVALID
    assert build(lib, work_bytes=8 * 2 - 1) == _lib.RNS_E_INVALID                # one block of datagrams: two pairs
    assert build(lib, n=_lib.RNS_CHAIN_MAX_PACKETS + 1) == _lib.RNS_E_INVALID
    assert build(lib, n=0, nacks=None) == _lib.RNS_E_INVALID                     # the counts are always written


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert update(lib) == _lib.RNS_E_NODEVICE
    assert update(lib, work_bytes=need(lib, 3, 2)) == _lib.RNS_E_NODEVICE
    assert update(lib, cap=0, pend_in=None, pend_out=None) == _lib.RNS_E_NODEVICE   # no pending lists wanted
    assert update(lib, n=0, meta=None, seg=None) == _lib.RNS_E_NODEVICE
    assert update(lib, nfl=0, flow_in=None, flow_out=None, res=None, pend_in=None, pend_out=None) == _lib.RNS_E_NODEVICE
    assert build(lib) == _lib.RNS_E_NODEVICE
    assert build(lib, cap=0, out=None, src=None, len8=None) == _lib.RNS_E_NODEVICE   # counting only
    assert build(lib, nfl=0, flow=None, tmpl=None, hl8=None, stride=0) == _lib.RNS_E_NODEVICE
    assert build(lib, n=0, meta=None, seg=None, work=None, work_bytes=0) == _lib.RNS_E_NODEVICE
    assert build(lib, work_bytes=need(lib, 3, 0)) == _lib.RNS_E_NODEVICE         # the update's workspace serves


def test_workspace_helper_is_monotone():
    lib = _lib.load()
    ns = (0, 1, 255, 256, 257, 70000, 1 << 20, 1 << 23, _lib.RNS_CHAIN_MAX_PACKETS)
    fs = (0, 1, 255, 256, 257, 70000, 1 << 20, 2 ** 31 - 1)
    grid = [[need(lib, n, f) for f in fs] for n in ns]
    for i in range(len(ns)):
        for j in range(len(fs)):
            assert grid[i][j] >= 4 * (ns[i] + 2 * fs[j])            # the lists and two dwords per flow at least
            assert i == 0 or grid[i][j] >= grid[i - 1][j]
            assert j == 0 or grid[i][j] >= grid[i][j - 1]
    assert flow.flow_update_work(1 << 20, 1024) == need(lib, 1 << 20, 1024)
    b = ctypes.c_uint64(0)
    assert lib.rns_rx_tcp_flow_update_work(1, 1, None) == _lib.RNS_E_INVALID
    assert lib.rns_rx_tcp_flow_update_work(_lib.RNS_CHAIN_MAX_PACKETS + 1, 1, ctypes.byref(b)) == _lib.RNS_E_INVALID
    assert lib.rns_rx_tcp_flow_update_work(1, 2 ** 31, ctypes.byref(b)) == _lib.RNS_E_INVALID


def test_python_wrappers_refuse_cpu_tensors():
    import torch
    z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="no CPU fallback"):
        flow.rx_tcp_flow_update(z(48), z(40), None, pend_cap=0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        flow.tx_ack_build(z(48), z(16), z(40), z((1, 64)), z(1), 0, ack_cap=4)
