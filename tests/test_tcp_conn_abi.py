"""The TCP connection update, the control-segment build and the close step (rns_rx_tcp_conn_update_dev,
rns_tx_tcp_ctl_build_dev, rns_tx_tcp_close_dev) without a GPU: the symbols, the constants and record sizes, every
argument error of the three entries and both workspace helpers (all before the device is touched), the GPU-less
error, the helpers' monotony and the CPU-tensor refusal."""
import ctypes

import pytest

from abi_helper import BIG, FAKE, ODD, assert_header_compiles, assert_header_defines
from rustnetworkstack_amd import _lib, conn, flow

UPD = ("meta", "flow_in", "pend_in", "flow_out", "pend_out", "ctl", "res", "work")
BLD = ("ctl", "tmpl", "hl8", "add", "work", "out", "src", "len8", "count")
CLS = ("flow_in", "flow_out", "op", "ctl")


def update(lib, n=3, nfl=2, cap=4, work_bytes=BIG, **kw):
    p = {k: kw.get(k, FAKE) for k in UPD}
    return lib.rns_rx_tcp_conn_update_dev(p["meta"], n, nfl, p["flow_in"], p["pend_in"], cap, p["flow_out"], p["pend_out"],
                                          p["ctl"], p["res"], p["work"], work_bytes, None)


def build(lib, n=3, nfl=2, stride=64, cap=4, work_bytes=BIG, **kw):
    p = {k: kw.get(k, FAKE) for k in BLD}
    return lib.rns_tx_tcp_ctl_build_dev(p["ctl"], n, nfl, p["tmpl"], stride, p["hl8"], 0xFFFE, p["add"], p["work"], work_bytes,
                                        p["out"], cap, p["src"], p["len8"], p["count"], None)


def close(lib, nfl=2, **kw):
    p = {k: kw.get(k, FAKE) for k in CLS}
    return lib.rns_tx_tcp_close_dev(p["flow_in"], p["flow_out"], nfl, p["op"], p["ctl"], None)


def need(lib, n, nfl):
    b = ctypes.c_uint64(0)
    assert lib.rns_rx_tcp_conn_update_work(n, nfl, ctypes.byref(b)) == _lib.RNS_OK
    return b.value


def need_build(lib, n):
    b = ctypes.c_uint64(0)
    assert lib.rns_tx_tcp_ctl_build_work(n, ctypes.byref(b)) == _lib.RNS_OK
    return b.value


def test_symbols_constants_and_sizes():
    lib = _lib.load()
    for name, argc in (("rns_rx_tcp_conn_update_dev", 13), ("rns_rx_tcp_conn_update_work", 3), ("rns_tx_tcp_ctl_build_dev", 16),
                       ("rns_tx_tcp_ctl_build_work", 2), ("rns_tx_tcp_close_dev", 6)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    assert conn.CTL_DTYPE.itemsize == 16
    assert_header_defines(("RNS_TCP_CLOSED", "RNS_TCP_ESTABLISHED", "RNS_TCP_SYN_RECEIVED", "RNS_TCP_CLOSE_WAIT", "RNS_TCP_LAST_ACK",
                           "RNS_TCP_FIN_WAIT1", "RNS_TCP_FIN_WAIT2", "RNS_TCP_CLOSING", "RNS_TCP_TIME_WAIT", "RNS_TCP_SYN_SENT",
                           "RNS_TCP_LISTEN", "RNS_CTL_CONSUMED", "RNS_CTL_SEND", "RNS_CTL_ACK_TIMER", "RNS_CTL_RESP_TIMER",
                           "RNS_CTL_TIMEWAIT", "RNS_CTL_RESET", "RNS_CTL_STATE", "RNS_EV_STATE", "RNS_STOP_TWICE"))
    assert_header_compiles("_Static_assert(sizeof(rns_tcp_ctl) == 16 && RNS_CTL_CONSUMED == RNS_SEG_CONSUMED && "
                           "RNS_CTL_SEND == RNS_SEG_ACK && RNS_CTL_ACK_TIMER == RNS_SEG_TIMER, \"\");\n"
                           "int main(void){ return 0; }\n")


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
    assert update(lib, n=0, meta=None, ctl=None, flow_in=None) == _lib.RNS_E_INVALID   # flows still get their records
    assert update(lib, nfl=0, meta=None) == _lib.RNS_E_INVALID


def test_build_argument_checks_come_before_the_device():
    lib = _lib.load()
    for name in BLD:
        if name != "add":                                                        # optional
            assert build(lib, **{name: None}) == _lib.RNS_E_INVALID, name
    for name in ("ctl", "add", "out", "src", "count", "work"):
        assert build(lib, **{name: ODD}) == _lib.RNS_E_INVALID, name
    assert build(lib, stride=0) == _lib.RNS_E_INVALID
    assert build(lib, work_bytes=need_build(lib, 3) - 1) == _lib.RNS_E_INVALID
    assert build(lib, n=_lib.RNS_CHAIN_MAX_PACKETS + 1) == _lib.RNS_E_INVALID
    assert build(lib, n=0, count=None) == _lib.RNS_E_INVALID                     # the counts are always written


def test_close_argument_checks_come_before_the_device():
    lib = _lib.load()
    assert close(lib, nfl=0, **{k: None for k in CLS}) == _lib.RNS_OK
    for name in CLS:
        assert close(lib, **{name: None}) == _lib.RNS_E_INVALID, name
    for name in ("flow_in", "flow_out", "ctl"):
        assert close(lib, **{name: ODD}) == _lib.RNS_E_INVALID, name
    assert close(lib, nfl=2 ** 31) == _lib.RNS_E_INVALID


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert update(lib) == _lib.RNS_E_NODEVICE
    assert update(lib, work_bytes=need(lib, 3, 2)) == _lib.RNS_E_NODEVICE
    assert update(lib, cap=0, pend_in=None, pend_out=None) == _lib.RNS_E_NODEVICE   # no pending lists wanted
    assert update(lib, n=0, meta=None, ctl=None) == _lib.RNS_E_NODEVICE
    assert update(lib, nfl=0, flow_in=None, flow_out=None, res=None, pend_in=None, pend_out=None) == _lib.RNS_E_NODEVICE
    assert build(lib) == _lib.RNS_E_NODEVICE
    assert build(lib, add=None) == _lib.RNS_E_NODEVICE
    assert build(lib, cap=0, out=None, src=None, len8=None) == _lib.RNS_E_NODEVICE   # counting only
    assert build(lib, nfl=0, tmpl=None, hl8=None, stride=0) == _lib.RNS_E_NODEVICE
    assert build(lib, n=0, ctl=None, work=None, work_bytes=0) == _lib.RNS_E_NODEVICE
    assert build(lib, work_bytes=need_build(lib, 3)) == _lib.RNS_E_NODEVICE
    assert build(lib, work_bytes=need(lib, 3, 0)) == _lib.RNS_E_NODEVICE         # the update's workspace serves
    assert close(lib) == _lib.RNS_E_NODEVICE
    assert close(lib, flow_out=FAKE, flow_in=FAKE) == _lib.RNS_E_NODEVICE        # in place


def test_workspace_helpers_are_monotone():
    lib = _lib.load()
    ns = (0, 1, 255, 256, 257, 70000, 1 << 20, 1 << 23, _lib.RNS_CHAIN_MAX_PACKETS)
    fs = (0, 1, 255, 256, 257, 70000, 1 << 20, 2 ** 31 - 1)
    grid = [[need(lib, n, f) for f in fs] for n in ns]
    for i in range(len(ns)):
        assert need_build(lib, ns[i]) > 0 and (i == 0 or need_build(lib, ns[i]) >= need_build(lib, ns[i - 1]))
        for j in range(len(fs)):
            assert grid[i][j] >= 4 * (ns[i] + 2 * fs[j])            # the lists and two dwords per flow at least
            assert grid[i][j] >= need_build(lib, ns[i])             # ... and it serves the build over its records
            assert i == 0 or grid[i][j] >= grid[i - 1][j]
            assert j == 0 or grid[i][j] >= grid[i][j - 1]
    assert conn.conn_work(1 << 20, 1024) == need(lib, 1 << 20, 1024) == flow.flow_update_work(1 << 20, 1024)
    b = ctypes.c_uint64(0)
    assert lib.rns_rx_tcp_conn_update_work(1, 1, None) == _lib.RNS_E_INVALID
    assert lib.rns_rx_tcp_conn_update_work(_lib.RNS_CHAIN_MAX_PACKETS + 1, 1, ctypes.byref(b)) == _lib.RNS_E_INVALID
    assert lib.rns_rx_tcp_conn_update_work(1, 2 ** 31, ctypes.byref(b)) == _lib.RNS_E_INVALID
    assert lib.rns_tx_tcp_ctl_build_work(1, None) == _lib.RNS_E_INVALID
    assert lib.rns_tx_tcp_ctl_build_work(_lib.RNS_CHAIN_MAX_PACKETS + 1, ctypes.byref(b)) == _lib.RNS_E_INVALID


def test_python_wrappers_refuse_cpu_tensors():
    import torch

    from rustnetworkstack_amd import batch
    z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="no CPU fallback"):
        batch.rx_tcp_conn_update(z(48), z(40), None, pend_cap=0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        batch.tx_tcp_ctl_build(z(32), 1, z((1, 64)), z(1), 0, out_cap=4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        batch.tx_tcp_close(z(40), z(1))
    assert batch.CTL_DTYPE is conn.CTL_DTYPE and batch.tcp_conn is conn.tcp_conn and batch.conn_update_host is conn.conn_update_host
