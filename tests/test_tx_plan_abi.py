"""TCP send planning (rns_tx_tcp_plan_dev) without a GPU: the symbols, the constants and the record size,
every argument check (all before the device is touched), the GPU-less error, the workspace helper and
the CPU-tensor refusal."""
import ctypes

import pytest

from abi_helper import BIG, FAKE, assert_header_compiles, assert_header_defines
from rustnetworkstack_amd import _lib, batch, send

# name -> required alignment (0: bytes); the optional ones are not in REQUIRED
ALIGN = {"flow_in": 4, "flow_out": 4, "sq_off": 8, "sq_seq": 4, "sq_len": 4, "mss": 2, "rexmit": 0, "tmpl": 0, "hl8": 0,
         "id_add": 4, "tmpl_out": 0, "hl8_out": 0, "pay_off": 8, "pay_len": 4, "mss_out": 2, "head_off": 8, "seg_first": 4,
         "blk_flow": 4, "n": 4, "res": 4, "work": 8}
OPTIONAL = ("rexmit", "id_add")


def plan(lib, nfl=3, stride=64, cap=100, work_bytes=BIG, **kw):
    p = {k: kw.get(k, FAKE) for k in ALIGN}
    return lib.rns_tx_tcp_plan_dev(p["flow_in"], p["flow_out"], nfl, p["sq_off"], p["sq_seq"], p["sq_len"], p["mss"], p["rexmit"],
                                   p["tmpl"], stride, p["hl8"], 0xFFFE, p["id_add"], 1 << 33, cap, p["tmpl_out"], p["hl8_out"],
                                   p["pay_off"], p["pay_len"], p["mss_out"], p["head_off"], p["seg_first"], p["blk_flow"],
                                   p["n"], p["res"], p["work"], work_bytes, None)


def need(lib, nfl):
    b = ctypes.c_uint64(0)
    assert lib.rns_tx_tcp_plan_work(nfl, ctypes.byref(b)) == _lib.RNS_OK
    return b.value


def test_symbols_constants_and_sizes():
    lib = _lib.load()
    for name, argc in (("rns_tx_tcp_plan_dev", 28), ("rns_tx_tcp_plan_work", 2)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    assert send.RES_DTYPE.itemsize == 16 and batch.PLAN_RES_DTYPE is send.RES_DTYPE
    assert batch.tx_tcp_plan is send.tx_tcp_plan and batch.plan_host is send.plan_host
    assert batch.tx_tcp_send is send.tx_tcp_send and batch.tx_plan_work is send.tx_plan_work
    assert_header_defines(("RNS_PLAN_NONE", "RNS_PLAN_WINDOW", "RNS_PLAN_STATE", "RNS_PLAN_BAD", "RNS_PLAN_TMPL", "RNS_PLAN_CAP"))
    assert_header_compiles("_Static_assert(sizeof(rns_tx_plan_res) == 16, \"\");\nint main(void){ return 0; }\n")


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    for name, al in ALIGN.items():
        if name not in OPTIONAL:
            assert plan(lib, **{name: None}) == _lib.RNS_E_INVALID, name
        for k in (1, 2, 4):
            if k < al:
                assert plan(lib, **{name: ctypes.c_void_p(4096 + k)}) == _lib.RNS_E_INVALID, (name, k)
    assert plan(lib, nfl=2 ** 30 + 1) == _lib.RNS_E_INVALID
    assert plan(lib, cap=_lib.RNS_CHAIN_MAX_PACKETS + 1) == _lib.RNS_E_INVALID
    assert plan(lib, stride=0) == _lib.RNS_E_INVALID
    assert plan(lib, work_bytes=need(lib, 3) - 1) == _lib.RNS_E_INVALID
    assert plan(lib, work_bytes=0) == _lib.RNS_E_INVALID
    # no flows: the counts, the index's one entry and the block array are still written
    assert plan(lib, nfl=0, seg_first=None) == _lib.RNS_E_INVALID
    assert plan(lib, nfl=0, n=None) == _lib.RNS_E_INVALID
    assert plan(lib, nfl=0, blk_flow=None) == _lib.RNS_E_INVALID


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert plan(lib) == _lib.RNS_E_NODEVICE
    assert plan(lib, work_bytes=need(lib, 3)) == _lib.RNS_E_NODEVICE
    assert plan(lib, rexmit=None, id_add=None) == _lib.RNS_E_NODEVICE
    assert plan(lib, nfl=2 ** 30, cap=_lib.RNS_CHAIN_MAX_PACKETS) == _lib.RNS_E_NODEVICE
    assert plan(lib, cap=0, blk_flow=None) == _lib.RNS_E_NODEVICE
    assert plan(lib, mss=ctypes.c_void_p(4096 + 2), mss_out=ctypes.c_void_p(4096 + 6)) == _lib.RNS_E_NODEVICE
    keep = ("seg_first", "blk_flow", "n")
    assert plan(lib, nfl=0, work_bytes=0, **{k: None for k in ALIGN if k not in keep}) == _lib.RNS_E_NODEVICE


def test_workspace_helper_is_monotone():
    lib = _lib.load()
    fs = (0, 1, 127, 128, 129, 255, 256, 257, 33000, 1 << 20, 2 ** 30)
    got = [need(lib, f) for f in fs]
    assert all(b >= a for a, b in zip(got, got[1:])) and all(g >= 16 * f and g % 8 == 0 for g, f in zip(got, fs))
    assert send.tx_plan_work(33000) == need(lib, 33000)
    b = ctypes.c_uint64(0)
    assert lib.rns_tx_tcp_plan_work(1, None) == _lib.RNS_E_INVALID
    assert lib.rns_tx_tcp_plan_work(2 ** 30 + 1, ctypes.byref(b)) == _lib.RNS_E_INVALID


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt)  # noqa: E731
    args = (z(80), z(2, torch.int64), z(2, torch.int32), z(2, torch.int32), z(2, torch.uint16), z((2, 64)), z(2))
    with pytest.raises(ValueError, match="no CPU fallback"):
        send.tx_tcp_plan(*args, head_first_off=0, seg_cap=8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        send.tx_tcp_send(z(4096), *args, head_first_off=0, seg_cap=8)
    with pytest.raises(TypeError):
        send.plan_host(z(80).numpy(), *[a.numpy() for a in args[1:]], head_first_off=0, seg_cap=8)
