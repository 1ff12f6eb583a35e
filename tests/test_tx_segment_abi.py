"""TCP segmentation offload (rns_tx_segment_dev) without a GPU: the symbols, the argument checks (all
before the device is touched), the GPU-less error, the CPU-tensor refusal and the two host helpers
(rns_tx_segment_layout, rns_tx_segment_chains) against the numpy expansion of tx_segment_helper."""
import ctypes

import numpy as np
import pytest

from abi_helper import FAKE
from rustnetworkstack_amd import _lib, batch
from tx_segment_helper import Flow, chains, data_bytes, lay, template

ARGS = ("arena", "tmpl", "hl", "po", "pl", "mss", "ho", "sf", "bf")


def call(lib, stride=40, n_flows=1, n_seg=1, status=None, **kw):
    p = {k: kw.get(k, FAKE) for k in ARGS}
    return lib.rns_tx_segment_dev(p["arena"], 4096, p["tmpl"], stride, p["hl"], p["po"], p["pl"], p["mss"], p["ho"],
                                  p["sf"], p["bf"], n_flows, n_seg, status, None)


def test_symbols_are_bound_and_declared():
    lib = _lib.load()
    for name, argc in (("rns_tx_segment_dev", 15), ("rns_tx_segment_layout", 10), ("rns_tx_segment_chains", 10)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    for name in ("tx_segment", "tx_segment_layout", "tx_segment_chains"):
        assert callable(getattr(batch, name))


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    assert call(lib, n_flows=0) == _lib.RNS_OK
    assert call(lib, n_seg=0) == _lib.RNS_OK
    assert lib.rns_tx_segment_dev(None, 0, None, 0, None, None, None, None, None, None, None, 0, 0, None, None) == _lib.RNS_OK
    for name in ARGS:
        assert call(lib, **{name: None}) == _lib.RNS_E_INVALID, name
    assert call(lib, stride=0) == _lib.RNS_E_INVALID
    assert call(lib, n_seg=_lib.RNS_CHAIN_MAX_PACKETS + 1) == _lib.RNS_E_INVALID


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    assert call(lib, status=FAKE, n_seg=_lib.RNS_CHAIN_MAX_PACKETS) == _lib.RNS_E_NODEVICE


def test_python_wrapper_refuses_cpu_tensors():
    import torch
    z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="no CPU fallback"):
        batch.tx_segment(z(1024, torch.uint8), z(40, torch.uint8), z(1, torch.uint8), z(1, torch.int64), z(1, torch.int32),
                         z(1, torch.int16), z(1, torch.int64), z(2, torch.int32), z(1, torch.int32), 1)


def flows_for(kind):
    t40, t52, t60 = template(), template(opts=12), template(v6=True)
    if kind == "zero_length_between":
        spec = [(t40, 0, 100), (t40, 3000, 1460), (t52, 0, 0), (t60, 0, 7), (t40, 1, 1460), (t40, 0, 1)]
    elif kind == "mss1":
        spec = [(t40, 70, 1), (t60, 130, 1), (t40, 1, 1)]
    elif kind == "65_flows_in_one_block":
        spec = [(t40, 1, 1460)] * 63 + [(t40, 0, 5)] * 3 + [(t52, 10, 10), (t40, 2921, 1460)]
    else:  # block edges: flows ending at 63, 64, 65, 128 and one spanning three blocks
        spec = [(t40, 63, 1), (t40, 1, 9), (t52, 1, 9), (t40, 63 * 7, 7), (t60, 200 * 3 - 1, 3)]
    return [Flow(t, data_bytes(i + 1, n), mss) for i, (t, n, mss) in enumerate(spec)]


@pytest.mark.parametrize("kind", ["zero_length_between", "mss1", "65_flows_in_one_block", "block_edges"])
def test_layout_helpers_against_numpy(kind):
    lib = _lib.load()
    flows = flows_for(kind)
    L = lay(flows, head_align=5)
    nfl = len(flows)
    hfirst = int(L.ho[0])
    seg_first = np.full(nfl + 2, 0xDEAD, dtype=np.uint32)
    head_off = np.full(nfl + 1, 0xDEAD, dtype=np.uint64)
    n_seg, head_end = ctypes.c_uint64(77), ctypes.c_uint64(77)
    args = (L.pl.ctypes.data, L.mss.ctypes.data, L.hl.ctypes.data, nfl, hfirst, seg_first.ctypes.data, head_off.ctypes.data)
    assert lib.rns_tx_segment_layout(*args, None, ctypes.byref(n_seg), ctypes.byref(head_end)) == _lib.RNS_OK
    assert n_seg.value == L.n_seg and head_end.value == L.head_end
    assert np.array_equal(seg_first[:nfl + 1], L.seg_first) and seg_first[nfl + 1] == 0xDEAD
    assert np.array_equal(head_off[:nfl], L.ho) and head_off[nfl] == 0xDEAD
    nb = (L.n_seg + 63) // 64
    blk = np.full(nb + 1, 0xDEAD, dtype=np.uint32)
    assert lib.rns_tx_segment_layout(*args, blk.ctypes.data, ctypes.byref(n_seg), ctypes.byref(head_end)) == _lib.RNS_OK
    assert np.array_equal(blk[:nb], L.blk_flow) and blk[nb] == 0xDEAD
    for b in range(nb):  # the flow that holds segment 64*b, never an empty one
        f = int(blk[b])
        assert L.seg_first[f] <= 64 * b < L.seg_first[f + 1]
    sf, ho, bf, ns, he = batch.tx_segment_layout(L.pl, L.mss, L.hl, hfirst)  # the Python wrapper
    assert (ns, he) == (L.n_seg, L.head_end)
    assert np.array_equal(sf, L.seg_first) and np.array_equal(ho, L.ho) and np.array_equal(bf, L.blk_flow)
    # the chains
    off, ln, first, _ = chains(L)
    g_off, g_ln, g_first = batch.tx_segment_chains(L.po, L.pl, L.mss, L.hl, L.ho)
    assert np.array_equal(g_off, off) and np.array_equal(g_ln, ln) and np.array_equal(g_first, first)
    frag_off = np.full(2 * L.n_seg + 1, 0xDEAD, dtype=np.uint64)
    frag_len = np.full(2 * L.n_seg + 1, 0xDEAD, dtype=np.uint32)
    cfirst = np.full(L.n_seg + 2, 0xDEAD, dtype=np.uint32)
    cargs = (L.po.ctypes.data, L.pl.ctypes.data, L.mss.ctypes.data, L.hl.ctypes.data, L.ho.ctypes.data, nfl)
    assert lib.rns_tx_segment_chains(*cargs, L.n_seg, frag_off.ctypes.data, frag_len.ctypes.data,
                                     cfirst.ctypes.data) == _lib.RNS_OK
    assert frag_off[-1] == 0xDEAD and frag_len[-1] == 0xDEAD and cfirst[-1] == 0xDEAD
    assert np.array_equal(frag_off[:-1], off) and np.array_equal(frag_len[:-1], ln) and np.array_equal(cfirst[:-1], first)
    for wrong in (L.n_seg - 1, L.n_seg + 1):  # not the flows' segment total
        assert lib.rns_tx_segment_chains(*cargs, wrong, frag_off.ctypes.data, frag_len.ctypes.data,
                                         cfirst.ctypes.data) == _lib.RNS_E_INVALID


def test_layout_rejects():
    lib = _lib.load()
    pl, mss = np.array([100, 0], dtype=np.uint32), np.array([10, 0], dtype=np.uint16)
    hl = np.array([40, 40], dtype=np.uint8)
    sf, ho = np.zeros(3, dtype=np.uint32), np.zeros(2, dtype=np.uint64)
    ns, he = ctypes.c_uint64(0), ctypes.c_uint64(0)
    out = (sf.ctypes.data, ho.ctypes.data, None, ctypes.byref(ns), ctypes.byref(he))
    assert lib.rns_tx_segment_layout(pl.ctypes.data, mss.ctypes.data, hl.ctypes.data, 2, 0, *out) == _lib.RNS_OK
    assert ns.value == 10 and sf.tolist() == [0, 10, 10]   # mss 0 with nothing to send is no error
    mss0 = np.array([0, 0], dtype=np.uint16)                 # mss 0 with data to send is
    assert lib.rns_tx_segment_layout(pl.ctypes.data, mss0.ctypes.data, hl.ctypes.data, 2, 0, *out) == _lib.RNS_E_INVALID
    big = np.array([0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)  # 2 * (2^32 - 1) one-byte segments
    one = np.array([1, 1], dtype=np.uint16)
    assert lib.rns_tx_segment_layout(big.ctypes.data, one.ctypes.data, hl.ctypes.data, 2, 0, *out) == _lib.RNS_E_INVALID
    for k in range(3):                                        # a NULL input
        a = [pl.ctypes.data, mss.ctypes.data, hl.ctypes.data]
        a[k] = None
        assert lib.rns_tx_segment_layout(*a, 2, 0, *out) == _lib.RNS_E_INVALID
    assert lib.rns_tx_segment_layout(pl.ctypes.data, mss.ctypes.data, hl.ctypes.data, 2, 0, sf.ctypes.data, ho.ctypes.data,
                                     None, None, ctypes.byref(he)) == _lib.RNS_E_INVALID
    assert lib.rns_tx_segment_layout(None, None, None, 0, 9, sf.ctypes.data, None, None, ctypes.byref(ns),
                                     ctypes.byref(he)) == _lib.RNS_OK
    assert ns.value == 0 and he.value == 9 and sf[0] == 0
    with pytest.raises(ValueError):
        batch.tx_segment_layout([100], [70000], [40])
    with pytest.raises(ValueError):
        batch.tx_segment_layout([100], [10], [256])
    with pytest.raises(ValueError):
        batch.tx_segment_layout([100, 5], [10], [40])
