"""The compact-descriptor chain finalize (rns_tx_fill_chain_packed_dev) without a GPU: the symbol
and its argument checks, the host layout helper (rns_tx_chain_packed_layout) against a numpy
cumsum, and the route TxChainPipeline(compact=True) chooses for a batch."""
import ctypes

import numpy as np
import pytest

from abi_helper import FAKE
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.batch import tx_chain_packed_layout
from rustnetworkstack_amd.pipeline import chain_compact_form, compact_desc_bytes



def call(lib, arena=FAKE, hblk=FAKE, hl=FAKE, pblk=FAKE, pl=FAKE, align=4, n=1):
    return lib.rns_tx_fill_chain_packed_dev(arena, 4096, hblk, hl, pblk, pl, align, n, None, None)


def test_symbol_is_bound_and_declared():
    lib = _lib.load()
    assert "rns_tx_fill_chain_packed_dev" in _lib.EXPORTED_SYMBOLS
    assert "rns_tx_chain_packed_layout" in _lib.EXPORTED_SYMBOLS
    assert lib.rns_tx_fill_chain_packed_dev.argtypes is not None
    assert len(lib.rns_tx_fill_chain_packed_dev.argtypes) == 10
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    assert call(lib, n=0) == _lib.RNS_OK
    assert lib.rns_tx_fill_chain_packed_dev(None, 0, None, None, None, None, 99, 0, None, None) == _lib.RNS_OK
    for kw in ({"arena": None}, {"hblk": None}, {"hl": None}, {"pblk": None}, {"pl": None}, {"align": 3},
               {"align": 13}, {"n": _lib.RNS_CHAIN_MAX_PACKETS + 1}):
        assert call(lib, **kw) == _lib.RNS_E_INVALID, kw


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    assert call(lib, align=12, n=_lib.RNS_CHAIN_MAX_PACKETS) == _lib.RNS_E_NODEVICE


def lengths(n, seed):
    rng = np.random.default_rng(seed)
    hl = rng.integers(0, 256, n).astype(np.uint8)
    pl = rng.integers(0, 65536, n).astype(np.uint16)
    pl[rng.random(n) < 0.3] = 0          # head-only datagrams
    if n > 2:
        pl[1] = 1
        pl[2] = 65535
    return hl, pl


def numpy_layout(hl, pl, align_log2, h0, p0):
    m = (1 << align_log2) - 1
    h, pad = hl.astype(np.uint64), (pl.astype(np.uint64) + np.uint64(m)) & ~np.uint64(m)
    hoff = np.uint64(h0) + np.concatenate([[0], np.cumsum(h)[:-1]]).astype(np.uint64) if hl.size else h
    poff = np.uint64(p0) + np.concatenate([[0], np.cumsum(pad)[:-1]]).astype(np.uint64) if hl.size else pad
    return hoff, poff, h0 + int(h.sum()), p0 + int(pad.sum())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200])
@pytest.mark.parametrize("align_log2,h0,p0", [(4, 0, 0), (11, 0, 0), (4, 3, 4096 + 16), (11, 12345, 1 << 33), (4, 7, 8)])
def test_layout_helper_matches_cumsum(n, align_log2, h0, p0):
    hl, pl = lengths(n, 100 + n)
    hoff, poff, hend, pend = numpy_layout(hl, pl, align_log2, h0, p0)
    hblk, pblk, ho, po, he, pe = tx_chain_packed_layout(hl, pl, align_log2, h0, p0)
    assert hblk.shape == pblk.shape == ((n + 63) // 64,)
    assert np.array_equal(ho, hoff) and np.array_equal(po, poff)
    assert np.array_equal(hblk, hoff[::64]) and np.array_equal(pblk, poff[::64])
    assert (he, pe) == (hend, pend)
    # a zero-length payload occupies nothing: the next payload starts where it does
    z = np.flatnonzero(pl[:-1] == 0)
    assert np.array_equal(po[z], po[z + 1])
    # the optional outputs as NULL, straight through the C ABI
    lib = _lib.load()
    nb = max((n + 63) // 64, 1)
    hb2, pb2 = np.zeros(nb, np.uint64), np.zeros(nb, np.uint64)
    e1, e2 = ctypes.c_uint64(), ctypes.c_uint64()
    st = lib.rns_tx_chain_packed_layout(hl.ctypes.data, pl.ctypes.data, n, align_log2, h0, p0, hb2.ctypes.data,
                                        pb2.ctypes.data, None, None, ctypes.byref(e1), ctypes.byref(e2))
    assert st == _lib.RNS_OK and (e1.value, e2.value) == (hend, pend)
    assert np.array_equal(hb2[:(n + 63) // 64], hblk) and np.array_equal(pb2[:(n + 63) // 64], pblk)


def test_layout_helper_rejects():
    lib = _lib.load()
    hl, pl = lengths(10, 1)
    blk = np.zeros(1, np.uint64)
    e = ctypes.c_uint64()
    args = (hl.ctypes.data, pl.ctypes.data, 10)
    assert lib.rns_tx_chain_packed_layout(*args, 3, 0, 0, blk.ctypes.data, blk.ctypes.data, None, None,
                                          ctypes.byref(e), ctypes.byref(e)) == _lib.RNS_E_INVALID
    assert lib.rns_tx_chain_packed_layout(*args, 13, 0, 0, blk.ctypes.data, blk.ctypes.data, None, None,
                                          ctypes.byref(e), ctypes.byref(e)) == _lib.RNS_E_INVALID
    assert lib.rns_tx_chain_packed_layout(*args, 4, 0, 0, None, blk.ctypes.data, None, None, ctypes.byref(e),
                                          ctypes.byref(e)) == _lib.RNS_E_INVALID
    assert lib.rns_tx_chain_packed_layout(*args, 4, 0, 0, blk.ctypes.data, blk.ctypes.data, None, None, None,
                                          ctypes.byref(e)) == _lib.RNS_E_INVALID
    with pytest.raises(ValueError):
        tx_chain_packed_layout([256], [10])
    with pytest.raises(ValueError):
        tx_chain_packed_layout([40], [65536])
    with pytest.raises(ValueError):
        tx_chain_packed_layout([40, 40], [10])
    with pytest.raises(ValueError):
        tx_chain_packed_layout([40], [10], 3)


def packed_batch(n, seed):
    rng = np.random.default_rng(seed)
    hl = rng.integers(1, 129, n)
    pl = rng.integers(0, 1461, n)
    pl[rng.random(n) < 0.25] = 0
    pad = (pl + 15) & ~15
    po = np.cumsum(pad) - pad
    return hl, po, pl


def test_pipeline_route_choice():
    """What TxChainPipeline(compact=True) decides per batch (chain_compact_form, no device): a
    packed batch yields the helper's compact descriptors, 3 B per datagram + 16 B per 64; a
    displaced payload offset, an unaligned first offset or a length the form cannot hold
    yields the CSR route."""
    head_region = 128 * 4096
    n = 500
    hl, po, pl = packed_batch(n, 7)
    c = chain_compact_form(hl, po, pl, head_region)
    assert c is not None
    hblk, hl8, pblk, pl16 = c
    w_hblk, w_pblk, _, w_po, _, _ = tx_chain_packed_layout(hl, pl, 4, 0, head_region)
    assert np.array_equal(hblk, w_hblk) and np.array_equal(pblk, w_pblk)
    assert np.array_equal(w_po[pl > 0], (po + head_region)[pl > 0])
    assert hl8.dtype == np.uint8 and pl16.dtype == np.uint16
    assert np.array_equal(hl8, hl) and np.array_equal(pl16, pl)
    assert hblk.nbytes + hl8.nbytes + pblk.nbytes + pl16.nbytes == 3 * n + 16 * 8 == compact_desc_bytes(n)
    # a packed region that starts later (16-aligned) is still the compact form
    c2 = chain_compact_form(hl, po + 4096, pl, head_region)
    assert c2 is not None and np.array_equal(c2[2], w_pblk + np.uint64(4096))
    # the offset of a head-only datagram means nothing
    po3 = po.copy()
    po3[np.flatnonzero(pl == 0)[0]] = 12345
    assert chain_compact_form(hl, po3, pl, head_region) is not None
    # one displaced payload, an unaligned start, oversize lengths: the CSR route
    k = np.flatnonzero(pl > 0)[100]
    for d in (16, -16, 1):
        po4 = po.copy()
        po4[k] += d
        assert chain_compact_form(hl, po4, pl, head_region) is None
    assert chain_compact_form(hl, po + 8, pl, head_region) is None
    assert chain_compact_form(hl, po, pl, head_region + 8) is None
    hl5 = hl.copy()
    hl5[3] = 256
    assert chain_compact_form(hl5, po, pl, head_region) is None
    pl6 = pl.copy()
    pl6[-1] = 65536
    assert chain_compact_form(hl, po, pl6, head_region) is None
    assert chain_compact_form([], [], [], head_region) is None


@pytest.mark.parametrize("config,n", [("c3_1500B", 200), ("c5_imix", 5000)])
def test_workload_layout_compact_descriptors(config, n):
    """workloads.tx_chain_compact: the compact descriptors of a tx_chain_layout (one payload
    fragment) imply exactly the layout's own fragment offsets; fragmented payloads are refused."""
    from rustnetworkstack_amd.workloads import tx_chain_compact, tx_chain_layout
    lay = tx_chain_layout(config, n=n, head=40, frag=0)
    hblk, hl8, pblk, pl16 = tx_chain_compact(lay)
    first = lay.first.astype(np.int64)
    assert np.array_equal(hl8, lay.frag_len[first[:-1]])
    total = np.add.reduceat(lay.frag_len.astype(np.int64), first[:-1])
    assert np.array_equal(pl16.astype(np.int64), total - hl8)
    hoff, poff, _, _ = numpy_layout(hl8, pl16, 4, int(hblk[0]), int(pblk[0]))
    assert np.array_equal(hblk, hoff[::64]) and np.array_equal(pblk, poff[::64])
    has = pl16 > 0
    assert np.array_equal(hoff, lay.frag_off[first[:-1]])
    assert np.array_equal(poff[has], lay.frag_off[first[:-1][has] + 1])
    assert hblk.nbytes + pblk.nbytes + hl8.nbytes + pl16.nbytes == compact_desc_bytes(n)
    with pytest.raises(ValueError):
        tx_chain_compact(tx_chain_layout(config, n=n, head=40, frag=512))
