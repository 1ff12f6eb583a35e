"""Receive verify over pool buffers (rns_rx_verify_pool_dev) without a GPU: the three symbols, the
argument checks (all before the device is touched), the GPU-less error, and the host layout helper
(rns_rx_pool_layout) against a numpy cumsum."""
import ctypes

import numpy as np
import pytest

from abi_helper import FAKE
from rustnetworkstack_amd import _lib, batch
from rustnetworkstack_amd.workloads import rx_chain_layout

L4 = bytes([10, 0, 0, 2])
L6 = bytes(range(16))


def call(lib, pool=FAKE, log2=9, idx=FAKE, n_frags=1, blk=FAKE, len16=FAKE, n=1, l4=L4, l6=L6, status=FAKE,
         l4_sum=None):
    return lib.rns_rx_verify_pool_dev(pool, 4096, log2, idx, n_frags, blk, len16, n, l4, l6, status, l4_sum, None)


def test_symbols_are_bound_and_declared():
    lib = _lib.load()
    for name, argc in (("rns_rx_verify_pool_dev", 13), ("rns_rx_pool_layout", 6), ("rns_io_recv_batch_pool", 11)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    for name in ("rx_pool_layout", "rx_verify_pool", "recv_batch_pool"):
        assert callable(getattr(batch, name))


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    assert call(lib, n=0) == _lib.RNS_OK
    assert lib.rns_rx_verify_pool_dev(None, 0, 0, None, 0, None, None, 0, None, None, None, None, None) == _lib.RNS_OK
    for kw in ({"log2": 5}, {"log2": 16}, {"log2": 0}, {"pool": None}, {"blk": None}, {"len16": None},
               {"status": None}, {"l4": None}, {"l6": None}, {"idx": None}, {"n": _lib.RNS_CHAIN_MAX_PACKETS + 1},
               {"pool": ctypes.c_void_p(4096 + 8)}, {"pool": ctypes.c_void_p(4096 + 1)}):
        assert call(lib, **kw) == _lib.RNS_E_INVALID, kw


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    assert call(lib, idx=None, n_frags=0) == _lib.RNS_E_NODEVICE  # no fragments: the index array may be NULL
    for log2 in (6, 15):
        assert call(lib, log2=log2) == _lib.RNS_E_NODEVICE
    assert call(lib, n=_lib.RNS_CHAIN_MAX_PACKETS, l4_sum=FAKE, pool=ctypes.c_void_p(4096 + 16)) == _lib.RNS_E_NODEVICE


def lengths(n, buf):
    edge = [0, buf - 1, buf, buf + 1, 65535, 1] + [x for x in (2 * buf, 2 * buf + 1) if x <= 65535]
    w = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(48)
    ln = w.astype(np.uint16)
    k = min(n, len(edge))
    ln[:k] = np.array(edge[:k], dtype=np.uint16)
    return np.roll(ln, n // 3) if n else ln


@pytest.mark.parametrize("log2", [6, 9, 11, 15])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 200])
def test_layout_against_numpy(n, log2):
    lib = _lib.load()
    buf = 1 << log2
    ln = lengths(n, buf)
    nfr = -(-ln.astype(np.int64) // buf)
    want = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nfr, out=want[1:])
    nb = (n + 63) // 64
    blk = np.full(nb + 1, 0xDEAD, dtype=np.uint32)
    first = np.full(n + 2, 0xDEAD, dtype=np.uint32)
    nf = ctypes.c_uint64(77)
    assert lib.rns_rx_pool_layout(ln.ctypes.data, n, log2, blk.ctypes.data, first.ctypes.data,
                                  ctypes.byref(nf)) == _lib.RNS_OK
    assert nf.value == want[-1]
    assert np.array_equal(first[:n + 1], want) and first[n + 1] == 0xDEAD
    assert np.array_equal(blk[:nb], want[:-1:64]) and blk[nb] == 0xDEAD
    nf2 = ctypes.c_uint64(0)                                        # first is optional
    blk2 = np.zeros(max(nb, 1), dtype=np.uint32)
    assert lib.rns_rx_pool_layout(ln.ctypes.data, n, log2, blk2.ctypes.data, None, ctypes.byref(nf2)) == _lib.RNS_OK
    assert nf2.value == want[-1] and np.array_equal(blk2[:nb], blk[:nb])
    b3, f3, n3 = batch.rx_pool_layout(ln, buf)                      # the Python wrapper
    assert n3 == want[-1] and np.array_equal(f3, want) and np.array_equal(b3, want[:-1:64])


def test_layout_rejects():
    lib = _lib.load()
    ln = np.full(4, 100, dtype=np.uint16)
    blk = np.zeros(1, dtype=np.uint32)
    nf = ctypes.c_uint64(0)
    ok = (ln.ctypes.data, 4)
    assert lib.rns_rx_pool_layout(*ok, 5, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    assert lib.rns_rx_pool_layout(*ok, 16, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    assert lib.rns_rx_pool_layout(*ok, 9, None, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    assert lib.rns_rx_pool_layout(None, 4, 9, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    assert lib.rns_rx_pool_layout(*ok, 9, blk.ctypes.data, None, None) == _lib.RNS_E_INVALID
    assert lib.rns_rx_pool_layout(None, 0, 9, None, None, ctypes.byref(nf)) == _lib.RNS_OK and nf.value == 0
    with pytest.raises(ValueError):
        batch.rx_pool_layout([70000], 512)
    with pytest.raises(ValueError):
        batch.rx_pool_layout([100], 500)


def test_layout_reports_a_fragment_total_past_32_bits():
    """65535-byte datagrams in 64-byte buffers take 1024 each: 2^22 of them are 2^32 fragments."""
    lib = _lib.load()
    n = 1 << 22
    ln = np.full(n, 65535, dtype=np.uint16)
    blk = np.zeros(n // 64, dtype=np.uint32)
    nf = ctypes.c_uint64(0)
    assert lib.rns_rx_pool_layout(ln.ctypes.data, n, 6, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    ln[-1] = 65535 - 64                                              # one fragment fewer: 2^32 - 1 fits
    assert lib.rns_rx_pool_layout(ln.ctypes.data, n, 6, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_OK
    assert nf.value == 2 ** 32 - 1 and blk[-1] == (n - 64) * 1024


@pytest.mark.parametrize("config,n", [("c3_1500B", 300), ("c5_imix", 3000)])
def test_layout_matches_the_workload(config, n):
    """The compact descriptors RxChainBatch uploads are those the helper gives for its lengths."""
    lay = rx_chain_layout(config, n=n)
    blk, first, nf = batch.rx_pool_layout(lay.flat.length, lay.buf_bytes)
    assert nf == lay.n_frags and np.array_equal(first, lay.first) and np.array_equal(blk, lay.first[:-1:64])
