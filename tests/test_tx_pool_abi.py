"""Transmit finalize over pool buffers (rns_tx_fill_pool_dev) without a GPU: the three symbols, the
argument checks (all before the device is touched), the GPU-less error, the CPU-tensor refusal and
the host layout helper (rns_tx_pool_layout) against a numpy restatement."""
import ctypes

import numpy as np
import pytest

from abi_helper import FAKE
from rustnetworkstack_amd import _lib, batch



def call(lib, pool=FAKE, log2=9, idx=FAKE, n_frags=1, blk=FAKE, hl=FAKE, pl=FAKE, n=1, status=None):
    return lib.rns_tx_fill_pool_dev(pool, 4096, log2, idx, n_frags, blk, hl, pl, n, status, None)


def test_symbols_are_bound_and_declared():
    lib = _lib.load()
    for name, argc in (("rns_tx_fill_pool_dev", 11), ("rns_tx_pool_layout", 6), ("rns_io_send_batch_pool", 8)):
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == argc
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays
    for name in ("tx_pool_layout", "tx_fill_pool", "send_batch_pool"):
        assert callable(getattr(batch, name))


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    assert call(lib, n=0) == _lib.RNS_OK
    assert lib.rns_tx_fill_pool_dev(None, 0, 0, None, 0, None, None, None, 0, None, None) == _lib.RNS_OK
    for kw in ({"log2": 7}, {"log2": 16}, {"log2": 0}, {"pool": None}, {"blk": None}, {"hl": None}, {"pl": None},
               {"idx": None}, {"n": _lib.RNS_CHAIN_MAX_PACKETS + 1}, {"pool": ctypes.c_void_p(4096 + 8)},
               {"pool": ctypes.c_void_p(4096 + 1)}):
        assert call(lib, **kw) == _lib.RNS_E_INVALID, kw


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    assert call(lib, idx=None, n_frags=0) == _lib.RNS_E_NODEVICE  # no fragments: the index array may be NULL
    for log2 in (8, 15):
        assert call(lib, log2=log2) == _lib.RNS_E_NODEVICE
    assert call(lib, n=_lib.RNS_CHAIN_MAX_PACKETS, status=FAKE, pool=ctypes.c_void_p(4096 + 16)) == _lib.RNS_E_NODEVICE


def test_python_wrapper_refuses_cpu_tensors():
    import torch
    z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="no CPU fallback"):
        batch.tx_fill_pool(z(1024, torch.uint8), z(2, torch.int32), z(1, torch.int32), z(1, torch.uint8), z(1, torch.int16))


LENGTHS = lambda buf: [0, 1, buf - 1, buf, buf + 1, 65535]  # noqa: E731


@pytest.mark.parametrize("buf", [256, 512, 32768])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_layout_against_numpy(n, buf):
    lib = _lib.load()
    log2 = buf.bit_length() - 1
    edge = LENGTHS(buf)
    pl = np.array([edge[(i * 5 + i // 6) % len(edge)] for i in range(n)], dtype=np.uint16)
    assert n < 6 or set(pl.tolist()) == set(edge)
    nfr = 1 + -(-pl.astype(np.int64) // buf)
    want = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nfr, out=want[1:])
    nb = (n + 63) // 64
    blk = np.full(nb + 1, 0xDEAD, dtype=np.uint32)
    first = np.full(n + 2, 0xDEAD, dtype=np.uint32)
    nf = ctypes.c_uint64(77)
    assert lib.rns_tx_pool_layout(pl.ctypes.data, n, log2, blk.ctypes.data, first.ctypes.data,
                                  ctypes.byref(nf)) == _lib.RNS_OK
    assert nf.value == want[-1]
    assert np.array_equal(first[:n + 1], want) and first[n + 1] == 0xDEAD
    assert np.array_equal(blk[:nb], want[:-1:64]) and blk[nb] == 0xDEAD
    nf2 = ctypes.c_uint64(0)                                        # first is optional
    blk2 = np.zeros(max(nb, 1), dtype=np.uint32)
    assert lib.rns_tx_pool_layout(pl.ctypes.data, n, log2, blk2.ctypes.data, None, ctypes.byref(nf2)) == _lib.RNS_OK
    assert nf2.value == want[-1] and np.array_equal(blk2[:nb], blk[:nb])
    b3, f3, n3 = batch.tx_pool_layout(pl, buf)                      # the Python wrapper
    assert n3 == want[-1] and np.array_equal(f3, want) and np.array_equal(b3, want[:-1:64])


def test_layout_rejects():
    lib = _lib.load()
    pl = np.full(4, 100, dtype=np.uint16)
    blk = np.zeros(1, dtype=np.uint32)
    nf = ctypes.c_uint64(0)
    ok = (pl.ctypes.data, 4)
    assert lib.rns_tx_pool_layout(*ok, 7, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    assert lib.rns_tx_pool_layout(*ok, 16, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    assert lib.rns_tx_pool_layout(*ok, 9, None, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    assert lib.rns_tx_pool_layout(None, 4, 9, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    assert lib.rns_tx_pool_layout(*ok, 9, blk.ctypes.data, None, None) == _lib.RNS_E_INVALID
    assert lib.rns_tx_pool_layout(None, 0, 9, None, None, ctypes.byref(nf)) == _lib.RNS_OK and nf.value == 0
    with pytest.raises(ValueError):
        batch.tx_pool_layout([70000], 512)
    with pytest.raises(ValueError):
        batch.tx_pool_layout([100], 128)
    with pytest.raises(ValueError):
        batch.tx_pool_layout([100], 500)


def test_layout_reports_a_fragment_total_past_32_bits():
    """65535-byte payloads in 256-byte buffers take 257 buffers each: 2^24 of them pass 2^32."""
    lib = _lib.load()
    n = 1 << 24
    pl = np.full(n, 65535, dtype=np.uint16)
    blk = np.zeros(n // 64, dtype=np.uint32)
    nf = ctypes.c_uint64(0)
    assert lib.rns_tx_pool_layout(pl.ctypes.data, n, 8, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_E_INVALID
    pl[1 << 23:] = 0                                                  # 2^23 * 257 + 2^23 buffers fit
    assert lib.rns_tx_pool_layout(pl.ctypes.data, n, 8, blk.ctypes.data, None, ctypes.byref(nf)) == _lib.RNS_OK
    assert nf.value == (1 << 23) * 258


@pytest.mark.parametrize("config,n", [("c3_1500B", 300), ("c5_imix", 3000)])
def test_layout_matches_the_descriptor_cost(config, n):
    """3 B per datagram + 4 B per buffer + 4 B per 64 datagrams: 19 B for a 1500-byte datagram in
    512-byte buffers against 52 B in CSR form (12 B per fragment + 4 B per datagram)."""
    from rustnetworkstack_amd.workloads import make_layout
    L = make_layout(config, n=n).length.astype(np.int64)
    blk, first, nf = batch.tx_pool_layout(L - 40, 512)
    assert nf == int((1 + -(-(L - 40) // 512)).sum())
    if config == "c3_1500B":
        assert nf == 4 * n and 3 + 4 * 4 == 19 and 12 * 4 + 4 == 52
