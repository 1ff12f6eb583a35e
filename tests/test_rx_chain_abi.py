"""Receive verify over fragment chains (rns_rx_verify_chain_dev) without a GPU: the symbol, its
argument checks (all before the device is touched), the GPU-less error, and the host layout of
the receive-chain workload (workloads.rx_chain_layout)."""
import ctypes

import numpy as np
import pytest

from abi_helper import FAKE
from rustnetworkstack_amd import _lib
from rustnetworkstack_amd.workloads import make_layout, rx_chain_layout

L4 = bytes([10, 0, 0, 2])
L6 = bytes(range(16))


def call(lib, arena=FAKE, off=FAKE, ln=FAKE, n_frags=1, first=FAKE, n=1, l4=L4, l6=L6, status=FAKE, l4_sum=None):
    return lib.rns_rx_verify_chain_dev(arena, 4096, off, ln, n_frags, first, n, l4, l6, status, l4_sum, None)


def test_symbol_is_bound_and_declared():
    lib = _lib.load()
    assert "rns_rx_verify_chain_dev" in _lib.EXPORTED_SYMBOLS
    assert "rns_io_recv_batch_chain" in _lib.EXPORTED_SYMBOLS
    assert len(lib.rns_rx_verify_chain_dev.argtypes) == 12
    assert len(lib.rns_io_recv_batch_chain.argtypes) == 12
    assert lib.rns_abi_version() == 1  # additive: the ABI version stays


def test_argument_checks_come_before_the_device():
    lib = _lib.load()
    assert call(lib, n=0) == _lib.RNS_OK
    assert lib.rns_rx_verify_chain_dev(None, 0, None, None, 0, None, 0, None, None, None, None, None) == _lib.RNS_OK
    for kw in ({"arena": None}, {"first": None}, {"status": None}, {"l4": None}, {"l6": None}, {"off": None},
               {"ln": None}, {"n": _lib.RNS_CHAIN_MAX_PACKETS + 1}):
        assert call(lib, **kw) == _lib.RNS_E_INVALID, kw


@pytest.mark.skipif(_lib.load().rns_device_count() > 0, reason="checks the GPU-less behaviour")
def test_valid_arguments_fail_loudly_without_gpu():
    lib = _lib.load()
    assert call(lib) == _lib.RNS_E_NODEVICE
    assert call(lib, off=None, ln=None, n_frags=0) == _lib.RNS_E_NODEVICE  # no fragments: the arrays may be NULL
    assert call(lib, n=_lib.RNS_CHAIN_MAX_PACKETS, l4_sum=FAKE) == _lib.RNS_E_NODEVICE


@pytest.mark.parametrize("config,n", [("c3_1500B", 300), ("c5_imix", 3000)])
@pytest.mark.parametrize("shuffled", [False, True])
def test_workload_layout(config, n, shuffled):
    """Every datagram in ceil(L / 512) buffers, full but the last; the buffers a permutation of
    the pool; in order they are the padded flat arena's rows."""
    lay = rx_chain_layout(config, n=n, shuffled=shuffled)
    L = make_layout(config, n=n).length.astype(np.int64)
    first = lay.first.astype(np.int64)
    assert np.array_equal(np.diff(first), (L + 511) // 512)
    assert np.array_equal(np.add.reduceat(lay.frag_len.astype(np.int64), first[:-1]), L)
    last = np.zeros(lay.n_frags, dtype=bool)
    last[first[1:] - 1] = True
    assert (lay.frag_len[~last] == 512).all() and (lay.frag_len[last] >= 1).all() and (lay.frag_len <= 512).all()
    assert np.array_equal(np.sort(lay.buf), np.arange(lay.n_frags))
    assert np.array_equal(lay.frag_off, (lay.buf * 512).astype(np.uint64))
    assert lay.flat.arena_bytes == 512 * lay.n_frags
    assert np.array_equal(lay.flat.off, (first[:-1] * 512).astype(np.uint64))
    assert shuffled == (not np.array_equal(lay.buf, np.arange(lay.n_frags)))
