"""Plain C programs call the C ABI the way a Rust / cgo / FFI binding would (no torch, no Python in
the process): tests/c/test_*_abi.c over the one harness tests/c/abi_test.h, each checked against the
oracle (oracle/csum_oracle.c, linked into the test binaries only).  `make` builds them in-tree.
Without a GPU every program still builds its inputs, runs its restated reference and checks the
argument errors of its entry points, then exits 2 at its first device allocation."""
import os
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "rustnetworkstack_amd")
PROGRAMS = (
    ("test_batch_abi", "the batch entries, host- and device-resident, and the transmit / receive entries behind them"),
    ("test_tx_chain_packed_abi", "the compact-descriptor chain finalize"),
    ("test_rx_chain_abi", "the receive verify over fragment chains"),
    ("test_rx_pool_abi", "the receive verify over pool buffers"),
    ("test_tx_pool_abi", "the transmit finalize over pool buffers"),
    ("test_tx_segment_abi", "TCP segmentation offload"),
    ("test_rx_place_abi", "TCP receive placement"),
    ("test_rx_flow_abi", "the TCP flow update and the ACK build"),
    ("test_tx_plan_abi", "TCP send planning, then segmentation"),
    ("test_icmp_echo_abi", "the ICMP echo responder"),
)
NAMES = [name for name, _ in PROGRAMS]


def _compile(name: str, out: str) -> None:
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "c", name + ".c"),
                           os.path.join(ROOT, "oracle", "csum_oracle.c"), "-L", PKG, "-lrns_checksum",
                           f"-Wl,-rpath,{PKG}", "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", out])


@pytest.mark.parametrize("name", NAMES)
def test_builds_and_fails_loudly_without_gpu(name, tmp_path):
    from rustnetworkstack_amd import _lib
    if _lib.load().rns_device_count() > 0:
        pytest.skip("checks the GPU-less behaviour")
    exe = str(tmp_path / name)
    _compile(name, exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    # 1 would be a check that failed before the device was reached
    assert r.returncode == 2 and "no usable device" in r.stderr and "FAIL" not in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_on_gpu(name, tmp_path):
    exe = os.path.join(ROOT, "tests", "c", name)
    if not os.path.exists(exe):  # `make` builds it in-tree; a tree without it gets a private copy
        exe = str(tmp_path / name)
        _compile(name, exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all checks passed" in r.stdout
