"""A plain C program calls TCP send planning (rns_tx_tcp_plan_dev) and then the segmentation offload
(rns_tx_segment_dev) on the planned descriptors, the way a Rust / cgo / FFI binding would (no torch, no
Python in the process): tests/c/test_tx_plan_abi.c plans 40 flows, checks every output array against
tcp.rs:256-292, 329-348 and 402-447 restated in C piece by piece, launches the segmentation with
n_seg = seg_cap on the same stream and checks every arena byte and status against the oracle's chain
finalize (oracle/csum_oracle.c, linked into the test binary only).
`make` builds it in-tree (tests/c/test_tx_plan_abi)."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "test_tx_plan_abi.c")
EXE = os.path.join(ROOT, "tests", "c", "test_tx_plan_abi")
PKG = os.path.join(ROOT, "rustnetworkstack_amd")


def _compile(out: str) -> None:
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", SRC,
                           os.path.join(ROOT, "oracle", "csum_oracle.c"), "-L", PKG, "-lrns_checksum",
                           f"-Wl,-rpath,{PKG}", "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", out])


@pytest.mark.gpu
def test_c_caller_on_gpu(tmp_path):
    exe = EXE
    if not os.path.exists(exe):  # `make` builds it in-tree; a tree without it gets a private copy
        exe = str(tmp_path / "test_tx_plan_abi")
        _compile(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all checks passed" in r.stdout
