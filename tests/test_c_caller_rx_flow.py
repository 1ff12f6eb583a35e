"""A plain C program calls the TCP flow update (rns_rx_tcp_flow_update_dev) and the ACK build
(rns_tx_ack_build_dev) the way a Rust / cgo / FFI binding would (no torch, no Python in the process):
tests/c/test_rx_flow_abi.c walks 300 meta records of four flows, checks every state, result and d_seg
record against tcp.rs:642-740 restated in C, and every ACK head against tcp_output / ip_output
restated over the oracle's primitives (oracle/csum_oracle.c, linked into the test binary only).
`make` builds it in-tree (tests/c/test_rx_flow_abi)."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "test_rx_flow_abi.c")
EXE = os.path.join(ROOT, "tests", "c", "test_rx_flow_abi")
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
        exe = str(tmp_path / "test_rx_flow_abi")
        _compile(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all checks passed" in r.stdout
