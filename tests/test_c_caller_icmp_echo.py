"""A plain C program calls the ICMP echo responder (rns_rx_icmp_echo_pool_dev, rns_rx_icmp_echo_work)
the way a Rust / cgo / FFI binding would (no torch, no Python in the process):
tests/c/test_icmp_echo_abi.c answers 200 datagrams in shuffled 512-byte buffers — echo requests over
IPv4 (with options) and IPv6 among echo replies, UDP and corrupted requests — and checks every flag,
count, id, descriptor and reply byte against replies it builds itself, then again with a free list
that runs out.  `make` builds it in-tree (tests/c/test_icmp_echo_abi)."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "test_icmp_echo_abi.c")
EXE = os.path.join(ROOT, "tests", "c", "test_icmp_echo_abi")
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
        exe = str(tmp_path / "test_icmp_echo_abi")
        _compile(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all checks passed" in r.stdout
