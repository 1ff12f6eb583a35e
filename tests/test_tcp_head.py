"""Builds and runs the host test of the shared TCP head builder (tests/cpp/test_tcp_head.cpp over
csrc/rns_k_tcp_head.hpp): the header is plain C++, so a host compiler takes it and the oracle checks
the checksums it closes.  Nothing is loaded into Python and no GPU is needed."""
import os
import subprocess

from conftest import ROOT


def test_tcp_head(tmp_path):
    exe, obj = tmp_path / "test_tcp_head", tmp_path / "csum_oracle.o"
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-c", os.path.join(ROOT, "oracle", "csum_oracle.c"), "-o", str(obj)])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "rustnetworkstack_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_tcp_head.cpp"), str(obj), "-lpthread", "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stdout
