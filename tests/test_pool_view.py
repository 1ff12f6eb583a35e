"""Builds and runs the host test of the pool receive view's header decode (tests/cpp/test_pool_view.cpp
over csrc/rns_k_pool_view.hpp): the decode is plain C++, so a host compiler takes it.  Nothing is loaded
into Python and no GPU is needed."""
import os
import subprocess

from conftest import ROOT


def test_pool_view(tmp_path):
    exe = tmp_path / "test_pool_view"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "rustnetworkstack_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_pool_view.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stdout
