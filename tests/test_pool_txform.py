"""Builds and runs the host test of the pool transmit form's plain-C++ parts (tests/cpp/test_pool_txform.cpp
over csrc/rns_k_pool_txform.hpp): the IP head words, the build workspace's size and the shared status bits.
Nothing is loaded into Python and no GPU is needed."""
import os
import subprocess

from conftest import ROOT


def test_pool_txform(tmp_path):
    exe = tmp_path / "test_pool_txform"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "rustnetworkstack_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pool_txform.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "all checks passed" in r.stdout
