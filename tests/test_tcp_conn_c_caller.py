"""The plain C caller of the TCP connection update, the control-segment build and the close step,
tests/c/test_tcp_conn_abi.c over the one harness tests/c/abi_test.h: test_c_caller.py's two tests for one more
program (`make` builds it in-tree with the others).  Without a GPU it runs its restated lifecycle, checks the
workspace sizes and every argument error of the three entries, then exits 2 at its first device allocation."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_c_caller import _compile

NAME = "test_tcp_conn_abi"


def test_builds_and_fails_loudly_without_gpu(tmp_path):
    from rustnetworkstack_amd import _lib
    if _lib.load().rns_device_count() > 0:
        pytest.skip("checks the GPU-less behaviour")
    exe = str(tmp_path / NAME)
    _compile(NAME, exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    # 1 would be a check that failed before the device was reached
    assert r.returncode == 2 and "no usable device" in r.stderr and "FAIL" not in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_on_gpu(tmp_path):
    exe = os.path.join(ROOT, "tests", "c", NAME)
    if not os.path.exists(exe):  # `make` builds it in-tree; a tree without it gets a private copy
        exe = str(tmp_path / NAME)
        _compile(NAME, exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all checks passed" in r.stdout
