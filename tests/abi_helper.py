"""What the C-ABI tests without a GPU (test_*abi.py) share: pointers that are never dereferenced, the
check of the header's constants against the binding's, and the header compiled as C."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from rustnetworkstack_amd import _lib

INCLUDE = os.path.join(ROOT, "include")
FAKE = ctypes.c_void_p(4096)      # aligned for every element type; the argument checks never read it
ODD = ctypes.c_void_p(4096 + 2)   # misaligned for 4- and 8-byte elements
BIG = 1 << 40                     # a workspace size no check finds short


def assert_header_defines(names):
    """Every `#define NAME <n>u` of include/rns_checksum.h holds the value the binding has for NAME."""
    text = open(os.path.join(INCLUDE, "rns_checksum.h")).read()
    for name in names:
        m = re.search(rf"#define {name}\s+(\d+)u", text)
        assert m and int(m.group(1)) == getattr(_lib, name), name


def assert_header_compiles(body, std="c11"):
    """`body` (a _Static_assert, a main) compiles behind the header: gcc -Wall -Werror -fsyntax-only."""
    subprocess.run(["gcc", f"-std={std}", "-Wall", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-fsyntax-only"],
                   input='#include "rns_checksum.h"\n' + body, text=True, check=True)
