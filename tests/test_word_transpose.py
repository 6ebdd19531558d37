"""The word mode's 32 x 32 bit transpose on the host (CPU only): tr32_step of csrc/ldpc_bitplane.h
is plain C++, so tests/native/transpose_check.cpp simulates the 32 lanes of k_word_out's exchange
(csrc/ldpc_word.hip) and checks the five rounds against the definition, out[r] bit c = in[c] bit r,
on random and one-bit matrices and in every order of the rounds."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "ldpc_error_floor_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "transpose_check.cpp")


def test_transpose_rounds(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "transpose_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I" + CSRC, SRC, "-o", exe], check=True,
                   capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.startswith("ok ")
