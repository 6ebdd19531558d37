"""The int8-LLR conversion of the bit-sliced kernels on the host (CPU only):
csrc/ldpc_bitplane.h is HIP-free, so tests/native/llr8_check.cpp calls l8_bytes / l8_invalid, the
functions the kernels' int8 prologue runs, over all 256 byte values in each of the four byte lanes,
for qmax in {15, 7, 3} with and without the shortened-bit markers, and this file compares them with
the q8 format as include/ldpc_nms.h states it."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "ldpc_error_floor_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "llr8_check.cpp")


def expected(byte, qmax, big):
    """The format: (kernel byte or None when invalid) of one input byte."""
    g = byte - 256 if byte >= 128 else byte
    if -qmax <= g <= qmax:
        return g + 16
    return {-128: 48 - qmax, 127: 48 + qmax}.get(g) if big else None


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("llr8") / "llr8_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I" + CSRC, SRC, "-o", out], check=True, capture_output=True, text=True)
    return out


def test_every_byte_in_every_lane(exe):
    lines = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    assert "other" not in lines, "a byte changed another lane's output or flag"
    rows = [tuple(map(int, ln.split())) for ln in lines if ln]
    assert len(rows) == 3 * 2 * 4 * 256
    seen = set()
    for qmax, big, lane, byte, out, inv in rows:
        seen.add((qmax, big, lane, byte))
        want = expected(byte, qmax, bool(big))
        if want is None:
            assert inv == 0x80, (qmax, big, lane, byte, out, inv)
        else:
            assert (out, inv) == (want, 0), (qmax, big, lane, byte, out, inv)
    assert len(seen) == len(rows)
    # the statement itself: valid counts, and the markers only with the shortened-bit path
    for qmax in (15, 7, 3):
        assert sum(expected(b, qmax, False) is not None for b in range(256)) == 2 * qmax + 1
        assert sum(expected(b, qmax, True) is not None for b in range(256)) == 2 * qmax + 3
        assert expected(0x80, qmax, True) == 48 - qmax and expected(0x7F, qmax, True) == 48 + qmax


def test_invalid_respects_a_partial_valid_mask(exe):
    """An invalid byte counts only in a row of the pack's codewords: l8_invalid(inv, valid4) is
    nonzero exactly when an invalid lane is a valid row."""
    out = subprocess.run([exe, "mask"], capture_output=True, text=True, check=True, timeout=60).stdout
    rows = [tuple(map(int, ln.split())) for ln in out.split("\n") if ln]
    assert len(rows) == 256
    for valid4, lanes, got in rows:
        assert got == (1 if valid4 & lanes else 0), (valid4, lanes, got)
