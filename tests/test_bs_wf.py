"""The dispatch of the bit-sliced builds with the weights frozen in kind (csrc/ldpc_bs_kernel.h, WF;
DESIGN 3.3), the host side (CPU, no GPU): ldpc_debug_bs_wf analyses a weight set as
ldpc_weights_set does and runs the launch's own planning and dispatch (bs_route, bs_frozen_fit,
bs_weight_path) for a request on a proto graph.

A launch takes such a build only when the geometry-frozen build would be taken, every iteration's
check table and channel table is one of the fixed set of csrc/ldpc_beta_tabs.h (or the identity
channel table), and no switch says otherwise:

  - the shipped C2 weights are taken at q = 5 and q = -5, for every T up to 20;
  - one check id missing at one iteration (no float alpha's table is outside the set, so the id is
    taken out by hand), per-row alpha, UCN weights, T = 21, q = 4, a channel
    table outside the set or differing by column, the early-stop and export requests, and each of
    LDPC_BS_WF=0, LDPC_BS_AFIX=0, LDPC_BS_NOBFIX and LDPC_BS_FROZEN=0 fall back;
  - the ids handed to the kernel equal host::alpha_table_id of each iteration's alpha and
    host::beta_table_id's table of each iteration's beta, element by element: both are checked
    against numpy float32 restatements of the tables, through the set's rows."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from ldpc_error_floor_amd.code import TannerGraph, load_base_graph
from ldpc_error_floor_amd.weights import expand_weights, read_weight_file

LIB = os.path.join(ROOT, "ldpc_error_floor_amd", "libldpc_nms.so")
DATA = os.path.join(ROOT, "ldpc_error_floor_amd", "data")
Q5, QM5, Q4 = 1, 2, 3                              # the modes of csrc/ldpc_host.h
NTAB = 210
SWITCHES = [("LDPC_BS_WF", "0"), ("LDPC_BS_AFIX", "0"), ("LDPC_BS_NOBFIX", "1"), ("LDPC_BS_FROZEN", "0")]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m ldpc_error_floor_amd.build")
    L = ctypes.CDLL(LIB)
    i32, p32 = ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)
    pf = ctypes.POINTER(ctypes.c_float)
    L.ldpc_debug_bs_wf.argtypes = [p32, i32, i32, i32, i32, pf, pf, pf, i32, i32, i32, ctypes.c_float, p32, p32,
                                   ctypes.POINTER(ctypes.c_uint64), p32]
    L.ldpc_debug_alpha_tid.argtypes = [ctypes.c_float, i32, p32, ctypes.POINTER(ctypes.c_uint8)]
    return L


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name, _ in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def c2():
    proto = load_base_graph(os.path.join(DATA, "BaseGraph", "wman_N0576_R34_z24.txt"))
    wf = read_weight_file(os.path.join(DATA, "Weights", "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt"))
    g = TannerGraph(proto, 24)
    W = expand_weights((3, 0, 3), {0: wf.blocks[0], 2: wf.blocks[2]}, 20, g)
    return proto, g, W


@pytest.fixture(scope="module")
def tabs():
    """The 210 rows of kBetaTab, read from the header."""
    src = open(os.path.join(ROOT, "ldpc_error_floor_amd", "csrc", "ldpc_beta_tabs.h")).read()
    body = src.split("kBetaTab[kNBetaTab][16] = {", 1)[1].split("};", 1)[0]
    rows = [[int(x) for x in re.findall(r"\d+", r)] for r in re.findall(r"\{([^{}]*)\}", body)]
    t = np.array(rows, np.uint8)
    assert t.shape == (NTAB, 16)
    return t


def wf(lib, proto, z, alpha, beta, T, mode=Q5, kind=0, alpha_ucn=None, tid_in=None):
    """(ldpc_debug_bs_wf's return, the check ids, the channel ids, the identity mask); tid_in: check
    ids that replace the analysis' own"""
    P = np.ascontiguousarray(proto, np.int32)
    p32, pf = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    a = np.ascontiguousarray(alpha, np.float32)
    b = np.ascontiguousarray(beta, np.float32)
    u = None if alpha_ucn is None else np.ascontiguousarray(alpha_ucn, np.float32)
    aids, bids = np.full(T, -9, np.int32), np.full(T, -9, np.int32)
    ident = ctypes.c_uint64(0)
    r = lib.ldpc_debug_bs_wf(P.ctypes.data_as(p32), P.shape[0], P.shape[1], z, a.shape[0], a.ctypes.data_as(pf),
                             None if u is None else u.ctypes.data_as(pf), b.ctypes.data_as(pf), T, mode, kind,
                             ctypes.c_float(20.0), aids.ctypes.data_as(p32), bids.ctypes.data_as(p32),
                             ctypes.byref(ident),
                             None if tid_in is None else np.ascontiguousarray(tid_in, np.int32).ctypes.data_as(p32))
    assert r in (0, 1), r
    return r, aids, bids, ident.value


def alpha_row(alpha, step):
    """q_mag5 for m = 0..15 in float32: fl32(fl32(m step) alpha), relu, / step, rint, clamp."""
    m = np.arange(16, dtype=np.float32)
    x = (m * np.float32(step)).astype(np.float32) * np.float32(alpha)
    x = np.where(x > 0, x, np.float32(0)).astype(np.float32)
    return np.clip(np.rint((x * (np.float32(1) / np.float32(step))).astype(np.float32)), -15, 15).astype(np.uint8)


def beta_row(beta):
    """min(15, |rint(fl32(m beta))|) for m = 0..15."""
    m = np.arange(16, dtype=np.float32)
    return np.minimum(15, np.abs(np.rint((m * np.float32(beta)).astype(np.float32)))).astype(np.uint8)


@pytest.mark.parametrize("mode", [Q5, QM5])
@pytest.mark.parametrize("T", [1, 2, 7, 20])
def test_c2_weights_are_taken_and_the_ids_name_the_tables(lib, c2, tabs, mode, T):
    proto, g, W = c2
    r, aids, bids, ident = wf(lib, proto, 24, W.alpha, W.beta, T, mode)
    assert r == 1
    step = 0.5 if mode == Q5 else 1.0
    for t in range(T):
        k = ctypes.c_int32(-7)
        assert lib.ldpc_debug_alpha_tid(ctypes.c_float(float(W.alpha[t, 0])), mode, ctypes.byref(k), None) == 0
        assert aids[t] == k.value and 0 <= aids[t] < NTAB, (t, aids[t], k.value)
        assert np.array_equal(tabs[aids[t]], alpha_row(W.alpha[t, 0], step)), t
        assert (W.beta[t] == W.beta[t, 0]).all()
        if (ident >> t) & 1:
            assert np.array_equal(beta_row(W.beta[t, 0]), np.arange(16)), t
        else:
            assert 0 <= bids[t] < NTAB, (t, bids[t])
        if bids[t] >= 0:
            assert np.array_equal(tabs[bids[t]], beta_row(W.beta[t, 0])), t


def test_identity_channel_tables_are_taken(lib, c2, tabs):
    """beta = 1 at some iterations: the identity mask has their bits, and the request is taken."""
    proto, g, W = c2
    beta = W.beta.copy()
    beta[[0, 3, 19]] = 1.0
    r, aids, bids, ident = wf(lib, proto, 24, W.alpha, beta, 20)
    assert r == 1
    assert all((ident >> t) & 1 for t in (0, 3, 19))
    assert np.array_equal(tabs[bids[3]], np.arange(16))          # (the identity is also a row of the set)


def test_requests_that_fall_back(lib, c2):
    proto, g, W = c2
    assert wf(lib, proto, 24, W.alpha, W.beta, 20)[0] == 1
    # one alpha outside the fixed set at one iteration: no float alpha has such a table
    # (test_every_alpha_is_in_the_set), so the id of iteration 7 is put to -1 by hand.  The ids go
    # up per weight set, all or none, so a T that stops short of that iteration falls back too.
    ids = wf(lib, proto, 24, W.alpha, W.beta, 20)[1].copy()
    assert wf(lib, proto, 24, W.alpha, W.beta, 20, tid_in=ids)[0] == 1
    ids[7] = -1
    r, aids, bids, _ = wf(lib, proto, 24, W.alpha, W.beta, 20, tid_in=ids)
    assert r == 0 and (aids == -1).all() and (bids >= 0).all()
    assert wf(lib, proto, 24, W.alpha, W.beta, 5, tid_in=ids)[0] == 0
    # per-row alpha
    rows = np.asarray(g.pe_row)
    pr = (W.alpha * np.where(rows % 2 == 0, 1.0, 0.75).astype(np.float32)[None, :]).astype(np.float32)
    assert wf(lib, proto, 24, pr, W.beta, 20)[0] == 0
    # UCN weights
    assert wf(lib, proto, 24, W.alpha, W.beta, 20, alpha_ucn=(W.alpha * np.float32(0.5)).astype(np.float32))[0] == 0
    # (alpha' equal to alpha is no UCN decoder)
    assert wf(lib, proto, 24, W.alpha, W.beta, 20, alpha_ucn=W.alpha.copy())[0] == 1
    # T = 21: past the frozen builds' T_CAP
    a21 = np.concatenate([W.alpha, W.alpha[-1:]])
    b21 = np.concatenate([W.beta, W.beta[-1:]])
    assert wf(lib, proto, 24, a21, b21, 21)[0] == 0
    assert wf(lib, proto, 24, a21, b21, 20)[0] == 1
    # q = 4: no fixed set
    r, aids, bids, _ = wf(lib, proto, 24, W.alpha, W.beta, 20, Q4)
    assert r == 0 and (aids == -1).all() and (bids == -1).all()
    # a negative beta at one iteration, and a beta that differs by column
    b = W.beta.copy()
    b[11, :] = -0.5
    assert wf(lib, proto, 24, W.alpha, b, 20)[0] == 0
    b = W.beta.copy()
    b[4, 5] = b[4, 5] * np.float32(0.5)
    assert wf(lib, proto, 24, W.alpha, b, 20)[0] == 0
    # early stop and the export / word builds
    assert wf(lib, proto, 24, W.alpha, W.beta, 20, kind=1)[0] == 0
    assert wf(lib, proto, 24, W.alpha, W.beta, 20, kind=2)[0] == 0


def test_every_alpha_is_in_the_set(lib):
    """Both grids' steps are powers of two, so the check table of any alpha is rint(m alpha) clamped,
    one of the set's rows: a sweep of [0, 16] and the exact halves with their neighbours finds no
    alpha without an id -- which is why the fall-back case above sets an id to -1 by hand."""
    halves = np.array([(2 * r + 1) / (2.0 * m) for m in range(1, 16) for r in range(16)], np.float32)
    a = np.concatenate([np.linspace(0, 16, 1601).astype(np.float32), halves,
                        np.nextafter(halves, np.float32(0)), np.nextafter(halves, np.float32(99))])
    for mode in (Q5, QM5):
        for x in a:
            k = ctypes.c_int32(-7)
            assert lib.ldpc_debug_alpha_tid(ctypes.c_float(float(x)), mode, ctypes.byref(k), None) == 0
            assert 0 <= k.value < NTAB, (x, mode, k.value)


@pytest.mark.parametrize("name,value", SWITCHES)
def test_each_switch_falls_back(lib, c2, monkeypatch, name, value):
    proto, g, W = c2
    assert wf(lib, proto, 24, W.alpha, W.beta, 20)[0] == 1
    monkeypatch.setenv(name, value)
    r, aids, bids, _ = wf(lib, proto, 24, W.alpha, W.beta, 20)
    assert r == 0
    if name == "LDPC_BS_AFIX":
        assert (aids == -1).all() and (bids >= 0).all()
    if name == "LDPC_BS_NOBFIX":
        assert (bids == -1).all() and (aids >= 0).all()
    if name == "LDPC_BS_WF":
        assert (aids >= 0).all()                                 # (the ids still go to the other builds)
        monkeypatch.setenv(name, "1")
        assert wf(lib, proto, 24, W.alpha, W.beta, 20)[0] == 1
