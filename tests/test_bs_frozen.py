"""The geometry-frozen builds of the bit-sliced kernel (csrc/ldpc_bs_frozen.h), the
host side (CPU, no GPU): ldpc_debug_bs_frozen runs the launch's own planning and dispatch
(bs_route, bs_frozen_fit) for a request on a proto graph.

  - The plan of the shipped wman graph (N576 R3/4, z = 24, LPC 4, one alpha and one beta per
    iteration, T = 20) equals every frozen constant, field by field: a change of slot_layout or
    plan_inst fails here instead of switching the fast path off silently.
  - A default wman request takes the frozen build; another graph, UCN or per-row / per-column
    weights, an early-stop request, an export / word request, more iterations than the frozen RED
    region holds, and LDPC_BS_FROZEN=0 do not.
  - tools/isa_phase_table.py takes the innermost loop that holds both barriers as the T loop
    (tests/golden/isa_two_level_loop.s: the pack loop around it has barriers of its own)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from ldpc_error_floor_amd.code import load_base_graph

LIB = os.path.join(ROOT, "ldpc_error_floor_amd", "libldpc_nms.so")
BG = os.path.join(ROOT, "ldpc_error_floor_amd", "data", "BaseGraph")
MODE = {5: 1, -5: 2, 4: 3, 3: 4}
NF = 22
DECODE, EARLY_STOP, EXPORT = 0, 1, 2
WMAN = ("wman_N0576_R34_z24", 24)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run python -m ldpc_error_floor_amd.build")
    L = ctypes.CDLL(LIB)
    i32, p32 = ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)
    L.ldpc_debug_bs_frozen.argtypes = [p32, i32, i32, i32, i32, i32, i32, i32, i32, i32, ctypes.c_float,
                                       p32, p32, i32, ctypes.c_char_p, i32]
    return L


def frozen(lib, graph=WMAN, T=20, q=5, au=1, bu=1, ucn=0, kind=DECODE, clip=20.0):
    """(served by a frozen build, the plan's fields, the frozen constants), both by field name."""
    name, z = graph
    P = np.ascontiguousarray(load_base_graph(os.path.join(BG, name + ".txt")), np.int32)
    plan, fz = (ctypes.c_int32 * NF)(), (ctypes.c_int32 * NF)()
    names = ctypes.create_string_buffer(512)
    r = lib.ldpc_debug_bs_frozen(P.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), P.shape[0], P.shape[1], z,
                                 T, MODE[q], au, bu, ucn, kind, clip, plan, fz, NF, names, 512)
    assert r in (0, 1), r
    keys = names.value.decode().split(",")
    assert len(keys) == NF, keys
    return r == 1, dict(zip(keys, plan)), dict(zip(keys, fz))


def test_the_wman_plan_equals_every_frozen_constant(lib, monkeypatch):
    monkeypatch.delenv("LDPC_BS_FROZEN", raising=False)
    served, plan, fz = frozen(lib)
    for k in fz:
        assert plan[k] == fz[k], (k, plan[k], fz[k])
    assert served
    # what the header states in words
    assert fz["n_vars"] == 576 and fz["n_checks"] == 144 and fz["z"] == 24 and fz["NT"] == 576 and fz["nw"] == 9
    assert fz["cstride"] == 24 * 20 and fz["AL"] == 64 and fz["BL"] == 68
    # the forced generic build sees the same plan (as bs_plan computes it)
    monkeypatch.setenv("LDPC_BS_FROZEN", "0")
    served0, plan0, _ = frozen(lib)
    assert not served0 and plan0 == plan


@pytest.mark.parametrize("T", [1, 2, 3, 16, 17, 20])
@pytest.mark.parametrize("q", [5, -5, 4, 3])
def test_a_default_wman_request_takes_the_frozen_build(lib, monkeypatch, T, q):
    """Any T up to the frozen RED region's 20 words and every QMS grid (qmax is a run-time
    argument): the plan, with RED sized for 20 iterations, equals the constants."""
    monkeypatch.delenv("LDPC_BS_FROZEN", raising=False)
    served, plan, fz = frozen(lib, T=T, q=q)
    assert served and plan == fz, (T, q)


@pytest.mark.parametrize("what,kw", [
    ("802.11n", dict(graph=("802_11n_N648_R56_z27", 27))),
    ("MacKay", dict(graph=("MACKAY_N96_K48", 1))),
    ("wman at another lifting", dict(graph=("wman_N0576_R34_z24", 27))),
    ("UCN weights", dict(ucn=1)),
    ("per-row alpha", dict(au=0)),
    ("per-column beta", dict(bu=0)),
    ("per-row alpha and per-column beta", dict(au=0, bu=0)),
    ("early stop", dict(kind=EARLY_STOP)),
    ("export / word mode", dict(kind=EXPORT)),
    ("T past the frozen RED region", dict(T=21)),
    ("T = 50", dict(T=50)),
])
def test_every_other_request_takes_the_generic_build(lib, monkeypatch, what, kw):
    monkeypatch.delenv("LDPC_BS_FROZEN", raising=False)
    served, _, _ = frozen(lib, **kw)
    assert not served, what


def test_the_switch_forces_the_generic_build(lib, monkeypatch):
    monkeypatch.setenv("LDPC_BS_FROZEN", "0")
    assert not frozen(lib)[0]
    monkeypatch.setenv("LDPC_BS_FROZEN", "1")
    assert frozen(lib)[0]
    monkeypatch.delenv("LDPC_BS_FROZEN")
    assert frozen(lib)[0]


def test_null_context_query(lib):
    assert lib.ldpc_ctx_last_frozen(None) == -1


def _phase_tool():
    spec = importlib.util.spec_from_file_location("isa_phase_table", os.path.join(ROOT, "tools", "isa_phase_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_phase_tool_takes_the_inner_loop_with_both_barriers():
    """The pack loop (depth 1) holds two barriers of its prologue, the T loop (depth 2) the check and
    the variable barrier, and a depth-3 copy loop sits inside it: the T loop is BB0_3, its members
    include the copy loop's blocks, and the prologue's v_rndne / v_cvt_pk_u8 and the pack loop's
    scratch reload are in no phase."""
    tool = _phase_tool()
    path = os.path.join(GOLDEN, "isa_two_level_loop.s")
    _, body = tool.function_lines(open(path).read().splitlines(), "k_bs_mini")
    head, members = tool.t_loop(tool.blocks_of(body))
    assert head == "BB0_3"
    assert members == {".LBB0_3", ".LBB0_4", "%bb.5"}
    _, tloop, c = tool.loop_counts(path, "k_bs_mini")
    assert tloop == "BB0_3"
    assert c["s_barrier"] == 2 and c["scalar loads"] == 1 and c["VALU"] == 5 and c["v_readlane"] == 1
    assert "scratch accesses" not in c
    _, counts, _, _ = tool.analyse(path, "k_bs_mini")
    assert set(counts) == {"top.0", "ck_min.0", "vn_sum.0"}
    assert sum(counts["top.0"].values()) == 1           # the copy loop's v_add, nothing of the prologue
