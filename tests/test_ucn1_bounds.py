"""Host-side checks of the one-chunk UCN instance of wman's geometry (CPU, no GPU): the last
kBsInst entry (index 9), which decodes without early stop take when UCN weights are set and no
earlier entry serves them -- wman with alpha' != alpha, the boosting cascade.

  - ldpc_debug_bs_bounds with flags bit 4 (LDPC_BOUNDS_UCN1 = 16) plans that entry too, with the UCN
    setting alone (only such requests are planned on it), and every read of the plan -- the hard
    decisions, cn_hd, the hard-decision addresses, the packed alpha-table address -- stays inside
    its allocation.  Without the bit the count is what it was (tests/test_es_bounds.py pins it).
  - Graphs the entry does not fit (a check degree above 15 or a variable degree above 6) have the
    same count with and without the bit.
  - The negative case: with the cn_hd guard dropped (LDPC_BOUNDS_PRE_GUARD) the check reports the
    new instance.  The guard matters where a workgroup has waves past its check lanes: wman at
    z = 24 has 9 waves, all of them check lanes, with every UCN instance (test_bs_bounds pins that
    it stays clean there); at the lifting z = 27 the column-aligned variable lanes take 12 waves
    against 11 of check lanes, and wave 11 would read past the table.
  - The dispatch (ldpc_debug_bs_frozen, as tests/test_bs_frozen.py calls it): a wman request with
    UCN weights plans instance 9 and no frozen build serves it; without them the plan is entry 0's
    and the frozen build serves it, as before."""
import pytest

from test_bs_bounds import bounds, lib  # noqa: F401  (the module's library fixture)
from test_bs_frozen import DECODE, EARLY_STOP, EXPORT, frozen
from test_bs_frozen import lib as frozen_lib  # noqa: F401

PRE_GUARD, ES, UCN1 = 1, 4, 16
WMAN, WIFI = ("wman_N0576_R34_z24", 24), ("802_11n_N648_R56_z27", 27)
BG1 = ("5G_LDPC_R0.73_n_dec2304_n2112_k1536_z72_s1537_1584", 72)
BG2 = ("5G_LDPC_R0.50_n_dec1280_n1024_k512_z64_s513_640", 64)


@pytest.mark.parametrize("T", [1, 20, 30, 50])
@pytest.mark.parametrize("au,bu", [(1, 1), (0, 0), (0, 1), (1, 0)])
@pytest.mark.parametrize("q", [5, -5, 4, 3])
def test_the_plan_under_the_bit_reads_inside_its_allocations(lib, T, au, bu, q):  # noqa: F811
    name, z = WMAN
    n0, v0, msg0 = bounds(lib, name, z, T, q=q, au=au, bu=bu)
    n, v, msg = bounds(lib, name, z, T, q=q, au=au, bu=bu, flags=UCN1)
    assert v0 == 0, msg0
    assert v == 0, msg
    assert n == n0 + 1, (n0, n)
    ne, ve, msge = bounds(lib, name, z, T, q=q, au=au, bu=bu, flags=ES)
    nb, vb, msgb = bounds(lib, name, z, T, q=q, au=au, bu=bu, flags=UCN1 | ES)
    assert (ve, vb) == (0, 0), (msge, msgb)
    assert nb == ne + 1, (ne, nb)


@pytest.mark.parametrize("name,z", [WIFI, BG2, BG1])
def test_graphs_without_the_instance(lib, name, z):  # noqa: F811
    for au, bu in ((1, 1), (0, 0)):
        n0, v0, _ = bounds(lib, name, z, 20, au=au, bu=bu)
        n, v, msg = bounds(lib, name, z, 20, au=au, bu=bu, flags=UCN1)
        assert (n, v) == (n0, v0) and v == 0, (name, au, bu, n0, n, msg)


def test_pre_guard_read_is_caught_on_the_new_instance(lib):  # noqa: F811
    name, _ = WMAN
    # z = 24: no wave past the check lanes, the dropped guard changes nothing (and the plan is there)
    n0, _, _ = bounds(lib, name, 24, 20, flags=PRE_GUARD)
    n, v, msg = bounds(lib, name, 24, 20, flags=PRE_GUARD | UCN1)
    assert n == n0 + 1 and v == 0, (n0, n, msg)
    # z = 27: 12 waves, 11 of check lanes; instance 9 is the only UCN one-chunk plan without the ES bit
    n0, v0, msg0 = bounds(lib, name, 27, 20, flags=PRE_GUARD)
    assert v0 == 0, msg0
    n, v, msg = bounds(lib, name, 27, 20, flags=UCN1)
    assert n == n0 + 1 and v == 0, (n0, n, msg)
    n, v, msg = bounds(lib, name, 27, 20, flags=PRE_GUARD | UCN1)
    assert n == n0 + 1 and v > 0, (n, v, msg)
    assert msg.startswith("instance 9 ucn: ") and "cn_hd" in msg, msg


@pytest.mark.parametrize("T", [1, 20, 30])
@pytest.mark.parametrize("au,bu", [(1, 1), (0, 0)])
def test_a_ucn_request_plans_instance_9_and_no_frozen_build(frozen_lib, monkeypatch, T, au, bu):  # noqa: F811
    monkeypatch.delenv("LDPC_BS_FROZEN", raising=False)
    monkeypatch.delenv("LDPC_BS_INST", raising=False)
    for kind in (DECODE, EXPORT):
        served, plan, _ = frozen(frozen_lib, T=T, au=au, bu=bu, ucn=1, kind=kind)
        assert plan["inst"] == 9, (kind, plan)
        assert not served
        assert plan["nw"] == 9 and plan["cn_lanes"] == 576 and plan["arows"] == (1 if au else 6)
    # the early-stop request keeps its own instance
    served, plan, _ = frozen(frozen_lib, T=T, au=au, bu=bu, ucn=1, kind=EARLY_STOP)
    assert plan["inst"] == 7 and not served


def test_a_request_without_ucn_weights_is_unchanged(frozen_lib, monkeypatch):  # noqa: F811
    monkeypatch.delenv("LDPC_BS_FROZEN", raising=False)
    monkeypatch.delenv("LDPC_BS_INST", raising=False)
    served, plan, fz = frozen(frozen_lib, ucn=0)
    assert served and plan == fz and plan["inst"] == 0
    served, plan, _ = frozen(frozen_lib, ucn=0, au=0, bu=0)
    assert not served and plan["inst"] == 0
    # forced, the entry still serves no request without UCN weights: no bsl plan, as with any
    # index past the table before it existed
    monkeypatch.setenv("LDPC_BS_INST", "9")
    served, plan, _ = frozen(frozen_lib, ucn=0)
    assert not served and plan["inst"] == -1
    served, plan, _ = frozen(frozen_lib, ucn=1)
    assert not served and plan["inst"] == 9


def test_ucn_requests_that_an_earlier_instance_serves_keep_it(frozen_lib, monkeypatch):  # noqa: F811
    monkeypatch.delenv("LDPC_BS_INST", raising=False)
    for graph, inst in ((WIFI, 3), (("MACKAY_N96_K48", 1), 3), (BG2, 5)):
        _, plan, _ = frozen(frozen_lib, graph=graph, ucn=1)
        assert plan["inst"] == inst, (graph, plan["inst"])
