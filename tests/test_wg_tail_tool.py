"""tools/wg_tail.py on a hand-written dump (tests/golden/wg_tail_two_cus.txt; CPU only): two CUs of
three workgroups each, one with every wave 0 on the same SIMD (class 3), one with three distinct
SIMDs (class 0).  The figures below are worked out by hand from the dump's numbers:
  durations 1000, 990, 990 ticks (class 3) and 800, 800, 900 (class 0); span 2000 - 1000 = 1000
  idle share 1 - (5480 / 6) / 1000 = 0.08667
  shader clocks 59600 over 12 packs (class 3: 4966.7 per pack), 50000 over 15 (class 0: 3333.3)
  109600 clocks in 5480 ticks of 10 ns: 2.000 GHz"""
import importlib.util
import io
import os

import pytest

from conftest import GOLDEN, ROOT

DUMP = os.path.join(GOLDEN, "wg_tail_two_cus.txt")


def _tool():
    spec = importlib.util.spec_from_file_location("wg_tail", os.path.join(ROOT, "tools", "wg_tail.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _result():
    tool = _tool()
    launches = tool.read_launches(DUMP)
    assert len(launches) == 1 and len(launches[0][1]) == 6
    assert launches[0][0].startswith("bs_wg_launch inst 0 T 20")
    return tool, launches[0][0], tool.analyse(launches[0][1])


def test_classes_of_the_two_cus():
    _, _, res = _result()
    assert res["workgroups"] == 6 and res["cus"] == 2 and res["packs"] == 27
    assert dict(res["wg_per_cu"]) == {3: 2}
    assert sorted(res["classes"]) == [0, 3]
    c0, c3 = res["classes"][0], res["classes"][3]
    assert (c0["cus"], c0["workgroups"], c3["cus"], c3["workgroups"]) == (1, 3, 1, 3)
    assert c0["packs_per_wg"] == 5 and c3["packs_per_wg"] == 4
    assert c0["clk_per_pack"] == pytest.approx(50000 / 15)
    assert c3["clk_per_pack"] == pytest.approx(59600 / 12)
    assert c3["us_per_pack"] == pytest.approx(29.8 / 12)


def test_class_of_a_cu():
    tool = _tool()
    assert tool.cu_class([0, 1, 3]) == 0
    assert tool.cu_class([2, 1, 2]) == 2
    assert tool.cu_class([2, 2, 2]) == 3
    assert tool.cu_class([1]) == 0
    # the CU is XCC and the SE / SH / CU bits of HW_ID; the SIMD is bits 5:4, the wave slot is not in it
    assert tool.cu_of(0x0123, 0) == tool.cu_of(0x0126, 0) != tool.cu_of(0x0123, 1)
    assert tool.simd_of(0x0232) == 3


def test_dispatch_order_on_the_cu():
    """Workgroups 0 and 1 are their CUs' first, 4 and 5 the last: 9 packs in 1800 ticks and 36000
    clocks, and 9 packs in 1890 ticks and 37800 clocks."""
    _, _, res = _result()
    assert sorted(res["order"]) == [0, 1, 2]
    o0, o2 = res["order"][0], res["order"][2]
    assert o0["workgroups"] == 2 and o0["packs_per_wg"] == 4.5
    assert o0["us_per_pack"] == pytest.approx(2.0) and o0["clk_per_pack"] == pytest.approx(4000)
    assert o2["us_per_pack"] == pytest.approx(2.1) and o2["clk_per_pack"] == pytest.approx(4200)


def test_idle_share_clock_and_end_times():
    _, _, res = _result()
    assert res["idle_share"] == pytest.approx(1 - (5480 / 6) / 1000)
    assert res["clock_ghz"] == pytest.approx(2.0)
    assert res["span_us"] == pytest.approx(10.0)
    assert sorted(res["end_us"]) == pytest.approx([8.0, 8.0, 9.0, 9.9, 10.0, 10.0])


def test_printed_report():
    tool, head, res = _result()
    out = io.StringIO()
    tool.report(head, res, out)
    text = out.getvalue()
    assert "workgroups 6  CUs 2  packs 27  workgroups per CU 3:2" in text
    assert "class 0: CUs    1 (0.500)  workgroups    3  packs/wg 5.00 (5-5)  clocks/pack 3333" in text
    assert "class 3: CUs    1 (0.500)  workgroups    3  packs/wg 4.00 (4-4)  clocks/pack 4967" in text
    assert "order 2: workgroups    2  packs/wg 4.50  clocks/pack 4200  us/pack 2.10" in text
    assert "idle share 0.0867" in text
    assert "shader clock under load 2.000 GHz" in text
    assert "max 10.0" in text and "min 8.0" in text
