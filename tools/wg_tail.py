#!/usr/bin/env python3
"""The tail of a bit-sliced pack-loop launch, from a stamp build's per-workgroup records.

A -DBS_STAMP library appends one "bs_wg" line per workgroup to the file LDPC_BS_WG_DUMP names
(bs_run in csrc/ldpc_bs.hip; one "bs_wg_launch" header per launch):

  LDPC_BS_WG_DUMP=bench_out/wg.txt python bench.py --steps 1 --warmup 0 --no-cpu-baseline
  python3 tools/wg_tail.py bench_out/wg.txt [--launch -1]

  bs_wg  wg packs rt_entry rt_exit clk_entry clk_exit hw_id xcc_id

rt: the 100 MHz constant-rate clock (s_memrealtime); clk: wave 0's shader clock (s_memtime);
hw_id: HW_ID of wave 0 (hex; SIMD bits 5:4, CU / SH / SE bits 15:8).

Prints, for one launch: how the workgroups of each CU fell on the SIMDs (the class of a CU is how
many of its workgroups share wave 0's SIMD with another: 0, 2 or 3 with three per CU), packs and
shader clocks per pack of each class and of each place in the CU's dispatch order (the CU's
first workgroup is its oldest for the whole launch), the distribution of the workgroups' end
times, the idle share 1 - mean(exit - entry) / (last exit - first entry), and the shader clock
under load.
"""
import argparse
import sys
from collections import Counter, defaultdict

RT_HZ = 100e6


def read_launches(path):
    """[(header line, [(wg, packs, rt0, rt1, clk0, clk1, hw, xcc), ...]), ...]"""
    launches = []
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if w[0] == "bs_wg_launch":
                launches.append((line.strip(), []))
            elif w[0] == "bs_wg":
                if not launches:
                    launches.append(("bs_wg_launch (no header)", []))
                launches[-1][1].append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), int(w[5]), int(w[6]),
                                        int(w[7], 16), int(w[8])))
    return launches


def cu_of(hw, xcc):
    return (xcc << 8) | ((hw >> 8) & 0xFF)


def simd_of(hw):
    return (hw >> 4) & 3


def cu_class(simds):
    """How many of a CU's workgroups share wave 0's SIMD with another one (the largest group)."""
    m = max(Counter(simds).values())
    return m if m >= 2 else 0


def percentile(xs, q):
    xs = sorted(xs)
    if len(xs) == 1:
        return float(xs[0])
    pos = q / 100.0 * (len(xs) - 1)
    i = int(pos)
    j = min(i + 1, len(xs) - 1)
    return xs[i] + (xs[j] - xs[i]) * (pos - i)


def analyse(recs):
    by_cu = defaultdict(list)
    for r in recs:
        by_cu[cu_of(r[6], r[7])].append(r)
    first = min(r[2] for r in recs)
    last = max(r[3] for r in recs)
    span = last - first
    res = {
        "workgroups": len(recs),
        "cus": len(by_cu),
        "packs": sum(r[1] for r in recs),
        "span_us": span / RT_HZ * 1e6,
        "idle_share": 1.0 - (sum(r[3] - r[2] for r in recs) / len(recs)) / span,
        "clock_ghz": sum(r[5] - r[4] for r in recs) / (sum(r[3] - r[2] for r in recs) / RT_HZ) / 1e9,
        "wg_per_cu": Counter(len(v) for v in by_cu.values()),
        "classes": {},
        "end_us": [(r[3] - first) / RT_HZ * 1e6 for r in recs],
    }
    cls = defaultdict(list)
    for cu, v in by_cu.items():
        cls[cu_class([simd_of(r[6]) for r in v])].append(v)
    for c, cus in sorted(cls.items()):
        wgs = [r for v in cus for r in v]
        packs = sum(r[1] for r in wgs)
        res["classes"][c] = {
            "cus": len(cus),
            "workgroups": len(wgs),
            "packs_per_wg": packs / len(wgs),
            "packs_min": min(r[1] for r in wgs),
            "packs_max": max(r[1] for r in wgs),
            "clk_per_pack": sum(r[5] - r[4] for r in wgs) / packs,
            "us_per_pack": sum(r[3] - r[2] for r in wgs) / RT_HZ * 1e6 / packs,
            "end_us": sum(r[3] - first for r in wgs) / len(wgs) / RT_HZ * 1e6,
        }
    # by a workgroup's place among its CU's, in workgroup-index order (the dispatch order: the
    # first is the oldest resident one for the whole launch)
    order = defaultdict(list)
    for v in by_cu.values():
        for k, r in enumerate(sorted(v)):
            order[k].append(r)
    res["order"] = {}
    for k, wgs in sorted(order.items()):
        packs = sum(r[1] for r in wgs)
        res["order"][k] = {
            "workgroups": len(wgs),
            "packs_per_wg": packs / len(wgs),
            "clk_per_pack": sum(r[5] - r[4] for r in wgs) / packs,
            "us_per_pack": sum(r[3] - r[2] for r in wgs) / RT_HZ * 1e6 / packs,
            "end_us": sum(r[3] - first for r in wgs) / len(wgs) / RT_HZ * 1e6,
        }
    return res


def report(head, res, out=sys.stdout):
    p = lambda *a: print(*a, file=out)
    p(head)
    p(f"workgroups {res['workgroups']}  CUs {res['cus']}  packs {res['packs']}  "
      f"workgroups per CU " + " ".join(f"{n}:{c}" for n, c in sorted(res["wg_per_cu"].items())))
    p("class = workgroups of a CU sharing wave 0's SIMD (0: all distinct)")
    for c, k in res["classes"].items():
        p(f"class {c}: CUs {k['cus']:4d} ({k['cus'] / res['cus']:.3f})  workgroups {k['workgroups']:4d}  "
          f"packs/wg {k['packs_per_wg']:.2f} ({k['packs_min']}-{k['packs_max']})  "
          f"clocks/pack {k['clk_per_pack']:.0f}  us/pack {k['us_per_pack']:.2f}  mean end {k['end_us']:.1f} us")
    p("by dispatch order on the CU (0: the CU's lowest workgroup index)")
    for k, o in res["order"].items():
        p(f"order {k}: workgroups {o['workgroups']:4d}  packs/wg {o['packs_per_wg']:.2f}  "
          f"clocks/pack {o['clk_per_pack']:.0f}  us/pack {o['us_per_pack']:.2f}  mean end {o['end_us']:.1f} us")
    e = res["end_us"]
    p("workgroup end times, us after the first entry: " +
      "  ".join(f"{n} {percentile(e, q):.1f}" for n, q in
                (("min", 0), ("p10", 10), ("p50", 50), ("p90", 90), ("p99", 99), ("max", 100))))
    p(f"launch span {res['span_us']:.1f} us")
    p(f"idle share {res['idle_share']:.4f}")
    p(f"shader clock under load {res['clock_ghz']:.3f} GHz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--launch", type=int, default=-1, help="which launch of the file (default: the last)")
    a = ap.parse_args()
    launches = [l for l in read_launches(a.path) if l[1]]
    if not launches:
        sys.exit("no bs_wg records in " + a.path)
    print(f"{len(launches)} launches in file")
    head, recs = launches[a.launch]
    report(head, analyse(recs))


if __name__ == "__main__":
    main()
