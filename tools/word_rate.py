#!/usr/bin/env python3
"""Rates of the decoded-word mode beside the counters-only decode, one GPU:

    python3 tools/word_rate.py [--configs C2 C3 C4 C5] [--batch 1048576] [--runs 3] [--steps 3]
    python3 tools/word_rate.py --root /path/to/another/checkout --modes counters      # A/B

Per config (its own T, weights and SNR; LLRs of dec.awgn, resident): HIP-event milliseconds per
decode of `decode(counters=True)` and of `decode(hard_last=True, word_flags=True, counters=True)`,
`--runs` times each, interleaved.  `--old-path B`: also the existing `decode(hard=True)` export
against the new call at batch B (where the old path's [T]-sized buffers fit).  One JSON line per
measurement.  The split between the decode kernel and k_word_out comes from a kernel trace of
this tool (rocprofv3 --kernel-trace --stats -- python3 tools/word_rate.py --runs 1)."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--configs", nargs="+", default=["C2", "C3", "C4", "C5"])
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["counters", "word"], choices=["counters", "word"])
    ap.add_argument("--old-path", type=int, default=0, metavar="B")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    import bench
    from ldpc_error_floor_amd.decoder import NMSDecoder
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize(dev)
        return round(e0.elapsed_time(e1) / a.steps, 3)

    for config in a.configs:
        cfg = bench.CONFIGS[config]
        T = cfg["T"]
        proto, g, W, cp = bench.load_problem(T, config)
        B = a.batch
        dec = NMSDecoder(proto, cfg["z"], W, 2, 5, device=dev, B_max=B)
        llr = dec.awgn(B, float(cp.sigma(cfg["snr"])), seed=1076, punct=cfg.get("punct", (0, 0)),
                       short=cfg.get("short", (0, 0)))
        cnt = torch.zeros(4, dtype=torch.int64, device=dev)
        fns = {"counters": lambda: dec.decode(llr, T=T, app=False, counters=cnt)}
        if "word" in a.modes:
            hl = torch.empty((B, (dec.n_vars + 31) // 32), dtype=torch.int32, device=dev)
            fns["word"] = lambda: dec.decode(llr, T=T, hard_last=hl, word_flags=True, counters=cnt,
                                             on_off_grid="mark")
        for run in range(a.runs):
            for mode in a.modes:
                ms = timed(fns[mode])
                print(json.dumps({"config": config, "B": B, "T": T, "mode": mode, "run": run, "ms": ms,
                                  "Mcw_per_s": round(B / ms / 1e3, 2), "kernel": dec.last_kernel()}), flush=True)
        if a.old_path and config == a.configs[0]:
            Bo = a.old_path
            sub = llr[:Bo]
            for run in range(a.runs):
                for mode, fn in (("hard_all_T", lambda: dec.decode(sub, T=T, app=False, hard=True, counters=cnt)),
                                 ("word", lambda: dec.decode(sub, T=T, hard_last=True, word_flags=True,
                                                             counters=cnt, on_off_grid="mark"))):
                    print(json.dumps({"config": config, "B": Bo, "T": T, "mode": mode, "run": run,
                                      "ms": timed(fn), "kernel": dec.last_kernel()}), flush=True)
        del llr, dec
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
