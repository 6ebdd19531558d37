#!/usr/bin/env python3
"""Step times of wman (C2's graph) with UCN weights alpha' != alpha -- the boosting cascade -- at
B = 2^20 on one GPU (profiles/wman_ucn/): the bit-sliced instance
``bsl[p32,w9,d15,v6,l4,ucn]`` against the v5 kernel, which serves the same requests under
``LDPC_BS=0`` (and served them before the instance existed), alternating in one process.

  python tools/wman_ucn_step.py [out_dir] [--cases cascade30,ucn20] [--modes decode,awgn,...]
                                [--paths bsl,v5] [--rounds 2] [--batch B] [--snr DB] [--tree DIR]

  cases   cascade30: T = 30, rows 0-19 the shipped wman weights (alpha' = alpha: those iterations
          skip the UCN work), rows 20-29 random with alpha' != alpha (seed 5; the weights of
          tests/test_gpu_bs_wman_ucn.py); ucn20: T = 20, random alpha' != alpha at every iteration
  modes   decode (counters-only ``decode`` of ``awgn()`` rows), awgn (``decode_awgn``); word /
          events (``decode(hard_last=)`` / ``decode(events=)`` at full T) and es / es_word /
          es_events (``decode_awgn(early_stop=True ...)``): the bit-sliced path only
  paths   bsl (the default routing), v5 (``LDPC_BS=0``, read at every decode)
  --tree  import the package and bench.py of another checkout (a built parent commit)

Per (case, mode, path, round): five HIP-event timings after two warm-up decodes and their median,
one JSON line each, and ``<out>/wman_ucn_step.json``.  The counters of both paths must be equal."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSL_ONLY = ("word", "events", "es", "es_word", "es_events")


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--cases", default="cascade30,ucn20")
    ap.add_argument("--modes", default="decode,awgn")
    ap.add_argument("--paths", default="bsl,v5")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--snr", type=float, default=3.5)
    ap.add_argument("--cap", type=int, default=1 << 16)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--tag", default="")
    return ap.parse_args(argv)


def weights(case, g):
    import numpy as np
    from ldpc_error_floor_amd.weights import expand_weights, read_weight_file
    wf = read_weight_file(os.path.join(ROOT, "ldpc_error_floor_amd", "data", "Weights",
                                       "C0_wman_N0576_R34_z24_Opt_Weight_End20.txt"))
    rs = np.random.RandomState(5)
    if case == "cascade30":
        T = 30
        a = np.concatenate([wf.blocks[0][:20], rs.uniform(0.5, 1.0, (10, 1))])
        u = np.concatenate([wf.blocks[0][:20], rs.uniform(0.2, 0.5, (10, 1))])
        b = np.concatenate([wf.blocks[2][:20], rs.uniform(0.8, 1.1, (10, 1))])
    elif case == "ucn20":
        T = 20
        a, u, b = rs.uniform(0.5, 1.0, (T, 1)), rs.uniform(0.2, 0.5, (T, 1)), rs.uniform(0.8, 1.1, (T, 1))
    else:
        raise SystemExit(f"unknown case {case!r}")
    return expand_weights((3, 3, 3), {0: a, 1: u, 2: b}, T, g)


def main(argv=None):
    a = parse(argv)
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np, torch
    import bench
    from ldpc_error_floor_amd.decoder import NMSDecoder
    B = a.batch
    dev = torch.device("cuda", 0)
    rows = []
    env0 = os.environ.pop("LDPC_BS", None)
    proto, g, _, cp = bench.load_problem(config="C2")
    sigma = float(cp.sigma(a.snr))
    for case in a.cases.split(","):
        dec = NMSDecoder(proto, 24, weights(case, g), 2, 5, device=dev, B_max=B)
        llr = dec.awgn(B, sigma, seed=11)
        modes = a.modes.split(",")
        hl = buf = None
        if "word" in modes or "es_word" in modes:
            hl = torch.empty((B, (dec.n_vars + 31) // 32), dtype=torch.int32, device=dev)
        if "events" in modes or "es_events" in modes:
            from ldpc_error_floor_amd.events import EventBuffer
            buf = EventBuffer(dec, a.cap)

        def run(mode):
            cnt = torch.zeros(4, dtype=torch.int64, device=dev)
            if buf is not None:
                buf.reset()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if mode == "decode":
                dec.decode(llr, app=False, counters=cnt)
            elif mode == "awgn":
                dec.decode_awgn(B, sigma, 11, counters=cnt)
            elif mode == "word":
                dec.decode(llr, hard_last=hl, word_flags=True, counters=cnt)
            elif mode == "events":
                dec.decode(llr, events=buf, counters=cnt)
            else:
                kw = {"es": {}, "es_word": dict(hard_last=hl, word_flags=True), "es_events": dict(events=buf)}[mode]
                dec.decode_awgn(B, sigma, 11, counters=cnt, early_stop=True, **kw)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), cnt.cpu().numpy()

        ref = {}
        for rnd in range(a.rounds):
            for mode in modes:
                for path in a.paths.split(","):
                    if path == "v5" and mode in BSL_ONLY:
                        continue
                    if path == "v5":
                        os.environ["LDPC_BS"] = "0"
                    else:
                        os.environ.pop("LDPC_BS", None)
                    for _ in range(2):
                        run(mode)
                    ts = []
                    for _ in range(5):
                        t, c = run(mode)
                        ts.append(t)
                    os.environ.pop("LDPC_BS", None)
                    key = "es" if mode.startswith("es") else "full"
                    c = c[:3] if key == "es" else c
                    assert np.array_equal(ref.setdefault(key, c), c), (case, mode, path, ref[key], c)
                    out = {"case": case, "T": dec.T, "snr_db": a.snr, "B": B, "mode": mode, "path": path, "round": rnd,
                           "kernel": dec.last_kernel(), "ms": [round(x, 3) for x in ts],
                           "ms_median": round(float(np.median(ts)), 3),
                           "Mcw_per_s": round(B / float(np.median(ts)) / 1e3, 1),
                           "frame_err_last": int(c[1]), "tag": a.tag}
                    if mode.endswith("events"):
                        out["events"] = buf.count()
                    print(json.dumps(out), flush=True)
                    rows.append(out)
        del dec, llr, hl, buf
        torch.cuda.empty_cache()
    if env0 is not None:
        os.environ["LDPC_BS"] = env0
    os.makedirs(a.out, exist_ok=True)
    name = "wman_ucn_step" + ("_" + a.tag if a.tag else "") + ".json"
    json.dump(rows, open(os.path.join(a.out, name), "w"), indent=1)


if __name__ == "__main__":
    main()
