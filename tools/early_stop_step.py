#!/usr/bin/env python3
"""Sweep step ``decode_awgn(early_stop=True)`` against ``decode_awgn`` at B = 2^20 on one GPU
(profiles/early_stop/): per point the five timings of each mode, the mean and the
pack-maximum iterations, the histogram and both modes' frame errors, one JSON line each and
``<out>/sweep_step.json``.

  python tools/early_stop_step.py [out_dir] [--points CONFIG:SNR,SNR,... ...] [--batch B] [--word]

  out_dir   default bench_out/, which git ignores
  --points  the configs (bench.py's) and their SNRs in dB; default C2:3.5,5.0,6.5 C3:4.5,6.0;
            C5 alone: --points C5:3.0,8.0,14.5
  --word    also time the early-stop decode that returns each frame's word at its stop iteration
            (``decode_awgn(early_stop=True, hard_last=..., word_flags=True)``, DESIGN.md 3.9:
            ``es_word_*``) and the full-T word mode on the same channel's LLRs resident in HBM
            (``decode(llr, hard_last=...)``, 3.8: ``word_full_*``), and check the early-stop
            outputs of the two early-stop modes against each other
  --q8      instead of the sweep step: the early-stop step on a resident int8 batch
            (``decode_q8(awgn_q8(...), early_stop=True)``) against the float step
            on the same codewords resident as float LLRs (``decode(awgn(...), early_stop=True)``),
            for the early-stop, stop-iteration-word and events steps: float and int8 alternated
            in one warmed process, five timings of each, their medians and the ratio int8 / float
            (``q8_<step>_*``), with the outputs of the two checked against each other
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--points", nargs="+", default=["C2:3.5,5.0,6.5", "C3:4.5,6.0"], metavar="CONFIG:SNRS")
    ap.add_argument("--batch", type=int, default=1 << 20, help="codewords per decode")
    ap.add_argument("--word", action="store_true", help="also time the two decoded-word modes")
    ap.add_argument("--q8", action="store_true", help="time the early-stop steps on int8 LLRs against float LLRs")
    a = ap.parse_args(argv)
    pts = []
    for p in a.points:
        config, _, snrs = p.partition(":")
        try:
            pts.append((config, [float(x) for x in snrs.split(",")]))
        except ValueError:
            ap.error(f"--points {p!r}: expected CONFIG:SNR,SNR,...")
    a.points = pts
    return a


def q8_point(dec, B, sigma, out, warm=6, n=5):
    """The --q8 timings of one point into ``out``: resident float and int8 batches of the same
    codewords; per step ``warm`` untimed pairs, then ``n`` timed pairs float, int8, float, ..."""
    import numpy as np, torch
    from ldpc_error_floor_amd.events import EventBuffer
    dev = dec.device
    assert dec.supports_q8(early_stop=True, has_short=dec.short[0] > 0)
    llr = dec.awgn(B, sigma, 11)
    q8 = dec.awgn_q8(B, sigma, 11)
    hl = torch.empty((B, (dec.n_vars + 31) // 32), dtype=torch.int32, device=dev)
    buf = EventBuffer(dec, 4096)
    steps = {"es": {}, "es_word": dict(hard_last=hl, word_flags=True), "es_events": dict(events=buf)}
    out["q8_bytes_per_cw"] = [4 * dec.n_vars, dec.n_vars]

    def run(int8, kw):
        cnt = torch.zeros(4, dtype=torch.int64, device=dev)
        buf.reset()
        kw = dict(kw, counters=cnt, early_stop=True, iter_hist=True, n_iter=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = dec.decode_q8(q8, on_invalid="mark", **kw) if int8 else dec.decode(llr, on_off_grid="mark", **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    for tag, kw in steps.items():
        for w in range(warm):
            run(False, kw), run(True, kw)
        ts = {False: [], True: []}
        for k in range(n):
            for int8 in (False, True):
                t, r = run(int8, kw)
                ts[int8].append(t)
                name = dec.last_kernel()
                res = [r.counters.clone(), r.n_iter, r.iter_hist, buf.count() if "events" in kw else 0]
                if int8:
                    assert name == fname + "+q8", (name, fname)
                    same = all(torch.equal(x, y) for x, y in zip(res[:3], fres[:3])) and res[3] == fres[3]
                    if "hard_last" in kw:
                        same = same and torch.equal(hl, fhl) and torch.equal(r.word_flags, fwf)
                    assert same, f"{tag}: the int8 step's outputs differ from the float step's"
                else:
                    fname, fres = name, res
                    if "hard_last" in kw:
                        fhl, fwf = hl.clone(), r.word_flags.clone()
        fm, qm = float(np.median(ts[False])), float(np.median(ts[True]))
        out[f"q8_{tag}_float_ms"] = [round(x, 3) for x in ts[False]]
        out[f"q8_{tag}_int8_ms"] = [round(x, 3) for x in ts[True]]
        out[f"q8_{tag}_float_ms_median"], out[f"q8_{tag}_int8_ms_median"] = round(fm, 3), round(qm, 3)
        out[f"q8_{tag}_ratio"] = round(qm / fm, 4)
        out[f"q8_{tag}_kernel"] = name
        if "events" in kw:
            out["q8_es_events_count"] = res[3]
    out["q8_frame_err"] = int(fres[0][1].item())
    out["q8_mean_iter"] = round(float((fres[2].double() * torch.arange(1, fres[2].numel() + 1, device=dev)).sum() / B), 3)


def main(argv=None):
    a = parse(argv)
    import numpy as np, torch
    import bench
    from ldpc_error_floor_amd.decoder import NMSDecoder
    for config, _ in a.points:
        if config not in bench.CONFIGS:
            raise SystemExit(f"unknown config {config!r}: one of {sorted(bench.CONFIGS)}")
    B = a.batch
    dev = torch.device("cuda", 0)
    rows = []
    for config, snrs in a.points:
        cfg = bench.CONFIGS[config]
        proto, g, W, cp = bench.load_problem(config=config)
        dec = NMSDecoder(proto, cfg["z"], W, 2, 5, device=dev, B_max=B)
        dec.punct, dec.short = cfg.get("punct", (0, 0)), cfg.get("short", (0, 0))
        assert dec.supports_early_stop(), config
        for snr in snrs:
            sigma = float(cp.sigma(snr))
            def run(es, seed):
                cnt = torch.zeros(4, dtype=torch.int64, device=dev)
                kw = dict(early_stop=True, iter_hist=True, n_iter=True) if es else {}
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = dec.decode_awgn(B, sigma, seed, counters=cnt, **kw)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), r
            out = {"config": config, "T": dec.T, "snr_db": snr}
            if a.q8:
                q8_point(dec, B, sigma, out)
                print(json.dumps(out), flush=True)
                rows.append(out)
                continue
            for es in (False, True):
                for w in range(2):
                    run(es, 11)
                ts = []
                for k in range(5):
                    t, r = run(es, 11)
                    ts.append(t)
                tag = "es" if es else "full"
                out[tag + "_ms"] = [round(x, 3) for x in ts]
                out[tag + "_ms_median"] = round(float(np.median(ts)), 3)
                out[tag + "_kernel"] = dec.last_kernel()
                c = r.counters.cpu().numpy()
                out[tag + "_frame_err_last"] = int(c[1]); out[tag + "_frames"] = B
                if es:
                    h = r.iter_hist.cpu().numpy().astype(np.float64)
                    ni = r.n_iter.cpu().numpy().astype(np.int64)
                    out["mean_iter"] = round(float((h * np.arange(1, h.size + 1)).sum() / h.sum()), 3)
                    pm = np.pad(ni, (0, -ni.size % 32)).reshape(-1, 32).max(axis=1)
                    out["pack_max_mean"] = round(float(pm.mean()), 3)
                    out["pack_max_max"] = int(pm.max())
                    out["iter_hist"] = [int(x) for x in h]
            if a.word:
                assert dec.supports_hard_last(early_stop=True), config
                hl = torch.empty((B, (dec.n_vars + 31) // 32), dtype=torch.int32, device=dev)
                llr = dec.awgn(B, sigma, 11)

                def run_word(es, seed=11):
                    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if es:
                        r = dec.decode_awgn(B, sigma, seed, counters=cnt, early_stop=True, iter_hist=True,
                                            n_iter=True, hard_last=hl, word_flags=True)
                    else:
                        r = dec.decode(llr, counters=cnt, hard_last=hl, word_flags=True, on_off_grid="mark")
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1), r
                for es in (True, False):
                    for w in range(2):
                        run_word(es)
                    ts = []
                    for k in range(5):
                        t, rw = run_word(es)
                        ts.append(t)
                    tag = "es_word" if es else "word_full"
                    out[tag + "_ms"] = [round(x, 3) for x in ts]
                    out[tag + "_ms_median"] = round(float(np.median(ts)), 3)
                    out[tag + "_kernel"] = dec.last_kernel()
                    out[tag + "_not_codeword"] = int((rw.word_flags & 1).sum().item())
                    if es:      # (r: the early-stop decode of the same seed, above)
                        same = all(torch.equal(getattr(rw, k), getattr(r, k)) for k in ("counters", "n_iter", "iter_hist"))
                        out["es_word_equals_es"] = bool(same)
                        assert same, "the early-stop outputs of the two early-stop modes differ"
                        out["es_word_nonzero_rows"] = int((hl != 0).any(dim=1).sum().item())
                del llr, hl
            print(json.dumps(out), flush=True)
            rows.append(out)
    os.makedirs(a.out, exist_ok=True)
    json.dump(rows, open(os.path.join(a.out, "sweep_step.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
