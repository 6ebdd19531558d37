#!/usr/bin/env python3
"""Sweep step of the three early-stop modes at B = 2^20 on one GPU, in-kernel channel (DESIGN.md
3.10, profiles/events/): ``decode_awgn(early_stop=True)`` alone (``es``), with the decoded word of
every frame (``es_word``, 3.9) and with the events collected on the device (``es_events``, 3.10);
per point the five timings of each mode and their median, one JSON line each and
``<out>/events_step.json``.

  python tools/events_step.py [out_dir] [--points CONFIG:SNR,SNR,... ...] [--batch B]
                              [--modes es,es_word,es_events] [--cap K] [--tree DIR]

  out_dir   default bench_out/, which git ignores
  --points  the configs (bench.py's) and their SNRs in dB; default C2:5.0 C3:6.0 C5:14.5,3.0
  --tree    import the package and bench.py of another checkout (a built parent commit, for an
            alternating A/B); modes that checkout does not have are skipped
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--points", nargs="+", default=["C2:5.0", "C3:6.0", "C5:14.5,3.0"], metavar="CONFIG:SNRS")
    ap.add_argument("--batch", type=int, default=1 << 20, help="codewords per decode")
    ap.add_argument("--modes", default="es,es_word,es_events")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--cap", type=int, default=1 << 16, help="events the buffer holds (more are counted only)")
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    a = ap.parse_args(argv)
    pts = []
    for p in a.points:
        config, _, snrs = p.partition(":")
        try:
            pts.append((config, [float(x) for x in snrs.split(",")]))
        except ValueError:
            ap.error(f"--points {p!r}: expected CONFIG:SNR,SNR,...")
    a.points = pts
    a.modes = [m for m in a.modes.split(",") if m]
    return a


def main(argv=None):
    a = parse(argv)
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np, torch
    import bench
    from ldpc_error_floor_amd.decoder import NMSDecoder
    B = a.batch
    dev = torch.device("cuda", 0)
    rows = []
    for config, snrs in a.points:
        cfg = bench.CONFIGS[config]
        proto, g, W, cp = bench.load_problem(config=config)
        dec = NMSDecoder(proto, cfg["z"], W, 2, 5, device=dev, B_max=B)
        dec.punct, dec.short = cfg.get("punct", (0, 0)), cfg.get("short", (0, 0))
        assert dec.supports_early_stop(), config
        modes = [m for m in a.modes if m != "es_events" or hasattr(dec, "supports_events")]
        hl = buf = None
        if "es_word" in modes:
            hl = torch.empty((B, (dec.n_vars + 31) // 32), dtype=torch.int32, device=dev)
        if "es_events" in modes:
            from ldpc_error_floor_amd.events import EventBuffer
            buf = EventBuffer(dec, a.cap)
        for snr in snrs:
            sigma = float(cp.sigma(snr))

            def run(mode, seed=11):
                cnt = torch.zeros(4, dtype=torch.int64, device=dev)
                kw = {"es": {}, "es_word": dict(hard_last=hl, word_flags=True), "es_events": dict(events=buf)}[mode]
                if buf is not None:
                    buf.reset()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = dec.decode_awgn(B, sigma, seed, counters=cnt, early_stop=True, iter_hist=True, n_iter=True, **kw)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), r

            out = {"config": config, "T": dec.T, "snr_db": snr, "B": B, "tag": a.tag}
            ref = None
            for mode in modes:
                for w in range(2):
                    run(mode)
                ts = []
                for k in range(5):
                    t, r = run(mode)
                    ts.append(t)
                out[mode + "_ms"] = [round(x, 3) for x in ts]
                out[mode + "_ms_median"] = round(float(np.median(ts)), 3)
                out[mode + "_kernel"] = dec.last_kernel()
                c = r.counters.cpu().numpy()
                if ref is None:
                    ref = c
                    out["frame_err_last"] = int(c[1])
                    h = r.iter_hist.cpu().numpy().astype(np.float64)
                    out["mean_iter"] = round(float((h * np.arange(1, h.size + 1)).sum() / h.sum()), 3)
                assert np.array_equal(c, ref), "the modes' counters differ"
                if mode == "es_word":
                    out["es_word_nonzero_rows"] = int((hl != 0).any(dim=1).sum().item())
                if mode == "es_events":
                    out["events"] = buf.count()
                    out["events_cap"] = buf.cap
                    tab = buf.table(allow_overflow=True)
                    out["events_ab_classes"] = len(tab.ab_histogram())
                    out["events_undetected"] = int(tab.undetected().sum())
                    assert int((tab.a_target > 0).sum()) == int(c[1]) or buf.count() > buf.cap
            print(json.dumps(out), flush=True)
            rows.append(out)
        del dec, hl, buf
    os.makedirs(a.out, exist_ok=True)
    name = "events_step" + ("_" + a.tag if a.tag else "") + ".json"
    json.dump(rows, open(os.path.join(a.out, name), "w"), indent=1)


if __name__ == "__main__":
    main()
