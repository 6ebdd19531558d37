#!/usr/bin/env python3
"""The floor events of one SNR point on one GPU: decode ``--n`` codewords of the
point's Philox stream, collect on the device every frame whose decoded word is nonzero, print the
(a, b) table -- a: wrong bits of the word, b: unsatisfied checks; b = 0 is an undetected error --
and write the events (frame index, iterations, a, a_target, b, the packed words) as npz.

  python tools/floor_events.py --config C2|C3|C4|C5 --snr DB --n N [--batch B] [--seed S]
                               [--begin I --end J] [--full-t] [--cap K] [--no-words] [--out FILE]
                               [--weights FILE --sharing a,b,c [--T n]]

  --config   one of bench.py's configs, with its weights, puncturing and shortening
  --full-t   the last iteration's word instead of the early-stop decode's word at the stop
             iteration: ``awgn()`` + ``decode()`` (the in-kernel channel has no full-T word build);
             the only mode of C4, which has no early-stop build
  --weights  a trained-weight file decoded with --sharing (and --T iterations, default the file's
             rows) instead of the config's weights; graph, lifting, puncturing and shortening stay
             the config's.  A trained cascade (base and post decoder as one graph, sharing 3,3,3 or
             2,2,2 with alpha' != alpha) on C2 runs bsl[...,ucn]; its full-T events need --full-t
  --begin/--end  a sub-range [I, J) of the N codewords; the npz files of a partition concatenate
             (``FloorEvents.concat``) to the file of the whole range
  --out      default bench_out/floor_events_<config>_<snr>dB.npz (bench_out/ is git-ignored)
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--snr", type=float, required=True, help="dB")
    ap.add_argument("--n", type=int, default=1 << 24, help="codewords of the point")
    ap.add_argument("--batch", type=int, default=1 << 20, help="codewords per decode")
    ap.add_argument("--seed", type=int, default=1076)
    ap.add_argument("--begin", type=int, default=None)
    ap.add_argument("--end", type=int, default=None)
    ap.add_argument("--full-t", action="store_true")
    ap.add_argument("--cap", type=int, default=1 << 16, help="events the device buffer holds")
    ap.add_argument("--no-words", action="store_true", help="keep the weights only, not the words")
    ap.add_argument("--out", default=None)
    ap.add_argument("--weights", default=None, help="a trained-weight file instead of the config's weights")
    ap.add_argument("--sharing", default=None, help="a,b,c: the sharing the file is decoded with")
    ap.add_argument("--T", type=int, default=None, help="iterations (default: the file's rows)")
    a = ap.parse_args(argv)
    if (a.weights is None) != (a.sharing is None) or (a.T is not None and a.weights is None):
        ap.error("--weights FILE --sharing a,b,c [--T n] go together")
    return a


def main(argv=None):
    a = parse(argv)
    import torch
    import bench
    from ldpc_error_floor_amd.decoder import NMSDecoder
    from ldpc_error_floor_amd.events import floor_events
    if a.config not in bench.CONFIGS:
        raise SystemExit(f"unknown config {a.config!r}: one of {sorted(bench.CONFIGS)}")
    cfg = bench.CONFIGS[a.config]
    proto, g, W, cp = bench.load_problem(config=a.config)
    if a.weights:
        from ldpc_error_floor_amd.weights import weights_from_file
        W = weights_from_file(a.weights, a.sharing.split(","), g, a.T)
    dev = torch.device("cuda", 0)
    batch = min(a.batch, a.n)
    dec = NMSDecoder(proto, cfg["z"], W, 2, 5, device=dev, B_max=batch)
    dec.punct, dec.short = cfg.get("punct", (0, 0)), cfg.get("short", (0, 0))
    es = not a.full_t
    if not dec.supports_events(early_stop=es):
        raise SystemExit(f"{a.config}: events are not served " +
                         ("with early stop (try --full-t)" if es and dec.supports_events() else "for this decoder"))
    t0 = time.time()
    try:
        c, tab = floor_events(dec, float(cp.sigma(a.snr)), a.n, batch, a.seed, early_stop=es, begin=a.begin,
                              end=a.end, cap=a.cap, words=not a.no_words)
    except OverflowError as e:
        raise SystemExit(f"{e}\nthis is no floor point for --cap {a.cap}: raise --cap, lower --n or raise --snr")
    dt = time.time() - t0
    out = a.out or os.path.join(ROOT, "bench_out", f"floor_events_{a.config}_{a.snr:g}dB.npz")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    tab.save(out)
    print(f"{a.config} ({cfg['label']}) at {a.snr:g} dB, T = {dec.T}, {'early stop' if es else 'full T'}, "
          f"kernel {dec.last_kernel()}: {c.frames} frames in {dt:.1f} s")
    print(f"bit errors {c.bit_err_last}, frame errors {c.frame_err_last} (FER {c.fer_last:.3e})" +
          (f", mean iterations {c.mean_iterations:.2f}" if c.iter_hist is not None else ""))
    print(tab.format())
    print(json.dumps({"config": a.config, "snr_db": a.snr, "frames": c.frames, "early_stop": es,
                      "events": len(tab), "undetected": int(tab.undetected().sum()),
                      "frame_err_last": c.frame_err_last,
                      "ab": [[k[0], k[1], n] for k, n in tab.ab_histogram().items()], "npz": out}))


if __name__ == "__main__":
    main()
