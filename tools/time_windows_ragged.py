"""Window fits with the drivers' own inducing inputs: 512 windows of 2001 frames cut from synthetic audio
(per_fun notes whose pitch and loudness change from window to window, plus noise), each window's Z from init_liv with
the transcription driver's decimation (dec = 3, transcription.py:229-238), so M differs per window.  Reports windows/s of
  ragged   fit_windows_batched on these windows (sorted by M, plans sized per batch)
  uniform  the same windows with every Z cut to the smallest count (one plan, uniform M: the path before ragged M)
  streams  fit_windows on eight HIP streams (the one-window engine)
Every step runs in a child process under a time limit of its own; the parent prints one JSON line per step and a
summary line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 16000.
WS = 2001


def make_windows(nwin, dec=3, seed=0, noise=0.02):
    from gpitch_amd import synth, window_overlap
    from gpitch_amd.init_models import init_liv
    rng = np.random.RandomState(seed)
    hop = (WS - 1) // 2
    n = hop * (nwin + 1) + 1
    x = np.linspace(0, (n - 1) / FS, n).reshape(-1, 1)
    y = np.zeros_like(x)
    for w in range(nwin + 1):
        f0 = 110. * 2 ** (rng.randint(0, 30) / 12.)
        seg = slice(w * hop, min(n, (w + 1) * hop + 1))
        y[seg] += (0.2 + rng.rand()) * synth.per_fun(x[seg], 3, f0)
    y += noise * rng.randn(*y.shape)
    xs, ys = window_overlap.windowed(x, y, WS)
    zs = [np.asarray(init_liv(a, b, dec=dec)[0][1][0]) for a, b in zip(xs, ys)]
    return list(zip(xs, ys, zs))


def make_model_fn(data, P, m):
    def make(h):
        from gpitch_amd.kernels import Add
        from gpitch_amd.matern12_spectral_mixture import MercerMatern12sm
        from gpitch_amd.sgpr_ss import SGPRSS
        ks = [MercerMatern12sm(1, energy=np.ones(m) / m, frequency=110. * 2 ** (4 * p / 12.) * np.arange(1, m + 1),
                               variance=1.0, lengthscales=0.05) for p in range(P)]
        return SGPRSS(data[0][0], data[0][1], Add(ks), data[0][2], handle=h)
    return make


def run_step(args):
    import torch
    data = make_windows(args.nwin)
    counts = np.array([w[2].shape[0] for w in data])
    if args.step == "uniform":
        mmin = int(counts.min())
        data = [(x, y, z[:mmin]) for x, y, z in data]
    make = make_model_fn(data, args.P, args.m)
    from gpitch_amd.windows import fit_windows, fit_windows_batched, ragged_batches
    if args.step == "streams":
        fit_windows(make, data[:8], maxiter=2, num_streams=8)                        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fit_windows(make, data, maxiter=args.maxiter, num_streams=8)
    else:
        fit_windows_batched(make, data[:args.batch], maxiter=2, batch=args.batch)     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fit_windows_batched(make, data, maxiter=args.maxiter, batch=args.batch)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    used = np.array([w[2].shape[0] for w in data])
    groups, single = ragged_batches(used, args.batch)
    out = {"step": args.step, "windows": len(data), "seconds": dt, "windows_per_s": len(data) / dt,
           "mean_M": float(used.mean()), "min_M": int(used.min()), "max_M": int(used.max()),
           "plans": sorted({m for m, _ in groups}), "single": len(single),
           "nfev_per_window": float(np.mean([r["nfev"] for r in res])),
           "failed": sum(1 for r in res if "error" in r)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["ragged", "uniform", "streams"], default=None, help="(child) run one step")
    ap.add_argument("--nwin", type=int, default=512)
    ap.add_argument("--P", type=int, default=3)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--maxiter", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    data = make_windows(args.nwin)
    counts = np.array([w[2].shape[0] for w in data])
    edges = np.arange(0, max(counts.max(), 16) + 17, 16)
    hist, _ = np.histogram(counts, bins=edges)
    print("M histogram (init_liv, dec=3; %d windows of %d frames): mean %.1f, min %d, max %d"
          % (len(counts), WS, counts.mean(), counts.min(), counts.max()))
    for lo, c in zip(edges[:-1], hist):
        if c:
            print("  M %3d-%3d: %4d %s" % (lo + 1, lo + 16, c, "#" * int(np.ceil(60.0 * c / hist.max()))))
    rates = {}
    for step in ("ragged", "uniform", "streams"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + \
              ["--%s=%s" % (k, getattr(args, k)) for k in ("nwin", "P", "m", "maxiter", "batch")]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("step %s: over its %d s limit; stopping" % (step, args.limit))
            return 1
        if p.returncode != 0:
            sys.stdout.write(p.stdout[-2000:] + p.stderr[-4000:])
            print("step %s: exit %d; stopping" % (step, p.returncode))
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line)
        rates[step] = json.loads(line)
    r, u, s = rates["ragged"], rates["uniform"], rates["streams"]
    scaled = u["windows_per_s"] * u["mean_M"] / r["mean_M"]
    print(json.dumps({"ragged_windows_per_s": r["windows_per_s"], "uniform_windows_per_s": u["windows_per_s"],
                      "uniform_scaled_to_mean_M": scaled, "ragged_over_scaled_uniform": r["windows_per_s"] / scaled,
                      "streams_windows_per_s": s["windows_per_s"],
                      "ragged_over_streams": r["windows_per_s"] / s["windows_per_s"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
