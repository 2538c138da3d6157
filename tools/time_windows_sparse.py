"""Times the sparse per-source posterior next to what it replaces, in one process on one GPU, arms interleaved after a
warm-up run of each:

  (a) the DESIGN section 3c window pipeline (256 windows, N = 2001, M = 64, 3 kernels x 10 partials, maxiter 10) as
      windows/s for fit only, predict=True and predict="sparse", and on the same loaded windows the sparse prediction call
      alone and predict_f alone;
  (b) one window at cfg5 size (N = 65536, M = 512, 5 sources): predict_s_sparse(X) next to predict_f(X).

Prints one JSON line.  python tools/time_windows_sparse.py [--reps 3] [--windows 256] [--skip-b]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _kernels(P, npart, w=0):
    from gpitch_amd.matern12_spectral_mixture import MercerMatern12sm
    ks = []
    for p in range(P):
        f0 = 220. * 2 ** (p * 4 / 12.)
        e = 1. / np.arange(1., npart + 1.)
        ks.append(MercerMatern12sm(1, energy=e / e.sum(), frequency=f0 * np.arange(1., npart + 1.),
                                   variance=1.0 + 0.1 * p, lengthscales=0.05 + 0.02 * p))
    return ks


def _window(N, M, P, w):
    rng = np.random.RandomState(w)
    X = np.linspace(0, (N - 1) / 16000., N).reshape(-1, 1) + 0.125 * w
    Y = np.zeros((N, 1))
    for p in range(P):
        f0 = 220. * 2 ** (p * 4 / 12.)
        Y += np.sin(2 * np.pi * f0 * X) * np.exp(-((X - X.mean()) / (0.3 * np.ptp(X))) ** 2)
    Y += 0.05 * rng.randn(N, 1)
    Z = X[np.linspace(0, N - 1, M).round().astype(int)].copy()
    return X, Y, Z


def _median(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--skip-b", action="store_true")
    a = ap.parse_args()
    import torch
    from gpitch_amd import _lib
    from gpitch_amd.sgpr_ss import SGPRSS
    from gpitch_amd.windows import SgprWindowBatch, fit_windows_batched
    out = {}
    # ---- (a) -----------------------------------------------------------------------------------------------------------
    N, M, P, W = 2001, 64, 3, a.windows
    wins = [_window(N, M, P, w) for w in range(W)]

    def make(handle):
        m = SGPRSS(wins[0][0], wins[0][1], np.sum(_kernels(P, 10)), wins[0][2], handle=handle)
        return m

    arms = [("fit", False), ("fit_predict", True), ("fit_sparse", "sparse")]
    for _, pr in arms:                                    # warm-up: plans, graphs, allocator
        fit_windows_batched(make, wins[:min(W, 64)], maxiter=2, batch=min(W, 64), predict=pr)
    t = {k: [] for k, _ in arms}
    for _ in range(a.reps):
        for k, pr in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit_windows_batched(make, wins, maxiter=10, batch=W, predict=pr)
            torch.cuda.synchronize()
            t[k].append(time.perf_counter() - t0)
    for k, _ in arms:
        out["a_%s_windows_per_s" % k] = W / _median(t[k])
    h = _lib.default_handle()
    tmpl = make(h)
    dev = SgprWindowBatch(tmpl, W, N, M, handle=h)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    tmpl._compile()
    tmpl._pack()
    pv = np.tile(tmpl._params.cpu().numpy(), (W, 1))
    calls = [("predict_f", dev.predict_f), ("predict_s_sparse", dev.predict_s_sparse)]
    for _, f in calls:
        f(pv)
    t = {k: [] for k, _ in calls}
    for _ in range(max(a.reps, 5)):
        for k, f in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(pv)
            torch.cuda.synchronize()
            t[k].append(time.perf_counter() - t0)
    for k, _ in calls:
        out["a_%s_ms_per_batch" % k] = 1e3 * _median(t[k])
    dev.close()
    tmpl._destroy()
    # ---- (b) -----------------------------------------------------------------------------------------------------------
    if not a.skip_b:
        N, M, P = 65536, 512, 5
        X, Y, Z = _window(N, M, P, 1)
        m = SGPRSS(X, Y, np.sum(_kernels(P, 10)), Z, handle=h)
        calls = [("predict_f", m.predict_f), ("predict_s_sparse", m.predict_s_sparse)]
        for _, f in calls:
            f(X)
        t = {k: [] for k, _ in calls}
        for _ in range(max(a.reps, 5)):
            for k, f in calls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(X)
                torch.cuda.synchronize()
                t[k].append(time.perf_counter() - t0)
        for k, _ in calls:
            out["b_%s_ms" % k] = 1e3 * _median(t[k])
        m._destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
