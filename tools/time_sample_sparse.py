"""Times the joint posterior draws of the SGPRSS sources (sample_s_sparse, S = 16) beside predict_s_sparse on the same
windows, and beside the route to draws there was before: build_predict_source(Xnew, full_cov=True) plus a host Cholesky of
each source's n x n covariance.  Reports, asserts nothing.  Sizes:

  one      one window, N = 2001, M = 64, 3 kernels x 10 partials, drawn at its own frames
  batch    256 such windows on one SgprWindowBatch
  cfg5     one window at cfg5 size, N = 65536, M = 512, 5 sources (the full-covariance route does not fit there: 5 matrices
           of 34 GB)

Each size runs in a child process of its own under its own time limit; a size that fails or runs out of time ends the run.
Prints one JSON line per size.  python tools/time_sample_sparse.py [--reps 5] [--sizes one,batch,cfg5]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"one": 180, "batch": 300, "cfg5": 300}          # seconds per size
S = 16


def _kernels(P, npart):
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


def _time(calls, reps):
    """median wall time in ms of each call, arms interleaved after one warm-up run of each"""
    import torch
    for _, f in calls:
        f()
    t = {k: [] for k, _ in calls}
    for _ in range(reps):
        for k, f in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t[k].append(time.perf_counter() - t0)
    return {k + "_ms": 1e3 * float(np.median(v)) for k, v in t.items()}


def _full_cov_route(m, X):
    """draws the way they could be had before: P exact n x n covariances, then a Cholesky of each on the host"""
    mean, cov = m.build_predict_source(X, full_cov=True)
    n = X.shape[0]
    rng = np.random.RandomState(0)
    for p in range(len(cov)):
        L = np.linalg.cholesky(cov[p][:, :, 0] + 1e-6 * np.eye(n))
        L.dot(rng.randn(n, S))


def step(size, reps):
    from gpitch_amd import _lib
    from gpitch_amd.sgpr_ss import SGPRSS
    from gpitch_amd.windows import SgprWindowBatch
    h = _lib.default_handle()
    out = {"size": size, "S": S}
    if size in ("one", "cfg5"):
        N, M, P = (2001, 64, 3) if size == "one" else (65536, 512, 5)
        X, Y, Z = _window(N, M, P, 1)
        m = SGPRSS(X, Y, np.sum(_kernels(P, 10)), Z, handle=h)
        calls = [("predict_s_sparse", lambda: m.predict_s_sparse(X)),
                 ("sample_s_sparse", lambda: m.sample_s_sparse(X, num_samples=S, seed=0))]
        out.update(_time(calls, reps))
        if size == "one":
            try:
                out.update(_time([("full_cov_and_host_cholesky", lambda: _full_cov_route(m, X))], max(1, reps // 2)))
            except np.linalg.LinAlgError as e:
                out["full_cov_and_host_cholesky_ms"] = None
                out["full_cov_note"] = "host Cholesky failed: %s" % e
        m._destroy()
    else:
        N, M, P, W = 2001, 64, 3, 256
        wins = [_window(N, M, P, w) for w in range(W)]
        tmpl = SGPRSS(wins[0][0], wins[0][1], np.sum(_kernels(P, 10)), wins[0][2], handle=h)
        dev = SgprWindowBatch(tmpl, W, N, M, handle=h)
        dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
        tmpl._compile()
        tmpl._pack()
        pv = np.tile(tmpl._params.cpu().numpy(), (W, 1))
        calls = [("predict_s_sparse", lambda: dev.predict_s_sparse(pv)),
                 ("sample_s_sparse", lambda: dev.sample_s_sparse(pv, num_samples=S, seed=0))]
        out["windows"] = W
        out.update(_time(calls, reps))
        dev.close()
        tmpl._destroy()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="one,batch,cfg5")
    ap.add_argument("--step", default=None, help="(internal) run one size in this process")
    a = ap.parse_args()
    if a.step:
        step(a.step, a.reps)
        return
    for size in a.sizes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", size, "--reps", str(a.reps)], cwd=ROOT,
                               timeout=LIMITS[size])
        except subprocess.TimeoutExpired:
            print(json.dumps({"size": size, "error": "ran past its %d s" % LIMITS[size]}))
            return
        if r.returncode != 0:
            print(json.dumps({"size": size, "error": "exit status %d" % r.returncode}))
            return


if __name__ == "__main__":
    main()
