"""Times the joint posterior draws of the Pdgp sources (Pdgp.sample_sources, S = 16) beside predict_sources at the same
inputs and, where it fits (n = 2000), beside the route to draws there was before: conditional(..., full_cov=True) of every
latent GP plus a host Cholesky of its n x n covariance.  Reports, asserts nothing.  Sizes:

  demo     the demo model: N = n = 16000 frames, M = 76, P = 1, Matern32 activation, MercerMatern12sm of 5 partials
  demo2k   the same model drawn at n = 2000 of its frames, with the full-covariance route
  p12      12 pitches, M = 256 for every latent GP, 5 partials, n = 16000

Each size runs in a child process of its own under its own time limit; a size that fails or runs out of time ends the run.
Prints one JSON line per size.  python tools/time_pdgp_sample.py [--reps 5] [--sizes demo,demo2k,p12]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"demo": 240, "demo2k": 240, "p12": 300}          # seconds per size
S = 16


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


def _full_cov_route(m, x):
    """draws the way they could be had before: 2P full n x n conditionals, then a Cholesky of each on the host"""
    from gpitch_amd.conditionals import conditional
    from gpitch_amd.flatvec import latent_gps
    n = x.shape[0]
    rng = np.random.RandomState(0)
    for kern, z, q_mu, q_sqrt in latent_gps(m):
        mean, cov = conditional(x, z.value, kern, q_mu.value, full_cov=True, q_sqrt=q_sqrt.value, whiten=m.whiten)
        L = np.linalg.cholesky(cov[:, :, 0] + 1e-6 * np.eye(n))
        mean + L.dot(rng.randn(n, S))


def step(size, reps):
    from gpitch_amd import _lib
    from gpitch_amd.synth import make_problem, pdgp_from_problem
    h = _lib.default_handle()
    N, M, P = (16000, 256, 12) if size == "p12" else (16000, 76, 1)
    prob = make_problem(N, M, P, num_partials=5, seed=0)
    m = pdgp_from_problem(prob, handle=h)
    x = prob["x"] if size != "demo2k" else prob["x"][::8].copy()
    out = {"size": size, "S": S, "n": int(x.shape[0]), "M": M, "P": P}
    calls = [("predict_sources", lambda: m.predict_sources(x)),
             ("sample_sources", lambda: m.sample_sources(x, num_samples=S, seed=0))]
    out.update(_time(calls, reps))
    if size == "demo2k":
        try:
            out.update(_time([("full_cov_and_host_cholesky", lambda: _full_cov_route(m, x))], max(1, reps // 2)))
        except np.linalg.LinAlgError as e:
            out["full_cov_and_host_cholesky_ms"] = None
            out["full_cov_note"] = "host Cholesky failed: %s" % e
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="demo,demo2k,p12")
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
