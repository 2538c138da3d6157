"""Times the state-space smoother (predict_s_ssm) next to the two per-source posteriors it sits beside, in one process on one
GPU: a warm-up call of each arm, then `--reps` timed calls with the arms interleaved; medians with the smallest and largest run.

  one    one window, N = n = 2001, M = 64, 3 sources x 10 partials (d = 60): predict_s, predict_s_sparse, predict_s_ssm and
         exact_log_likelihood (the forward walk alone)
  batch  256 such windows through SgprWindowBatch, the same three
  fit    fit_windows_batched (maxiter 10) with predict=True, "sparse" and "ssm", as windows/s
  score  the exact likelihood's gradient: exact_log_likelihood_and_grad of the one window beside exact_log_likelihood
         and predict_s_ssm at Xnew = X; SgprWindowBatch.exact_loglik_grad of the 256 windows beside its forward walk alone and
         predict_s_ssm; fit_windows_exact (maxiter 10) beside fit_windows_batched as windows/s, with the mean exact
         log-likelihood per window that each fit reaches
  cfg5   one window of N = 65536, 5 sources x 10 partials (d = 100), Xnew = X: predict_s_ssm next to predict_s_sparse (M = 512).
         predict_s cannot run there (one N x N float64 matrix is 34 GB) and is recorded as such.
  sample joint draws from the exact posterior: sample_s_ssm at S = 1 and 16 (seeded: the normals' generation and
         the download of the draws are inside the figure) of the one window and of the 256, beside the gain walk alone
         (exact_log_likelihood), predict_s_ssm and sample_s_sparse (M = 64); then 16 draws of the N = 65536, d = 100 window with
         the call's workspace beside predict_s_ssm's

Writes one JSON file (default profiles/ssm/ssm_smooth_time.json; profiles/ssm/ssm_sample_time.json for --parts sample) and prints it.  GPITCH_AMD_SWITCHES=ssm_wide=1 times the
two-wavefront walks at d = 60 (the switch is read once per process; it is recorded in the output).
python tools/time_ssm_smooth.py [--parts one,batch,fit,cfg5,score,sample] [--reps 5] [--windows 256] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def _data_only(model, x, y, z):
    """a `reset` for fit_windows_batched that keeps the template's parameter values (what fit_windows_exact starts from)"""
    model.X = x
    model.Y = y
    model.Z = z


def _time(arms, reps, sync):
    """{name: {"median_ms", "min_ms", "max_ms", "runs"}} of callables, interleaved after one warm-up call of each"""
    for _, f in arms:
        f()
    t = {k: [] for k, _ in arms}
    for _ in range(reps):
        for k, f in arms:
            sync()
            t0 = time.perf_counter()
            f()
            sync()
            t[k].append(1e3 * (time.perf_counter() - t0))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "runs": len(v)}
            for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="one,batch,fit,cfg5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parts = a.parts.split(",")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "ssm", "ssm_sample_time.json" if parts == ["sample"] else "ssm_smooth_time.json")
    import torch
    from gpitch_amd import _lib
    from gpitch_amd.sgpr_ss import SGPRSS
    from gpitch_amd.windows import SgprWindowBatch, fit_windows_batched
    sync = torch.cuda.synchronize
    h = _lib.default_handle()
    out = {"device": torch.cuda.get_device_name(0), "switches": os.environ.get("GPITCH_AMD_SWITCHES", ""), "reps": a.reps}
    N, M, P, W = 2001, 64, 3, a.windows
    wins = [_window(N, M, P, w) for w in range(W if ("batch" in parts or "fit" in parts or "score" in parts or "sample" in parts) else 1)]

    def make(handle):
        return SGPRSS(wins[0][0], wins[0][1], np.sum(_kernels(P, 10)), wins[0][2], handle=handle)

    if "one" in parts:
        m = make(h)
        X = wins[0][0]
        out["one_window_N2001_d60"] = _time([("predict_s", lambda: m.predict_s(X)), ("predict_s_sparse", lambda: m.predict_s_sparse(X)),
                                             ("predict_s_ssm", lambda: m.predict_s_ssm(X)),
                                             ("exact_log_likelihood", lambda: m.exact_log_likelihood())], a.reps, sync)
        m._destroy()
        print("one window: done", file=sys.stderr, flush=True)
    if "batch" in parts:
        tmpl = make(h)
        dev = SgprWindowBatch(tmpl, W, N, M, handle=h)
        dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
        tmpl._compile()
        tmpl._pack()
        pv = np.tile(tmpl._params.cpu().numpy(), (W, 1))
        res = _time([("predict_s", lambda: dev.predict_s(pv)), ("predict_s_sparse", lambda: dev.predict_s_sparse(pv)),
                     ("predict_s_ssm", lambda: dev.predict_s_ssm(pv))], a.reps, sync)
        for v in res.values():
            v["windows_per_s"] = W / (1e-3 * v["median_ms"])
        out["batch_%d_windows_N2001_d60" % W] = res
        dev.close()
        tmpl._destroy()
        print("batch: done", file=sys.stderr, flush=True)
    if "fit" in parts:
        arms = [("predict_True", True), ("predict_sparse", "sparse"), ("predict_ssm", "ssm"), ("fit_only", False)]
        res = _time([(k, (lambda pr=pr: fit_windows_batched(make, wins, maxiter=10, batch=W, predict=pr))) for k, pr in arms],
                    max(3, a.reps // 2), sync)
        for v in res.values():
            v["windows_per_s"] = W / (1e-3 * v["median_ms"])
        out["fit_windows_batched_%d_windows" % W] = res
        print("fit: done", file=sys.stderr, flush=True)
    if "score" in parts:
        from gpitch_amd.windows import fit_windows_exact
        m = make(h)
        X = wins[0][0]
        out["score_one_window_N2001_d60"] = _time([("exact_log_likelihood_and_grad", lambda: m.exact_log_likelihood_and_grad()),
                                                   ("exact_log_likelihood", lambda: m.exact_log_likelihood()),
                                                   ("predict_s_ssm", lambda: m.predict_s_ssm(X))], a.reps, sync)
        m._compile()
        m._pack()
        pv = np.tile(m._params.cpu().numpy(), (W, 1))
        dev = SgprWindowBatch(m, W, N, M, handle=h)
        dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
        res = _time([("exact_loglik_grad", lambda: dev.exact_loglik_grad(pv)),
                     ("exact_loglik", lambda: dev.exact_loglik_grad(pv, with_grad=False)),
                     ("predict_s_ssm", lambda: dev.predict_s_ssm(pv))], a.reps, sync)
        for v in res.values():
            v["windows_per_s"] = W / (1e-3 * v["median_ms"])
        out["score_batch_%d_windows_N2001_d60" % W] = res
        print("score, batch: done", file=sys.stderr, flush=True)
        kept = {}

        def fit(name, f):
            kept[name] = f()

        res = _time([("fit_windows_exact", lambda: fit("exact", lambda: fit_windows_exact(make, wins, maxiter=10, batch=W))),
                     ("fit_windows_batched", lambda: fit("bound", lambda: fit_windows_batched(make, wins, maxiter=10, batch=W,
                                                                                                reset=_data_only)))],
                    max(3, a.reps // 2), sync)
        for k, name in (("fit_windows_exact", "exact"), ("fit_windows_batched", "bound")):
            res[k]["windows_per_s"] = W / (1e-3 * res[k]["median_ms"])
            ll = dev.exact_loglik_grad(np.stack([r["params"] for r in kept[name]]), with_grad=False)[0]
            res[k]["mean_exact_loglik_reached"] = float(np.mean(ll))
            res[k]["mean_nfev"] = float(np.mean([r["nfev"] for r in kept[name]]))
        res["mean_exact_loglik_at_start"] = float(np.mean(dev.exact_loglik_grad(pv, with_grad=False)[0]))
        out["score_fit_%d_windows" % W] = res
        dev.close()
        m._destroy()
        print("score, fit: done", file=sys.stderr, flush=True)
    if "cfg5" in parts:
        N5, M5, P5 = 65536, 512, 5
        X, Y, Z = _window(N5, M5, P5, 1)
        m = SGPRSS(X, Y, np.sum(_kernels(P5, 10)), Z, handle=h)
        res = _time([("predict_s_sparse", lambda: m.predict_s_sparse(X)), ("predict_s_ssm", lambda: m.predict_s_ssm(X)),
                     ("exact_log_likelihood", lambda: m.exact_log_likelihood())], max(3, a.reps // 2), sync)
        res["predict_s"] = "cannot run: one N x N float64 matrix is %.0f GB" % (8e-9 * N5 * N5)
        res["ssm_workspace_GB"] = 1e-9 * int(h.lib.gp_ssm_smooth_workspace_bytes(100, N5, P5, 1))
        out["one_window_N65536_d100"] = res
        m._destroy()
    if "sample" in parts:
        m = make(h)
        X = wins[0][0]
        out["sample_one_window_N2001_d60"] = _time(
            [("sample_s_ssm_S1", lambda: m.sample_s_ssm(X, 1, seed=1)), ("sample_s_ssm_S16", lambda: m.sample_s_ssm(X, 16, seed=1)),
             ("exact_log_likelihood", lambda: m.exact_log_likelihood()), ("predict_s_ssm", lambda: m.predict_s_ssm(X)),
             ("sample_s_sparse_S1", lambda: m.sample_s_sparse(X, 1, seed=1)),
             ("sample_s_sparse_S16", lambda: m.sample_s_sparse(X, 16, seed=1))], a.reps, sync)
        print("sample, one window: done", file=sys.stderr, flush=True)
        m._compile()
        m._pack()
        pv = np.tile(m._params.cpu().numpy(), (W, 1))
        dev = SgprWindowBatch(m, W, N, M, handle=h)
        dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
        res = _time([("sample_s_ssm_S1", lambda: dev.sample_s_ssm(pv, None, 1, seed=1)),
                     ("sample_s_ssm_S16", lambda: dev.sample_s_ssm(pv, None, 16, seed=1)),
                     ("exact_loglik", lambda: dev.exact_loglik_grad(pv, with_grad=False)),
                     ("predict_s_ssm", lambda: dev.predict_s_ssm(pv)),
                     ("sample_s_sparse_S16", lambda: dev.sample_s_sparse(pv, None, 16, seed=1))], a.reps, sync)
        for k, v in res.items():
            v["windows_per_s"] = W / (1e-3 * v["median_ms"])
        res["sample_workspace_GB_S16"] = 1e-9 * int(h.lib.gp_ssm_sample_workspace_bytes(60, N, P, 16, W))
        res["smooth_workspace_GB"] = 1e-9 * int(h.lib.gp_ssm_smooth_workspace_bytes(60, N, P, W))
        out["sample_batch_%d_windows_N2001_d60" % W] = res
        dev.close()
        m._destroy()
        print("sample, batch: done", file=sys.stderr, flush=True)
        N5, M5, P5 = 65536, 512, 5
        X, Y, Z = _window(N5, M5, P5, 1)
        m = SGPRSS(X, Y, np.sum(_kernels(P5, 10)), Z, handle=h)
        res = _time([("sample_s_ssm_S16", lambda: m.sample_s_ssm(X, 16, seed=1)),
                     ("exact_log_likelihood", lambda: m.exact_log_likelihood())], max(3, a.reps // 2), sync)
        res["sample_workspace_GB_S16"] = 1e-9 * int(h.lib.gp_ssm_sample_workspace_bytes(100, N5, P5, 16, 1))
        res["sample_workspace_GB_S1"] = 1e-9 * int(h.lib.gp_ssm_sample_workspace_bytes(100, N5, P5, 1, 1))
        res["smooth_workspace_GB"] = 1e-9 * int(h.lib.gp_ssm_smooth_workspace_bytes(100, N5, P5, 1))
        out["sample_one_window_N65536_d100"] = res
        m._destroy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
