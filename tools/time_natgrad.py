"""NatGradAdam beside AdamOptimizer on one GPU: what an iteration costs, and how far it gets.

    python tools/time_natgrad.py time     [--out DIR] [--iters 200] [--reps 5]
        milliseconds per iteration of Pdgp.optimize with AdamOptimizer and with NatGradAdam, same model, same box, the two
        alternating (each figure the difference of a long and a short window, so that optimize()'s own packing and its final
        evaluation drop out): at the demo size (tools/time_demo_step.py's model, minibatch 100) and at the headline size (N = 32768,
        M = 512, P = 12, 20 partials, float64, full batch); median over --reps windows of --iters iterations after a warm-up
        window.  Then gp_pdgp_natgrad_step alone (device events around --iters calls), and from the handle's timers its
        factorisation launch and its two new launches (form + apply) separately.
    python tools/time_natgrad.py progress [--out DIR] [--iters 2000] [--every 100]
        the real-audio anchor model (oracle/demo_anchor.py's configuration: tests/golden/init_liv_real_audio.npz, minibatch 100):
        the full-data ELBO every --every iterations for AdamOptimizer(0.0025) and NatGradAdam(gamma, 0.0025), gamma in 0.05, 0.1,
        0.5, and the iteration count at which each first passes the ELBO that Adam reaches at the end.
Writes natgrad_time.json / natgrad_progress.json into --out (default profiles/natgrad/)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def demo_model():
    import gpitch_amd
    from gpitch_amd.kernels import Matern32
    from gpitch_amd.matern12_spectral_mixture import MercerMatern12sm
    n, fs = 16000, 16000
    x = np.linspace(0., (n - 1.) / fs, n).reshape(-1, 1)
    f = sum(np.sin(2 * np.pi * x * (i + 1) * 15.) for i in range(3))
    envelope = np.exp(-25 * (x - 0.33) ** 2) + np.exp(-75 * (x - 0.66) ** 2)
    y = f / np.max(np.abs(f)) * envelope / np.max(np.abs(envelope)) + np.sqrt(1e-6) * np.random.RandomState(0).randn(n, 1)
    z, _ = gpitch_amd.init_liv(x=x, y=y, win_size=31, thres=0.05, dec=1)
    m = gpitch_amd.pdgp.Pdgp(x=x.copy(), y=y.copy(), z=z, kern=[[Matern32(1, lengthscales=1.0, variance=1.0)],
                             [MercerMatern12sm(1, energy=np.ones(3), frequency=np.array([15., 30., 45.]))]], minibatch_size=100)
    m.za.fixed = True
    m.zc.fixed = True
    return m


def headline_model():
    from gpitch_amd.synth import make_problem, pdgp_from_problem
    m = pdgp_from_problem(make_problem(32768, 512, 12, num_partials=20, seed=0))
    m.za.fixed = True
    m.zc.fixed = True
    return m


def anchor_model(minibatch):
    import gpitch_amd
    from gpitch_amd.kernels import Matern32
    from gpitch_amd.matern12_spectral_mixture import MercerMatern12sm
    d = np.load(os.path.join(ROOT, "tests", "golden", "init_liv_real_audio.npz"))
    y = np.asarray(d["y"], dtype=np.float64).reshape(-1, 1)
    fs = int(d["fs"])
    x = np.linspace(0., (y.size - 1.) / fs, y.size).reshape(-1, 1)
    f0 = gpitch_amd.find_ideal_f0([str(d["fname"])])
    z, _ = gpitch_amd.init_liv(x=x, y=y, win_size=31, thres=0.033, dec=9)
    kcom = MercerMatern12sm(input_dim=1, energy=np.ones(5), frequency=f0 * np.arange(1, 6))
    m = gpitch_amd.pdgp.Pdgp(x=x.copy(), y=y.copy(), z=z, kern=[[Matern32(input_dim=1, lengthscales=1.0, variance=1.0)], [kcom]],
                             minibatch_size=minibatch or y.size)
    m.za.fixed = True
    m.zc.fixed = True
    return m


def window(m, method, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.optimize(method=method, maxiter=iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def time_model(name, build, iters, reps, gamma=0.01):
    """two models of the same build, one per optimiser, windows alternating; gamma small: a timing, not a training run"""
    import torch
    from gpitch_amd.train import AdamOptimizer, NatGradAdam
    adam, ng = AdamOptimizer(0.0025), NatGradAdam(gamma, 0.0025)
    ma, mn = build(), build()
    window(ma, adam, max(iters // 4, 3))
    window(mn, ng, max(iters // 4, 3))
    # optimize() packs the Params before its loop and evaluates and unpacks after it: a window of 3 n iterations minus one of
    # n leaves 2 n iterations and none of that
    ta, tn = [], []
    for _ in range(reps):
        for m, method, acc in ((ma, adam, ta), (mn, ng, tn)):
            t1 = window(m, method, iters) * iters
            t3 = window(m, method, 3 * iters) * 3 * iters
            acc.append((t3 - t1) / (2 * iters))
    # the step alone: the work of the three launches does not depend on the values (the gradient blocks are zero after the
    # first call: B = I), so repeated calls time it
    h = mn._handle
    mask = (C.c_int32 * len(mn._layout))(*([1] * len(mn._layout)))
    call = lambda: h.check(h.lib.gp_pdgp_natgrad_step(mn._plan, mn._params.data_ptr(), mn._free.data_ptr(), mn._grad.data_ptr(),
                                                      gamma, mask, mn._ng_ws.data_ptr(), mn._ng_ws.numel()))
    for _ in range(5):
        call()
    alone = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        alone.append(e0.elapsed_time(e1) / iters)
    h.check(h.lib.gp_timers_enable(h.h, 1))
    h.check(h.lib.gp_timers_reset(h.h))
    for _ in range(iters):
        call()
    h.sync()
    tm = h.timers()
    h.check(h.lib.gp_timers_enable(h.h, 0))
    res = {"model": name, "latent_gps": len(mn._layout), "M": [int(v) for v in list(mn.num_inducing_a) + list(mn.num_inducing_c)],
           "iters_per_window": iters, "windows": reps,
           "adam_ms_per_iteration": {"median": float(np.median(ta)), "min": min(ta), "max": max(ta)},
           "natgradadam_ms_per_iteration": {"median": float(np.median(tn)), "min": min(tn), "max": max(tn)},
           "natgrad_step_alone_ms": {"median": float(np.median(alone)), "min": min(alone), "max": max(alone)},
           "natgrad_step_launches_ms": {"factor_and_inverse (chol.hip)": tm["chol"][0] / max(tm["chol"][1], 1),
                                        "form + apply (natgrad.hip)": 2.0 * tm["small_gemm"][0] / max(tm["small_gemm"][1], 1)}}
    print(json.dumps(res))
    del ma, mn
    return res


def full_elbo(evalm, m):
    for dst, src in zip(evalm._param_order(), m._param_order()):
        dst.value = src.value
    return float(evalm.compute_log_likelihood())


def progress(iters, every):
    from gpitch_amd import _lib
    from gpitch_amd.train import AdamOptimizer, NatGradAdam
    evalm = anchor_model(None)
    runs = [("AdamOptimizer(0.0025)", AdamOptimizer(0.0025))] + [("NatGradAdam(%g, 0.0025)" % g, NatGradAdam(g, 0.0025))
                                                                 for g in (0.05, 0.1, 0.5)]
    out = {"model": "real-audio anchor (tests/golden/init_liv_real_audio.npz), minibatch 100", "every": every, "runs": []}
    for name, method in runs:
        m = anchor_model(100)
        trace, note = [full_elbo(evalm, m)], None
        for it in range(every, iters + 1, every):
            try:
                m.optimize(method=method, maxiter=every)
            except _lib.NotPositiveDefiniteError as e:
                note = "refused between iterations %d and %d: %s" % (it - every, it, e)
                break
            trace.append(full_elbo(evalm, m))
        out["runs"].append({"method": name, "full_data_elbo": trace, "note": note})
        print(name, "ELBO at 0 / %d / %d: %.3f / %.3f / %.3f %s" % (every, every * (len(trace) - 1), trace[0], trace[min(1, len(trace) - 1)],
                                                                  trace[-1], note or ""))
    target = out["runs"][0]["full_data_elbo"][-1]
    out["adam_elbo_at_end"] = target
    for r in out["runs"]:
        hit = [i * every for i, v in enumerate(r["full_data_elbo"]) if v >= target]
        r["first_iteration_at_or_above_adam_end"] = hit[0] if hit else None
        print("%-28s first at or above Adam's final ELBO %.3f: %s" % (r["method"], target, hit[0] if hit else "never"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["time", "progress"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "natgrad"))
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--every", type=int, default=100)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.what == "time":
        res = [time_model("demo (N = 16000, minibatch 100, P = 1)", demo_model, args.iters or 200, args.reps),
               time_model("headline (N = 32768, M = 512, P = 12, m = 20, float64, full batch)", headline_model,
                          max((args.iters or 200) // 10, 5), args.reps)]
        path = os.path.join(args.out, "natgrad_time.json")
    else:
        res = progress(args.iters or 2000, args.every)
        path = os.path.join(args.out, "natgrad_progress.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
