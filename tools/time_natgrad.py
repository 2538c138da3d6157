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
    python tools/time_natgrad.py adaptive-time [--out DIR] [--iters 200] [--reps 5] [--gamma-com G] [--halvings 4]
        the token with a length per role / a halving budget on twin models, windows alternating in one process:
        the plain token NatGradAdam(0.01, 0.0025) against NatGradAdam(0.01, 0.0025, gamma_com=G, halvings=H) with nothing to
        halve (the idle rounds), at the demo and headline sizes; then, on tests/natgrad_adaptive_ref.py's 6e-6 problem, one step
        from gamma = 1 (two real halvings) against one from gamma = 1/4 (none) and the plain entry at 1/4, state and gradient
        restored before every call.  With GPITCH_AMD_LIB naming another build of the library and --plain-only: the plain token
        alone (the figure to set beside this build's).
    python tools/time_natgrad.py adaptive-progress [--out DIR] [--iters 2000] [--every 100]
        the progress protocol above with AdamOptimizer(0.0025), NatGradAdam(0.1, 0.0025), NatGradAdam(0.5, 0.0025, gamma_com=1,
        halvings=4) and NatGradAdam(1, 0.0025, halvings=6), and the halvings each window took.
Writes natgrad_time.json / natgrad_progress.json / adaptive_time.json / adaptive_progress.json into --out (default
profiles/natgrad/)."""
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


def adaptive_time_model(name, build, iters, reps, gamma_com, halvings, plain_only, gamma=0.01):
    """twin models, plain token and adaptive token, windows alternating (time_model's long-minus-short windows)"""
    from gpitch_amd.train import NatGradAdam
    runs = [("plain", NatGradAdam(gamma, 0.0025), build())]
    if not plain_only:
        runs.append(("adaptive", NatGradAdam(gamma, 0.0025, gamma_com=gamma_com, halvings=halvings), build()))
    for _, method, m in runs:
        window(m, method, max(iters // 4, 3))
    t = {k: [] for k, _, _ in runs}
    halv = None
    for _ in range(reps):
        for k, method, m in runs:
            t1 = window(m, method, iters) * iters
            t3 = window(m, method, 3 * iters) * 3 * iters
            t[k].append((t3 - t1) / (2 * iters))
    if not plain_only:
        halv = runs[1][2].optimize(method=runs[1][1], maxiter=iters).natgrad["halvings"]
    res = {"model": name, "library": os.environ.get("GPITCH_AMD_LIB", "product"), "gamma": gamma, "gamma_com": gamma_com,
           "halvings": halvings, "iters_per_window": iters, "windows": reps, "halvings_taken_in_a_last_window": halv}
    for k, v in t.items():
        res[k + "_token_ms_per_iteration"] = {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    if not plain_only:
        res["adaptive_over_plain"] = res["adaptive_token_ms_per_iteration"]["median"] / res["plain_token_ms_per_iteration"]["median"]
    print(json.dumps(res))
    return res


def real_halvings(iters, reps):
    """the 6e-6 problem: device time of one step that halves twice, one that does not, and the plain entry, alternating; params,
    free state and gradient are restored by three device copies before every call (in all three)"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import natgrad_adaptive_ref as nga
    from gpitch_amd.synth import pdgp_from_problem
    m = pdgp_from_problem(nga.halving_problem(6e-6), whiten=True)
    m._pack()
    m._elbo(True)
    h = m._handle
    keep = [t.clone() for t in (m._params, m._free, m._grad)]
    G = len(m._layout)
    ws = h.workspace(h.lib.gp_pdgp_natgrad_workspace_bytes(m._plan))
    wsa = h.workspace(h.lib.gp_pdgp_natgrad_adaptive_workspace_bytes(m._plan))
    h.check(h.lib.gp_pdgp_natgrad_counts(m._plan, wsa.data_ptr(), None, None, 1))
    ptrs = (m._plan, m._params.data_ptr(), m._free.data_ptr(), m._grad.data_ptr())

    def restore():
        for dst, src in zip((m._params, m._free, m._grad), keep):
            dst.copy_(src)
    one, quarter = (C.c_double * G)(1.0, 1.0), (C.c_double * G)(0.25, 1.0)
    calls = {"adaptive from 1 (two halvings)": lambda: h.lib.gp_pdgp_natgrad_step_adaptive(*(ptrs + (one, 4, None, wsa.data_ptr(), wsa.numel()))),
             "adaptive from 1/4 (none), halvings=4": lambda: h.lib.gp_pdgp_natgrad_step_adaptive(*(ptrs + (quarter, 4, None, wsa.data_ptr(), wsa.numel()))),
             "adaptive from 1/4, halvings=0": lambda: h.lib.gp_pdgp_natgrad_step_adaptive(*(ptrs + (quarter, 0, None, wsa.data_ptr(), wsa.numel()))),
             "plain entry at 1/4": lambda: h.lib.gp_pdgp_natgrad_step(*(ptrs + (0.25, None, ws.data_ptr(), ws.numel())))}
    t = {k: [] for k in calls}
    for _ in range(reps + 1):                       # (the first round is the warm-up)
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                restore()
                h.check(fn())
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) / iters)
    hv, sg = (C.c_int64 * G)(), (C.c_double * G)()
    h.check(h.lib.gp_pdgp_natgrad_counts(m._plan, wsa.data_ptr(), hv, sg, 0))
    h.check(h.lib.gp_check_not_pd(h.h))
    res = {"model": "tests/natgrad_adaptive_ref.py halving_problem(6e-6): M = 12 / 10", "calls_per_window": iters, "windows": reps,
           "ms_per_call_with_three_restoring_copies": {k: {"median": float(np.median(v[1:])), "min": min(v[1:]), "max": max(v[1:])}
                                                       for k, v in t.items()},
           "halvings_counted": list(hv), "shortest_gamma": list(sg)}
    print(json.dumps(res))
    return res


def adaptive_progress(iters, every):
    from gpitch_amd import _lib
    from gpitch_amd.train import AdamOptimizer, NatGradAdam
    evalm = anchor_model(None)
    runs = [("AdamOptimizer(0.0025)", AdamOptimizer(0.0025)), ("NatGradAdam(0.1, 0.0025)", NatGradAdam(0.1, 0.0025)),
            ("NatGradAdam(0.5, 0.0025, gamma_com=1.0, halvings=4)", NatGradAdam(0.5, 0.0025, gamma_com=1.0, halvings=4)),
            ("NatGradAdam(1.0, 0.0025, halvings=6)", NatGradAdam(1.0, 0.0025, halvings=6))]
    out = {"model": "real-audio anchor (tests/golden/init_liv_real_audio.npz), minibatch 100", "every": every, "runs": []}
    for name, method in runs:
        m = anchor_model(100)
        trace, note, halv, shortest = [full_elbo(evalm, m)], None, [], []
        for it in range(every, iters + 1, every):
            try:
                res = m.optimize(method=method, maxiter=every)
            except _lib.NotPositiveDefiniteError as e:
                note = "refused between iterations %d and %d: %s" % (it - every, it, e)
                break
            if "natgrad" in res:
                halv.append(res.natgrad["halvings"])
                shortest.append(res.natgrad["shortest_gamma"])
            trace.append(full_elbo(evalm, m))
        out["runs"].append({"method": name, "full_data_elbo": trace, "note": note, "halvings_per_window": halv,
                            "shortest_gamma_per_window": shortest})
        print(name, "ELBO at 0 / %d / %d: %.3f / %.3f / %.3f %s" % (every, every * (len(trace) - 1), trace[0], trace[min(1, len(trace) - 1)],
                                                                  trace[-1], note or ""), "halvings", [sum(h) for h in halv])
    target = out["runs"][0]["full_data_elbo"][-1]
    out["adam_elbo_at_end"] = target
    for r in out["runs"]:
        hit = [i * every for i, v in enumerate(r["full_data_elbo"]) if v >= target]
        r["first_iteration_at_or_above_adam_end"] = hit[0] if hit else None
        print("%-52s first at or above Adam's final ELBO %.3f: %s" % (r["method"], target, hit[0] if hit else "never"))
    return out


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
    ap.add_argument("what", choices=["time", "progress", "adaptive-time", "adaptive-progress"])
    ap.add_argument("--gamma-com", type=float, default=None)
    ap.add_argument("--halvings", type=int, default=4)
    ap.add_argument("--plain-only", action="store_true", help="adaptive-time: the plain token alone (another build of the library)")
    ap.add_argument("--name", default=None, help="adaptive-time: file name instead of adaptive_time.json")
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
    elif args.what == "adaptive-time":
        it = args.iters or 200
        res = [adaptive_time_model("demo (N = 16000, minibatch 100, P = 1)", demo_model, it, args.reps, args.gamma_com, args.halvings,
                                   args.plain_only),
               adaptive_time_model("headline (N = 32768, M = 512, P = 12, m = 20, float64, full batch)", headline_model,
                                   max(it // 10, 5), args.reps, args.gamma_com, args.halvings, args.plain_only)]
        if not args.plain_only:
            res.append(real_halvings(it, args.reps))
        path = os.path.join(args.out, args.name or "adaptive_time.json")
    elif args.what == "adaptive-progress":
        res = adaptive_progress(args.iters or 2000, args.every)
        path = os.path.join(args.out, "adaptive_progress.json")
    else:
        res = progress(args.iters or 2000, args.every)
        path = os.path.join(args.out, "natgrad_progress.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
