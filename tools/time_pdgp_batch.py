"""Steps per second of many demo-size Pdgp models trained together (gpitch_amd.optimize_many) against the same
models trained one after another by Pdgp.optimize.

Every model is the real-audio notebook model (tests/golden/init_liv_real_audio.npz: 32 000 frames, init_liv -> 109
inducing points, Matern32 + MercerMatern12sm with 5 partials, minibatch 100, z fixed).  Device-synchronised wall
time, warm-up steps excluded; one JSON line per W on stdout.

    python tools/time_pdgp_batch.py [--models 1 12 88] [--steps 200] [--warmup 20] [--seq-steps 100]

    python tools/time_pdgp_batch.py --natgrad GAMMA [--models 12 88] [--steps 100] [--seq-steps 20] [--repeats 5]

times optimize_many with NatGradAdam(GAMMA, 0.0025) per step, optimize_many with AdamOptimizer(0.0025) on the same
batch (the figure of the Adam path) and the loop of m.optimize(method=NatGradAdam(GAMMA, 0.0025)) over twin models,
in the same process: medians of --repeats windows each, the three alternating, with their ranges.

    python tools/time_pdgp_batch.py --natgrad GAMMA [--gamma-com G] --halvings H [--models 12 88] [--steps 100] [--repeats 5]

times optimize_many with the plain token NatGradAdam(GAMMA, 0.0025) against the token with gamma_com = G and / or
halvings = H (gp_pdgpb_natgrad_adaptive) on twin batches, the two alternating: the cost of the loop around the
form kernel when nothing is halved.  The halving counts of the last window are printed with it.

    python tools/time_pdgp_batch.py --tied [--natgrad GAMMA] [--models 12 88] [--steps 200] [--repeats 5]

times optimize_many with the noise variance and the kernels of all models tied (tie_groups; DESIGN.md 3l: one more launch
per iteration) against the untied twin batch, the two alternating.
"""
import argparse
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
    d = np.load(os.path.join(ROOT, "tests", "golden", "init_liv_real_audio.npz"))
    y = np.asarray(d["y"], dtype=np.float64).reshape(-1, 1)
    fs = int(d["fs"])
    x = np.linspace(0., (y.size - 1.) / fs, y.size).reshape(-1, 1)
    f0 = gpitch_amd.find_ideal_f0([str(d["fname"])])
    z, _ = gpitch_amd.init_liv(x=x, y=y, win_size=31, thres=0.033, dec=9)
    kcom = MercerMatern12sm(input_dim=1, energy=np.ones(5), frequency=f0 * np.arange(1, 6))
    m = gpitch_amd.pdgp.Pdgp(x=x, y=y, z=z, kern=[[Matern32(1, lengthscales=1.0, variance=1.0)], [kcom]],
                             minibatch_size=100)
    m.za.fixed = True
    m.zc.fixed = True
    return m


def natgrad_main(a):
    """three figures per model count, medians of a.repeats device-synchronised windows"""
    import copy
    import torch
    import gpitch_amd
    from gpitch_amd.pdgp_batch import PdgpBatch
    ng = gpitch_amd.train.NatGradAdam(a.natgrad, 0.0025)
    adam = gpitch_amd.train.AdamOptimizer(0.0025)
    base = demo_model()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for W in a.models:
        bn = PdgpBatch([copy.deepcopy(base) for _ in range(W)])
        ba = PdgpBatch([copy.deepcopy(base) for _ in range(W)])
        seq = [copy.deepcopy(base) for _ in range(W)]
        bn.optimize(ng, a.warmup)
        ba.optimize(adam, a.warmup)
        for m in seq:
            m.optimize(method=ng, maxiter=a.warmup)
        t = {"natgrad": [], "adam": [], "loop": []}
        ok = True
        for _ in range(a.repeats):
            res = []
            t["natgrad"].append(1e3 * window(lambda: res.extend(bn.optimize(ng, a.steps))) / a.steps)
            ok = ok and all(r.success for r in res)
            t["adam"].append(1e3 * window(lambda: ba.optimize(adam, a.steps)) / a.steps)
            t["loop"].append(1e3 * window(lambda: [m.optimize(method=ng, maxiter=a.seq_steps) for m in seq])
                             / (W * a.seq_steps))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"models": W, "gamma": a.natgrad, "steps": a.steps, "repeats": a.repeats, "every_model_succeeded": ok,
                          "batched_natgrad_ms_per_step": med["natgrad"], "batched_natgrad_range": [min(t["natgrad"]), max(t["natgrad"])],
                          "batched_adam_ms_per_step": med["adam"], "batched_adam_range": [min(t["adam"]), max(t["adam"])],
                          "loop_natgrad_ms_per_model_step": med["loop"], "loop_natgrad_range": [min(t["loop"]), max(t["loop"])],
                          "natgrad_over_adam": med["natgrad"] / med["adam"],
                          "batched_natgrad_model_steps_per_s": 1e3 * W / med["natgrad"],
                          "loop_natgrad_model_steps_per_s": 1e3 / med["loop"],
                          "speedup_over_loop": W * med["loop"] / med["natgrad"]}), flush=True)


def adaptive_main(a):
    """plain token against the per-role / halving token on twin batches, alternating windows"""
    import copy
    import torch
    import gpitch_amd
    from gpitch_amd.pdgp_batch import PdgpBatch
    plain = gpitch_amd.train.NatGradAdam(a.natgrad, 0.0025)
    adapt = gpitch_amd.train.NatGradAdam(a.natgrad, 0.0025, gamma_com=a.gamma_com, halvings=a.halvings)
    base = demo_model()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for W in a.models:
        bp = PdgpBatch([copy.deepcopy(base) for _ in range(W)])
        bq = PdgpBatch([copy.deepcopy(base) for _ in range(W)])
        bp.optimize(plain, a.warmup)
        bq.optimize(adapt, a.warmup)
        t = {"plain": [], "adaptive": []}
        ok, halv = True, 0
        for _ in range(a.repeats):
            rp, rq = [], []
            t["plain"].append(1e3 * window(lambda: rp.extend(bp.optimize(plain, a.steps))) / a.steps)
            t["adaptive"].append(1e3 * window(lambda: rq.extend(bq.optimize(adapt, a.steps))) / a.steps)
            ok = ok and all(r.success for r in rp + rq)
            halv = sum(sum(r.natgrad["halvings"]) for r in rq if r.success)
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"models": W, "gamma": a.natgrad, "gamma_com": a.gamma_com, "halvings": a.halvings, "steps": a.steps,
                          "repeats": a.repeats, "every_model_succeeded": ok, "halvings_taken_in_the_last_window": halv,
                          "library": os.environ.get("GPITCH_AMD_LIB", "product"),
                          "plain_token_ms_per_step": med["plain"], "plain_token_range": [min(t["plain"]), max(t["plain"])],
                          "adaptive_token_ms_per_step": med["adaptive"],
                          "adaptive_token_range": [min(t["adaptive"]), max(t["adaptive"])],
                          "adaptive_over_plain": med["adaptive"] / med["plain"]}), flush=True)


def tied_main(a):
    """the batch with noise and kernels of all models tied (tie_groups) against its untied twin, alternating windows"""
    import copy
    import torch
    import gpitch_amd
    from gpitch_amd.pdgp_batch import PdgpBatch, tie_groups
    tok = gpitch_amd.train.AdamOptimizer(0.0025) if a.natgrad is None else gpitch_amd.train.NatGradAdam(a.natgrad, 0.0025)
    base = demo_model()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for W in a.models:
        mt = [copy.deepcopy(base) for _ in range(W)]
        bt = PdgpBatch(mt, tied=tie_groups(mt))
        bu = PdgpBatch([copy.deepcopy(base) for _ in range(W)])
        bt.optimize(tok, a.warmup)
        bu.optimize(tok, a.warmup)
        t = {"tied": [], "untied": []}
        ok = True
        for _ in range(a.repeats):
            rt, ru = [], []
            t["untied"].append(1e3 * window(lambda: ru.extend(bu.optimize(tok, a.steps))) / a.steps)
            t["tied"].append(1e3 * window(lambda: rt.extend(bt.optimize(tok, a.steps))) / a.steps)
            ok = ok and all(r.success for r in rt + ru)
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"models": W, "method": "adam" if a.natgrad is None else "natgrad %g" % a.natgrad, "steps": a.steps,
                          "repeats": a.repeats, "every_model_succeeded": ok, "tie_groups": len(bt._tie_groups),
                          "members_per_group": W,
                          "untied_ms_per_step": med["untied"], "untied_range": [min(t["untied"]), max(t["untied"])],
                          "tied_ms_per_step": med["tied"], "tied_range": [min(t["tied"]), max(t["tied"])],
                          "tied_minus_untied_ms": med["tied"] - med["untied"],
                          "tied_over_untied": med["tied"] / med["untied"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, nargs="+", default=[1, 12, 88])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seq-steps", type=int, default=100, help="Adam steps per model on the one-after-another path")
    ap.add_argument("--natgrad", type=float, default=None, metavar="GAMMA",
                    help="time NatGradAdam(GAMMA, 0.0025): batched, the batched Adam step, and the single-model loop")
    ap.add_argument("--repeats", type=int, default=5, help="windows per figure with --natgrad (the median is reported)")
    ap.add_argument("--gamma-com", type=float, default=None, help="with --natgrad: the component GPs' own step length")
    ap.add_argument("--halvings", type=int, default=0, help="with --natgrad: the halving budget (0..10)")
    ap.add_argument("--tied", action="store_true",
                    help="time the batch with noise and kernels of all models tied (tie_groups) against its untied twin")
    a = ap.parse_args()
    if a.tied:
        return tied_main(a)
    if a.natgrad is not None and (a.gamma_com is not None or a.halvings):
        return adaptive_main(a)
    if a.natgrad is not None:
        return natgrad_main(a)
    import copy
    import torch
    import gpitch_amd
    from gpitch_amd.pdgp_batch import PdgpBatch
    tok = gpitch_amd.train.AdamOptimizer(0.0025)
    base = demo_model()
    for W in a.models:
        models = [copy.deepcopy(base) for _ in range(W)]
        batch = PdgpBatch(models)
        batch.optimize(tok, a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch.optimize(tok, a.steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        seq = [copy.deepcopy(base) for _ in range(W)]
        for m in seq:
            m.optimize(method=tok, maxiter=a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for m in seq:
            m.optimize(method=tok, maxiter=a.seq_steps)
        torch.cuda.synchronize()
        ds = time.perf_counter() - t0
        print(json.dumps({"models": W, "steps": a.steps, "batched_steps_per_s": a.steps / dt,
                          "batched_ms_per_step": 1e3 * dt / a.steps, "batched_model_steps_per_s": W * a.steps / dt,
                          "sequential_model_steps_per_s": W * a.seq_steps / ds,
                          "sequential_ms_per_model_step": 1e3 * ds / (W * a.seq_steps),
                          "speedup": (W * a.steps / dt) / (W * a.seq_steps / ds)}), flush=True)


if __name__ == "__main__":
    main()
