"""Wall time of predicting many demo-size Pdgp models together (gpitch_amd.predict_many) against the loop of
m.predict_act_n_com over the same models.

Every model is the real-audio notebook model (tests/golden/init_liv_real_audio.npz: 32 000 frames, init_liv -> 109
inducing points, Matern32 + MercerMatern12sm with 5 partials).  Inputs: x[::3] (notebook cell 11) and all 32 000 frames.
The loop is timed twice: on fresh models, so that it builds every model's single-model engine plan, and on models whose
plans exist, at inputs none of them has seen (the prediction memo does not answer; the Params have not changed, so each
model reuses its factorisation and runs its strip kernels only).  Host clock around device-synchronised
work, warm-up excluded, medians of --reps runs.  One JSON line per (models, inputs) on stdout.

    python tools/time_pdgp_predict.py [--models 1 12 88] [--reps 5] [--fresh-reps 3]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_pdgp_batch import demo_model  # noqa: E402


def _timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, nargs="+", default=[1, 12, 88])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fresh-reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import gpitch_amd
    sync = torch.cuda.synchronize
    base = demo_model()
    x = base.x._array.reshape(-1, 1).copy()
    # every model its own Params: q_mu of the activation perturbed per model (the plans cannot be shared)
    rs = np.random.RandomState(0)
    for W in a.models:
        pool = []
        for j in range(W):
            m = copy.deepcopy(base)
            m.q_mu_act[0].value = 0.1 * rs.randn(*m.q_mu_act[0].value.shape)
            m.q_mu_com[0].value = 0.1 * rs.randn(*m.q_mu_com[0].value.shape)
            pool.append(m)
        for label, xs in (("x[::3]", x[::3]), ("all", x)):
            xin = lambda r: xs + 1e-9 * (r + 1)          # new inputs on every run: no memo answers
            gpitch_amd.predict_many(pool, xin(-1))       # warm-up
            many = sorted(_timed(lambda: gpitch_amd.predict_many(pool, xin(r)), sync)[0] for r in range(a.reps))
            # the loop on fresh models: it builds the engine plan of every model
            fresh_t, plan_bytes = [], 0
            for r in range(a.fresh_reps + 1):
                fresh = [copy.deepcopy(m) for m in pool]
                sync()
                m0 = torch.cuda.memory_allocated()
                dt, _ = _timed(lambda: [m.predict_act_n_com(xin(r)) for m in fresh], sync)
                plan_bytes = torch.cuda.memory_allocated() - m0
                if r:
                    fresh_t.append(dt)
                last = fresh
            # the loop with the plans in place, at new inputs
            for m in last:
                m.predict_act_n_com(xin(-2))
            warm_t = sorted(_timed(lambda: [m.predict_act_n_com(xin(100 + r)) for m in last], sync)[0]
                            for r in range(a.reps))
            fresh_t.sort()
            med = lambda v: v[len(v) // 2]
            n = xs.shape[0]
            print(json.dumps({"models": W, "inputs": label, "frames_per_model": n, "gp_frames": 2 * W * n,
                              "predict_many_ms": 1e3 * med(many), "loop_fresh_ms": 1e3 * med(fresh_t),
                              "loop_planned_ms": 1e3 * med(warm_t),
                              "speedup_fresh": med(fresh_t) / med(many), "speedup_planned": med(warm_t) / med(many),
                              "loop_plans_device_MiB": plan_bytes / 2.0 ** 20,
                              "predict_many_runs_ms": [round(1e3 * t, 3) for t in many]}), flush=True)
            del last
        del pool


if __name__ == "__main__":
    main()
