"""Wall time of drawing joint posterior samples of many demo-size Pdgp models together (gpitch_amd.sample_sources_many)
against the loop of m.sample_sources over the same models.

Every model is the real-audio notebook model of tools/time_pdgp_predict.py (32 000 frames, 109 inducing points, a Matern32
activation and a MercerMatern12sm component with 5 partials).  S = 16 seeded draws at x[::3].  The loop is timed twice: on
fresh models, so that it builds every model's single-model engine plan and factorises, and on models whose plans and
factorisations exist.  Loop and batched call run in the same process; host clock around device-synchronised work, warm-up
excluded, medians of --reps runs.  One JSON line per model count on stdout.

    python tools/time_pdgp_sample_many.py [--models 12 88] [--draws 16] [--reps 5] [--fresh-reps 3] [--only-many]

--only-many runs the batched call alone (for a kernel trace in a run of its own).
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
    ap.add_argument("--models", type=int, nargs="+", default=[12, 88])
    ap.add_argument("--draws", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fresh-reps", type=int, default=3)
    ap.add_argument("--only-many", action="store_true")
    a = ap.parse_args()
    import torch
    import gpitch_amd
    sync = torch.cuda.synchronize
    base = demo_model()
    xs = base.x._array.reshape(-1, 1)[::3].copy()
    S, n = a.draws, xs.shape[0]
    med = lambda v: sorted(v)[len(v) // 2]
    rs = np.random.RandomState(0)
    for W in a.models:
        pool = []
        for j in range(W):
            m = copy.deepcopy(base)
            m.q_mu_act[0].value = 0.1 * rs.randn(*m.q_mu_act[0].value.shape)
            m.q_mu_com[0].value = 0.1 * rs.randn(*m.q_mu_com[0].value.shape)
            pool.append(m)
        gpitch_amd.sample_sources_many(pool, xs, num_samples=S, seed=0)          # warm-up
        many = [_timed(lambda: gpitch_amd.sample_sources_many(pool, xs, num_samples=S, seed=1 + r), sync)[0]
                for r in range(a.reps)]
        row = {"models": W, "draws": S, "frames_per_model": n, "sample_sources_many_ms": 1e3 * med(many),
               "many_model_draws_per_s": W * S / med(many), "sample_sources_many_runs_ms": [round(1e3 * t, 3) for t in many]}
        if not a.only_many:
            fresh_t = []
            for r in range(a.fresh_reps + 1):
                fresh = [copy.deepcopy(m) for m in pool]
                dt, _ = _timed(lambda: [m.sample_sources(xs, num_samples=S, seed=1 + r + k) for k, m in enumerate(fresh)], sync)
                if r:
                    fresh_t.append(dt)
                last = fresh
            warm_t = [_timed(lambda: [m.sample_sources(xs, num_samples=S, seed=50 + r + k) for k, m in enumerate(last)], sync)[0]
                      for r in range(a.reps)]
            row.update({"loop_fresh_ms": 1e3 * med(fresh_t), "loop_fresh_model_draws_per_s": W * S / med(fresh_t),
                        "loop_planned_ms": 1e3 * med(warm_t), "loop_planned_model_draws_per_s": W * S / med(warm_t),
                        "speedup_fresh": med(fresh_t) / med(many), "speedup_planned": med(warm_t) / med(many)})
            del last
        print(json.dumps(row), flush=True)
        del pool


if __name__ == "__main__":
    main()
