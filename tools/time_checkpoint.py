"""What a checkpoint costs: file size and wall time of gpitch_amd.save / gpitch_amd.load.

    python tools/time_checkpoint.py [--out DIR] [--reps 5] [--models 88]

One notebook-size Pdgp (one pitch, M = 109 inducing points for the activation and for the component, 5 partials, 32 000
frames), trained for two Adam iterations so that it is compiled and carries moments on the device — with its data and
with data=False — and --models of them in one file.  Host timers only, each figure the median of --reps runs; the handle
is synchronised before every timer starts (save reads the moments of a compiled model from the device, load does no
device work).  Writes checkpoint_time.json into --out (default profiles/checkpoint/)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def notebook_model(seed=0):
    import gpitch_amd
    from gpitch_amd.synth import make_problem, pdgp_from_problem
    m = pdgp_from_problem(make_problem(32000, 109, 1, num_partials=5, seed=seed), minibatch_size=100)
    m.za.fixed = True
    m.zc.fixed = True
    m.optimize(method=gpitch_amd.train.AdamOptimizer(0.005), maxiter=2)
    return m


def median_ms(fn, sync, reps):
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def measure(obj, data, path, sync, reps):
    import gpitch_amd
    save_ms = median_ms(lambda: gpitch_amd.save(path, obj, data=data), sync, reps)
    given = None
    if not data:
        pair = lambda m: (m.x._array, m.y._array)
        given = [pair(m) for m in obj] if isinstance(obj, list) else pair(obj)
    load_ms = median_ms(lambda: gpitch_amd.load(path, data=given), sync, reps)
    return {"data": bool(data), "file_bytes": os.path.getsize(path), "save_ms": save_ms, "load_ms": load_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", type=int, default=88)
    args = ap.parse_args()
    from gpitch_amd import _lib
    h = _lib.default_handle()
    one = notebook_model()
    many = [one] + [notebook_model(seed=k) for k in range(1, args.models)]
    res = {"model": {"frames": 32000, "M": 109, "partials": 5, "sources": 1}, "reps": args.reps, "format_version": None}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ckpt.npz")
        res["one_model"] = [measure(one, True, path, h.sync, args.reps), measure(one, False, path, h.sync, args.reps)]
        res["many_models"] = dict(measure(many, True, path, h.sync, args.reps), models=args.models)
    from gpitch_amd import checkpoint
    res["format_version"] = checkpoint.FORMAT_VERSION
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "checkpoint_time.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
