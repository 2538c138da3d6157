"""Times the kernel-learning stage (samplecov / kernelfit) on the device.

For B in {1, 12, 88} recordings, L = 441, K = 10 000: the segment Gram (gp_segment_gram: start upload, MFMA kernel and
partial-tile reduction, HIP events around the launches of one call, median of --reps) and its fraction of the 78.6 TF
float64 matrix peak (useful flop B L (L + 1) K: the lower triangle only).  Then learn_kernels on 12 synthetic notes
(MIDI 55..66, 2 s at 16 kHz) against the numpy restatement of the reference path on the host (10 000 outer products per
note, L-BFGS-B by forward differences).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F64_MATRIX = 78.6e12


def note(midi, fs=16000., seconds=2.0, seed=0):
    rng = np.random.RandomState(seed)
    t = np.arange(int(fs * seconds)) / fs
    f0 = 440. * 2 ** ((midi - 69) / 12.)
    y = sum(np.exp(-(2 + h) * t) * (0.6 ** h) * np.sin(2 * np.pi * f0 * (h + 1) * (1 + 1e-4 * h * h) * t + h)
            for h in range(8) if f0 * (h + 1) < fs / 2)
    return (y + 1e-3 * rng.randn(t.size)).reshape(-1, 1)


def host_reference(y, name, fs, num_sam=10000, size=441, max_par=20):
    """the reference path restated in numpy: get_samples + comatrix + kernelfit.fit (no gradient)"""
    from scipy.optimize import minimize
    from gpitch_amd.methods import find_ideal_f0, init_cparam
    x = y.reshape(-1)
    cov = np.zeros((size, size))
    for _ in range(num_sam):
        i = np.random.randint(0, x.size - size)
        s = x[i:i + size].reshape(-1, 1)
        cov += s @ s.T
    cov *= 1. / num_sam
    kern = cov[0].copy()
    kern /= np.max(np.abs(kern))
    xk = np.linspace(0., (size - 1.) / fs, size)
    if0 = find_ideal_f0([name])[0]
    f, v = init_cparam(y=y, fs=fs, maxh=max_par, ideal_f0=if0, scaled=False)[0:2]
    p0 = np.hstack(([0., 1.], v, f))

    def loss(p):
        m = (p.size - 2) // 2
        a = np.sqrt(3.) * xk / np.abs(p[1])
        k = (1 + a) * np.exp(-a) * (np.abs(p[2:2 + m]) @ np.cos(2 * np.pi * np.abs(p[2 + m:, None]) * xk[None, :]))
        return np.sqrt(np.mean((k - kern) ** 2))
    return minimize(loss, p0, method="L-BFGS-B", tol=1e-12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-notes", type=int, default=12)
    args = ap.parse_args()
    import ctypes as C
    import torch
    from gpitch_amd import _lib, kernelfit, samplecov
    h = _lib.default_handle()
    L, K = 441, 10000
    out = {"L": L, "K": K, "device": torch.cuda.get_device_name(0)}
    rng = np.random.RandomState(0)
    for B in (1, 12, 88):
        xs = [rng.randn(32000) for _ in range(B)]
        starts = [rng.randint(0, 32000 - L, size=K) for _ in range(B)]
        groups = samplecov.plan_launches([x.size for x in xs], K, L)
        prepared = []
        for b0, b1 in groups:
            lens = np.array([x.size for x in xs[b0:b1]], np.int64)
            offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
            st = np.ascontiguousarray(np.stack([s + o for s, o in zip(starts[b0:b1], offs)]).astype(np.int32))
            nb = samplecov.gram_workspace_bytes(b1 - b0, K, L)
            prepared.append((b1 - b0, lens, offs, st, h.to_device(np.concatenate(xs[b0:b1])), h.empty(b1 - b0, L, L),
                             h.workspace(nb), nb))

        def call():
            for nb_, lens, offs, st, y, c, ws, nb in prepared:
                h.check(h.lib.gp_segment_gram(h.h, _lib._ptr(y), int(lens.sum()), offs.ctypes.data_as(C.c_void_p),
                                              lens.ctypes.data_as(C.c_void_p), nb_, st.ctypes.data_as(C.c_void_p), K, L,
                                              _lib._ptr(c), _lib._ptr(ws), nb))
        call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = float(np.median(ts))
        out["gram_B%d_ms" % B] = round(ms, 4)
        out["gram_B%d_of_peak" % B] = round(B * L * (L + 1) * K / (ms * 1e-3) / PEAK_F64_MATRIX, 3)
        out["gram_B%d_launches" % B] = len(groups)
        del prepared
    notes = [note(55 + i, seed=i) for i in range(12)]
    names = ["synth_M%d_train.wav" % (55 + i) for i in range(12)]
    np.random.seed(0)
    kernelfit.learn_kernels(notes[:1], names[:1], 16000.)        # warm-up (library, self-check of lbfgsb_batch)
    np.random.seed(0)
    t0 = time.perf_counter()
    kernelfit.learn_kernels(notes, names, 16000.)
    out["learn_kernels_12_s"] = round(time.perf_counter() - t0, 3)
    if args.host_notes > 0:
        np.random.seed(0)
        t0 = time.perf_counter()
        nfev = []
        for i in range(args.host_notes):
            nfev.append(int(host_reference(notes[i], names[i], 16000.).nfev))
        hs = time.perf_counter() - t0
        out["host_reference_notes"] = args.host_notes
        out["host_reference_s"] = round(hs, 3)
        out["host_reference_nfev_median"] = int(np.median(nfev))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
