"""Sampled covariance of a training recording — gpitch/samplecov.py.

`get_cov` estimates the covariance of an isolated-note recording from `num_sam` randomly placed segments of `size`
samples (samplecov.py:5-53).  The reference sums one outer product per segment (one tf.matmul session call each);
here the Gram matrix of the segments is one float64 MFMA launch over the recording itself (gp_segment_gram: the segment
matrix is never built), and `get_cov_many` does all the recordings of a training set in as few launches as the 32-bit
addressing of the kernel allows.  `autocorr` (samplecov.py:56-74) is one fixed-order reduction per lag (gp_autocorr).

Kept from the reference: segment starts come from the global `np.random` stream, drawn as
`np.random.randint(0, x.size - size)` (so the last possible start is never drawn; one vectorised call draws the same
sequence as the reference's scalar calls, so `np.random.seed(s)` selects the reference's segments); `kern` is row 0 of
the covariance divided by its largest magnitude.  There is no CPU fallback: without a device these raise GpitchError.
"""
import ctypes as C

import numpy as np

from . import _lib

# launches of gp_segment_gram: y below the kernel's 32-bit buffer-offset limit, partial tiles below this workspace size
MAX_Y_BYTES = 2 ** 31 - 4096          # GP_SEGMENT_GRAM_MAX_Y_BYTES
MAX_WORKSPACE_BYTES = 2 ** 30


def draw_starts(n, num_sam, size):
    """start indices of `num_sam` segments of `size` samples in a recording of n samples (samplecov.py:10)"""
    return np.random.randint(0, n - size, size=num_sam)


def get_samples(x, num_sam, size):
    """samplecov.py:5-13: list of `num_sam` copies of randomly placed segments x[idx : idx + size]"""
    return [x[i:i + size].copy() for i in draw_starts(x.size, num_sam, size)]


def gram_workspace_bytes(B, K, L):
    return int(_lib.load_library().gp_segment_gram_workspace_bytes(int(B), int(K), int(L)))


def plan_launches(lengths, K, L, max_y_bytes=MAX_Y_BYTES, max_workspace_bytes=MAX_WORKSPACE_BYTES, ws_bytes=None):
    """Split recordings of `lengths` samples into consecutive groups [(begin, end), ...], one gp_segment_gram launch each:
    a group's recordings together hold at most max_y_bytes of float64 and need at most max_workspace_bytes of workspace
    (a group of one recording is always allowed the workspace).  A recording that alone exceeds max_y_bytes raises
    ValueError.  ws_bytes(B): workspace of B recordings (default: gp_segment_gram_workspace_bytes)."""
    if ws_bytes is None:
        def ws_bytes(B):
            return gram_workspace_bytes(B, K, L)
    groups = []
    begin, nbytes = 0, 0
    for i, n in enumerate(lengths):
        b = 8 * int(n)
        if b > max_y_bytes:
            raise ValueError("samplecov: a recording of %d samples exceeds the %d-byte limit of one segment-Gram launch"
                             % (n, max_y_bytes))
        if i > begin and (nbytes + b > max_y_bytes or ws_bytes(i + 1 - begin) > max_workspace_bytes):
            groups.append((begin, i))
            begin, nbytes = i, 0
        nbytes += b
    if len(lengths) > begin:
        groups.append((begin, len(lengths)))
    return groups


def _gram(xs, starts, L, handle=None):
    """(B, L, L) segment Gram matrices: xs 1-D float64 recordings, starts[b] (K,) start indices into xs[b]"""
    h = handle or _lib.default_handle()
    B, K = len(xs), len(starts[0])
    lens = np.array([x.size for x in xs], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    st = np.ascontiguousarray(np.stack([np.asarray(s, dtype=np.int64) + o for s, o in zip(starts, offs)]).astype(np.int32))
    y = h.to_device(np.concatenate(xs))
    out = h.empty(B, L, L)
    nbytes = gram_workspace_bytes(B, K, L)
    ws = h.workspace(nbytes)
    h.check(h.lib.gp_segment_gram(h.h, _lib._ptr(y), int(lens.sum()), offs.ctypes.data_as(C.c_void_p),
                                  lens.ctypes.data_as(C.c_void_p), B, st.ctypes.data_as(C.c_void_p), K, L, _lib._ptr(out),
                                  _lib._ptr(ws), nbytes))
    return out.cpu().numpy()


def segment_gram(xs, starts, L, handle=None):
    """(1/K) sum_k s_k s_k^T, s_k = xs[b][starts[b][k] : starts[b][k] + L], for every recording b of xs (1-D float64
    arrays; every starts[b] of the same length K): a list of (L, L) matrices, in the launches plan_launches gives"""
    h = handle or _lib.default_handle()
    out = []
    for b0, b1 in plan_launches([x.size for x in xs], len(starts[0]), L):
        out.extend(list(_gram(xs[b0:b1], starts[b0:b1], L, h)))
    return out


def _check_segments(n, starts, size):
    s = np.asarray(starts)
    if s.size and (s.min() < 0 or s.max() + size > n):
        raise ValueError("samplecov: a segment lies outside its recording")


def comatrix(X, handle=None):
    """samplecov.py:16-35: (1/K) sum_k X[k] X[k]^T over a list of K equally long segments"""
    K = len(X)
    L = np.asarray(X[0]).size
    y = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1) for s in X])
    return _gram([y], [np.arange(K, dtype=np.int64) * L], L, handle)[0]


def get_cov_many(xs, num_sam, size, handle=None):
    """get_cov for every recording of `xs`, in as few launches as plan_launches allows.  The segment starts are drawn
    recording by recording, in order (the draws of sequential get_cov calls).  Returns (covs, kerns, starts): lists of
    (size, size) covariances, (size, 1) normalised row 0 and the (num_sam,) start indices (the segments themselves are
    x[s : s + size]; they are not copied out, 35 MB per recording at the drivers' defaults)."""
    ys = [np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]
    starts = [draw_starts(y.size, num_sam, size) for y in ys]
    for y, s in zip(ys, starts):
        _check_segments(y.size, s, size)
    covs = segment_gram(ys, starts, size, handle)
    kerns = []
    for cov in covs:
        kern = cov[0, :].copy().reshape(-1, 1)
        kern /= np.max(np.abs(kern))
        kerns.append(kern)
    return covs, kerns, starts


def get_cov(x, num_sam, size, handle=None):
    """samplecov.py:38-53: (cov, kern, samples) — the sampled covariance, its row 0 divided by its max |.| as a (size, 1)
    column, and the list of segments used"""
    covs, kerns, starts = get_cov_many([x], num_sam, size, handle)
    samples = [x[i:i + size].copy() for i in starts[0]]
    return covs[0], kerns[0], samples


def autocorr(x, size, handle=None):
    """samplecov.py:56-74: (r / max|r| as (size, 1), samples) with r[j] = sum_{i < n - size} x[i] x[i + j].  `samples` is
    the reference's (size, n - size) matrix of shifted copies, returned as a read-only view of x (no copy)."""
    y = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    n = y.size
    if n <= size:
        raise ValueError("samplecov.autocorr: the recording must be longer than size")
    h = handle or _lib.default_handle()
    yd = h.to_device(y)
    r = h.empty(size)
    h.check(h.lib.gp_autocorr(h.h, _lib._ptr(yd), n, size, _lib._ptr(r)))
    r = r.cpu().numpy()
    r /= np.max(np.abs(r))
    samples = np.lib.stride_tricks.sliding_window_view(y, size)[:n - size].T
    return r.reshape(-1, 1), samples
