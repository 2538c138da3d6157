"""The flat parameter vector of a Pdgp model, shared by the single-model engine (pdgp.py) and the batch
(pdgp_batch.py): a vector is described by its segments [(offset, Param)] — Pdgp._segments takes the offsets from
the engine's padded layout, pdgp_batch.model_segments lays them out back to back — and everything below walks them.
Host-side only."""
import numpy as np

from .param import sorted_params


def col(a, i):
    """row i of a (rows, n) result as the (n, 1) column the reference's predict_* return (a view)"""
    return a[i].reshape(-1, 1)


def latent_gps(m, rows=None):
    """(kern, z, q_mu, q_sqrt) of model m's latent GPs `rows` of [g_0..g_{P-1}, f_0..f_{P-1}] (default: all, in order)"""
    P = m.num_sources
    return [(m.kern_act[g], m.za[g], m.q_mu_act[g], m.q_sqrt_act[g]) if g < P else
            (m.kern_com[g - P], m.zc[g - P], m.q_mu_com[g - P], m.q_sqrt_com[g - P])
            for g in (range(2 * P) if rows is None else rows)]


def pack(segs, n, handle=None, out=None):
    """(values, transform codes) of a vector of n slots.  The values go into `out` when given (a page-locked buffer:
    slots no segment covers keep what it held), else into zeros.  The codes are made when `handle` is given (a Logistic
    transform registers its pair there): 2 for a `.fixed` Param and for padding, None without a handle."""
    host = np.zeros(n) if out is None else out
    tc = None if handle is None else np.full(n, 2, dtype=np.uint8)
    for off, p in segs:
        v = p.value.reshape(-1)
        host[off:off + v.size] = v
        if tc is not None and not p.fixed:
            tc[off:off + v.size] = p.transform.device_code(handle)
    return host, tc


def free_index(m, segs):
    """offsets in the vector of the entries of model m's GPflow free state, in GPflow's order (param.sorted_params:
    Params by attribute name, `.fixed` ones absent) — the layout of optimize()'s `x` and `jac`"""
    off = {id(p): o for o, p in segs}
    idx = [np.arange(off[id(p)], off[id(p)] + p.size) for p in sorted_params(m) if not p.fixed and id(p) in off]
    return np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)


def free_gradient(segs, free, grad):
    """chain rule through each Param's transform: `grad` (with respect to the parameters) times d forward / d free at
    the free vector `free`; zero outside the non-fixed segments (fixed Params are not part of the free state)"""
    out = np.zeros_like(grad)
    for off, p in segs:
        if not p.fixed:
            s = slice(off, off + p.size)
            out[s] = grad[s] * p.transform.dforward(free[s])
    return out


def set_grad_needs(h, entry, plan, gps, first=0):
    """`.fixed` Params drop out of the backward pass (GPflow removes them from the free state): tell the plan, through
    its `entry` (gp_pdgp_set_grad_needs / gp_pdgpb_set_grad_needs), for the latent GPs `gps` numbered from `first`"""
    for g, (kern, z, _, _) in enumerate(gps, first):
        need_theta = any(not p.fixed for p in kern.theta_params())
        h.check(entry(plan, g, int(need_theta), int(not z.fixed)))
