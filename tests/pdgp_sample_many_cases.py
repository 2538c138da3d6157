"""The models of the batched Pdgp sampling tests (sample_sources_many): unequal P, n, M and nonlinearity inside one call, M at
the batch's limit of 128 and M not a multiple of 16, n below and above one 64-frame tile, every supported kernel family in both
roles, partial paddings 4, 8, 20 and 32.  Frames: ref.frames(prob, n, seed + 100); eps: ref.random_eps(prob, n, S, seed + 200).
C keeps act_ls = 0.1: with the reference's l = 1 s its two host routes differ by 1.06 of a tenth of the rule."""
import numpy as np

import pdgp_sample_ref as ref

#        name  problem args                kwargs                                                        n    nlin
CASES = [("A", (12, 10, 1, 2, 204), dict(seed=401), 37, 0),
         ("B", (50, 64, 3, 2, 512), dict(seed=402), 215, 1),
         ("C", (128, 109, 2, 5, 2990), dict(seed=403, act_ls=0.1), 429, 2),
         ("D", (16, 128, 1, 20, 34816), dict(seed=404), 65, 0),
         ("E", (14, 9, 2, 3, 300), dict(seed=405, act="matern12", com="matern32", act_ls=0.05, com_ls=0.02), 23, 0),
         ("F", (113, 128, 1, 32, 4096), dict(seed=406, act_ls=0.1), 130, 0)]
NAMES = [c[0] for c in CASES]
_cache = {}


def case(name):
    """(prob, frames, nlin code, seed) of model `name`, built once and shared (treat as read-only)"""
    if name not in _cache:
        _, args, kw, n, nlin = CASES[NAMES.index(name)]
        prob = ref.problem(*args, **kw)
        if name == "E":
            prob["kern_com"][1] = ref._plain("matern12", 2.0, 0.02)
        _cache[name] = (prob, ref.frames(prob, n, kw["seed"] + 100), nlin, kw["seed"])
    return _cache[name]


def eps(name, S):
    prob, xs, _, seed = case(name)
    return ref.random_eps(prob, xs.shape[0], S, seed + 200)


def rule(got, want):
    """|got - want| against the project's rule 1e-8 max(|want|, 1e-3): (largest difference, bar)"""
    return np.abs(got - want).max() if got.size else 0.0, 1e-8 * max(np.abs(want).max() if want.size else 0.0, 1e-3)
