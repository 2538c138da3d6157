"""Cases for the activations' product on the float64 matrix cores (afar.hip afar_prod_kernel), shared by
test_afar_mfma_cases_cpu.py (the host check that every case still reaches what it is listed for) and test_gpu_afar_mfma.py.
The problems are built the way test_gpu_afar._problem builds its own (num_partials = 3, seed 5, lengthscale in inducing
spacings); P <= 2 and strips of 2^20 to 1.2 * 2^20 entries.  What the kernel can get wrong that the older layouts do not reach:
row-tile counts that are no multiple of 2 or 4, a single tile, every count of near tiles from 0 to 5 (two are kept in
registers, the others are read again per row tile), near ranges that begin off a multiple of 64, and the skip of the tiles of
W above the diagonal."""
import numpy as np

import afar_rule as af

FS = 16000.0

# nk: near-row counts the case must reach (others may occur); kbeg: range starts it must reach; crowd: (nk, groups that have it)
CASES = {
    "one_tile_16x65536": dict(N=65536, M=16, P=1, ls=8, nk={0, 16}),                      # the diagonal tile is the only tile
    "three_tiles_48x22016": dict(N=22016, M=48, P=1, ls=8, nk={0, 16}),
    "five_tiles_80x13312": dict(N=13312, M=80, P=1, ls=8, nk={16, 32}),
    "crowded_272x4096": dict(N=4096, M=272, P=1, ls=8, nk={32}, crowd=(32, 15)),          # 17 row tiles
    "steps_240x4608": dict(N=4608, M=240, P=1, ls=8, z=(1.7, {0: 48, 2: 64, 5: 16, 9: 32, 12: 80}),
                           nk={0, 16, 32, 48, 64, 80}, kbeg={48, 112, 128, 160}),
    "two_gps_48x22016": dict(N=22016, M=48, P=2, ls=[8, 20], nk={0, 16}),                 # item indexing
}


def problem(N, M, P, ls, z=None, seed=5, **_):
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=3, seed=seed)
    lss = ls if isinstance(ls, list) else [ls] * P
    for p in range(P):
        unit = (N / float(M)) / FS
        if z is not None:
            step, per = z
            zz = np.concatenate([(g * 256 + 0.37 + step * np.arange(k)) / FS for g, k in sorted(per.items())])
            assert zz.shape[0] == M
            prob["za"][p] = zz.reshape(-1, 1).copy()
            unit = step / FS
        prob["kern_act"][p]["lengthscales"] = lss[p] * unit
    return prob


def case_ranges(prob, p):
    return af.ranges(np.ravel(prob["za"][p]), np.ravel(prob["x"]))
