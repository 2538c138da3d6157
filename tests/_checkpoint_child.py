"""child of tests/test_gpu_checkpoint.py::test_another_process_continues_the_file: a fresh process loads a checkpoint,
runs one more optimize() call and saves the model (and the call's fun / jac / x beside it)

    python _checkpoint_child.py IN.npz OUT.npz MAXITER"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import gpitch_amd
    from gpitch_amd.train import AdamOptimizer
    src, out, maxiter = sys.argv[1], sys.argv[2], int(sys.argv[3])
    m = gpitch_amd.load(src)
    res = m.optimize(method=AdamOptimizer(0.01), maxiter=maxiter)
    gpitch_amd.save(out, m)
    np.savez(out + ".result.npz", fun=np.float64(res.fun), jac=res.jac, x=res.x)


if __name__ == "__main__":
    main()
