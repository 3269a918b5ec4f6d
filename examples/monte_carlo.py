#!/usr/bin/env python3
"""A small Monte-Carlo study in ONE batched call: mean |S_vec - ErrVec| against the corruption level q, averaged over a few trials
of Uniform_Topology(100, 0.5, q, 0.1) -- the shape of the figures the DESC paper draws (error against q on graphs of 100-200 nodes).

    python examples/monte_carlo.py [--trials 5] [--n 100] [--iters 100]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from desc_amd import ConstantStepSize, DESC_PGD_batch, Uniform_Topology  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    qs = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5]
    models = [Uniform_Topology(a.n, 0.5, q, 0.1, "uniform", seed=1000 * k + t) for k, q in enumerate(qs) for t in range(a.trials)]
    t0 = time.perf_counter()
    S = DESC_PGD_batch(models, dict(iters=a.iters, Gradient=ConstantStepSize(0.01), seed=0, verbose=False))
    ms = (time.perf_counter() - t0) * 1e3
    err = np.array([np.abs(s - mo.ErrVec).mean() for s, mo in zip(S, models)]).reshape(len(qs), a.trials)
    print(f"{len(models)} problems (n = {a.n}, {a.trials} trials per q) in one DESC_PGD_batch call: {ms:.1f} ms")
    print("    q   mean |S_vec - ErrVec|   (min .. max over the trials)")
    for q, row in zip(qs, err):
        print(f" {q:4.2f}   {row.mean():.4f}                ({row.min():.4f} .. {row.max():.4f})")


if __name__ == "__main__":
    main()
