#!/usr/bin/env python3
"""A params.Gradient plugin of your own: heavy-ball momentum, written once with NumPy and once with torch on the GPU.

DESC_PGD.m:207 reads  wijk = wijk + params.Gradient.GetStep(grad_long)  for any handle object with a GetStep method.  Objects other
than the three classes of desc_amd.stepsize are called once per iteration, between the library's gradient pass and its apply pass:
  - by default with a NumPy float64 array of m_cycle entries, returning one (two 8 m_cycle-byte copies per iteration: slow, works
    everywhere);
  - with the class attribute device_tensors = True with a float64 torch tensor on the solver's GPU (read-only), returning a tensor of
    the same dtype, device and length: no per-cycle data leaves the device.

    python examples/custom_step.py
"""
import os
import sys
import time

import numpy as np
import torch          # before desc_amd loads its library: a process holds one ROCm runtime, and torch needs its own

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from desc_amd import DESC_PGD  # noqa: E402
from desc_amd.models import Uniform_Topology  # noqa: E402


class Momentum:
    """v = mu v - lr g; step = v."""

    def __init__(self, lr=0.01, mu=0.9):
        self.lr, self.mu, self.v = lr, mu, None

    def GetStep(self, grad):
        self.v = -self.lr * grad if self.v is None else self.mu * self.v - self.lr * grad
        return self.v


class MomentumOnDevice(Momentum):
    device_tensors = True          # grad is a torch.float64 tensor on cuda:<device>; the same two lines run as torch ops


def main():
    mo = Uniform_Topology(1000, 0.5, 0.3, 0.1, "uniform", seed=0)
    for name, G in (("NumPy plugin", Momentum()), ("torch plugin, device mode", MomentumOnDevice())):
        t0 = time.perf_counter()
        S_vec, info = DESC_PGD(mo.Ind, mo.RijMat, dict(iters=100, Gradient=G, verbose=False), return_info=True)
        dt = time.perf_counter() - t0
        print(f"{name:26s} iterations {info['iters_run']:3d}  mean|S_vec - ErrVec| = {np.mean(np.abs(S_vec - mo.ErrVec)):.5f}  "
              f"objective {info['obj'][-1]:.3f}  {dt:.2f} s  (m_cycle = {info['m_cycle']})")


if __name__ == "__main__":
    main()
