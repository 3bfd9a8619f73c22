"""Generate tests/golden/cor_loss.npz by running the REFERENCE's `cor_loss` on the CPU (this container only).

    python tools/make_cor_golden.py

The reference's model/help/loss.py is loaded by path, unmodified (it imports torch only); the fixture holds inputs
and the reference's outputs.  Per case c in A..D:

    {c}.X        float32 [n, D]     the input
    {c}.K        int                factor_k
    {c}.loss64 / {c}.grad64         the reference function and its autograd gradient evaluated in float64
    {c}.loss32 / {c}.grad32         the same in float32 (loss32, grad32 stored as float64 / float32)

The float64 values are the yardstick; the float32 values record the reference's own fp32 error (its matmul form of
|x_i - x_j|^2 cancels on the diagonal), which is the bar the kernels are held to.  The achieved errors of the fp32
reference are printed."""
import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REF_LOSS = "/root/reference/model/help/loss.py"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "cor_loss.npz")


def cases():
    import torch
    g = torch.Generator().manual_seed(20260)
    rn = lambda *s: torch.randn(*s, generator=g)
    out = {"A": (rn(7, 8), 2), "B": (0.1 * rn(129, 32), 8)}
    out["C"] = (torch.nn.functional.normalize(rn(100, 64), dim=1) * 0.5 + 0.01 * rn(100, 64), 4)      # embedding-like
    X = 0.02 * rn(96, 256)
    X[:, 64:128] = 0.7 * X[:, :64] + 0.3 * X[:, 64:128]                                              # correlated factors
    out["D"] = (X, 4)
    return out


def main():
    import torch
    spec = importlib.util.spec_from_file_location("reference_loss", REF_LOSS)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    fx = {}
    for name, (X, K) in cases().items():
        X = X.float().contiguous()
        D = X.shape[1]
        fx[f"{name}.X"], fx[f"{name}.K"] = X.numpy().copy(), np.int64(K)
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            x = X.to(dt).clone().requires_grad_(True)
            loss = ref.cor_loss(torch.split(x, D // K, dim=1), K)
            loss.backward()
            fx[f"{name}.loss{tag}"] = np.float64(float(loss.detach()))
            fx[f"{name}.grad{tag}"] = x.grad.numpy().copy()
        dl = abs(fx[f"{name}.loss32"] - fx[f"{name}.loss64"])
        dg = np.abs(fx[f"{name}.grad32"].astype(np.float64) - fx[f"{name}.grad64"]).max()
        print(f"{name}: n={X.shape[0]} D={D} K={K} loss64={fx[f'{name}.loss64']:.9f} |loss32-loss64|={dl:.3e} "
              f"max|grad32-grad64|={dg:.3e} max|grad64|={np.abs(fx[f'{name}.grad64']).max():.3e}")
    np.savez_compressed(OUT, **fx)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
