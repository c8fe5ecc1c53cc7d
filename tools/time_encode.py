#!/usr/bin/env python3
"""normalise + encode of N rows alone (one GPU): where the last millisecond of the step goes.

The encode both ways -- PG_ENCODE_FUSED=1, the eval-mode encoder folded into one affine map and run by ONE kernel
(pg_affine_rows), and PG_ENCODE_FUSED=0, the layers (cat, two 512-wide fp32 GEMMs, two BatchNorm passes, two identity
activations, l_mu) -- then the parts of the fused form (the fold, the kernel) and, as the yardstick of a kernel that is bound
by reading its inputs, a plain device copy of the same bytes."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from pangaea_amd import _lib  # noqa: E402
from pangaea_amd.data import Data  # noqa: E402
from pangaea_amd.models.VAENET import VAENET  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000
dev = torch.device("cuda:0")
abd = torch.randint(0, 50, (n, 400), dtype=torch.int32, device=dev)
tnf = torch.randint(0, 500, (n, 136), dtype=torch.int32, device=dev)
names = np.arange(n)
torch.manual_seed(1)
vae = VAENET(400, 136, 32, 30, 1, True, 1, 0.005, 0.2, 0.1, 0.015, 0.0001)
vae.network.eval()


def timed(f, reps=20):
    f(); torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def encode(fused: str):
    os.environ["PG_ENCODE_FUSED"] = fused
    return vae.encode(d)


d = Data(names, abd, tnf)
print(f"Data (normalise + weights): {timed(lambda: Data(names, abd, tnf)):.3f} ms")
for _ in range(2):                  # (twice: the second pair is free of first-call costs of either form)
    print(f"encode, layers (PG_ENCODE_FUSED=0): {timed(lambda: encode('0')):.3f} ms")
    print(f"encode, fused  (PG_ENCODE_FUSED=1): {timed(lambda: encode('1')):.3f} ms")
mu0, mu1 = encode("0"), encode("1")
print(f"max |mu_fused - mu_layers| = {float((mu1 - mu0).abs().max()):.3e} at max |mu| = {float(mu0.abs().max()):.3e}")
with torch.no_grad():
    print(f"fold alone (affine_encoder): {timed(vae.network.affine_encoder):.3f} ms")
    w, b = vae.network.affine_encoder()
    out = torch.empty((n, 32), dtype=torch.float32, device=dev)
    L = _lib.load()

    def kernel():
        _lib.check(L.pg_affine_rows(d.abd_dev.data_ptr(), 400, d.tnf_dev.data_ptr(), 136, n, w.data_ptr(), b.data_ptr(), 32, out.data_ptr(), None))
    t_kernel = timed(kernel, 50)
    x = torch.cat([d.abd_dev, d.tnf_dev], dim=1)
    y = torch.empty_like(x)
    t_copy = timed(lambda: y.copy_(x), 50)
    mb = x.numel() * 4 / 1e6
    print(f"pg_affine_rows alone: {t_kernel:.4f} ms ({mb / t_kernel / 1e3:.2f} TB/s of input read)")
    print(f"device copy of the same {mb:.0f} MB: {t_copy:.4f} ms (read + write; kernel / copy = {t_kernel / t_copy:.2f})")
    wl = torch.randn(536, 512, device=dev)
    print(f"one {n} x 536 x 512 fp32 matmul: {timed(lambda: x @ wl):.3f} ms")
