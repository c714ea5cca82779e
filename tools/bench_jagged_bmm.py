"""Jagged x dense product with bias (hstu_jagged.triton_jagged_dense_bmm_broadcast_add): forward and forward + backward times
next to the torch composition timed in the same process (HIP events, warmed up, --windows windows of --reps calls each, the two
paths alternating window by window; the median window is reported with the spread (max - min) / median of the windows):

  torch   scatter the jagged rows into a zero-padded [B, max_len, K] (index_copy_ with a precomputed index: no host sync is
          charged to it), torch.baddbmm with the bias, gather the rows back (index_select).  Its backward is what autograd
          makes of those statements.
  hip     the function of this package: one launch forward; two GEMM launches and the column sum backward.

"torch /" is the torch time over the hip time (> 1: hip is faster).  TF/s counts 2 rows K N per GEMM: one forward, three in
forward + backward; the padded rows the torch path multiplies are not counted for either side.  The outputs and gradients of
the two paths are compared before anything is timed.

Shapes: B = 32, the 32 Zipf(1.2) lengths in [32, 4096] of tools/bench_jagged.py and 32 x 512 rows, K = N in {128, 256, 512}, bf16.

    python tools/bench_jagged_bmm.py [--reps 200] [--windows 5] [--shapes zipf,32x512] [--dims 128,256,512]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hstu_jagged import triton_jagged_dense_bmm_broadcast_add  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--shapes", default="zipf,32x512")
ap.add_argument("--dims", default="128,256,512")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_jagged_bmm.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")

SHAPES = {
    "zipf": ("zipf(1.2) 32 in [32, 4096]", np.clip(np.random.default_rng(1).zipf(1.2, 32) + 31, 32, 4096)),
    "32x512": ("32 x 512", [512] * 32),
}


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def alternate(fns, reps, windows):
    """median and spread of each function's windows; the functions take turns"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            times[i].append(window(fn, reps))
    return [(statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for t in times]


print(f"{'shape':28s} {'K=N':>4s} {'rows':>6s} {'padded':>7s} | {'fwd hip':>8s} {'+-':>4s} {'TF/s':>6s} {'torch':>8s} {'+-':>4s} {'torch /':>7s} | "
      f"{'f+b hip':>8s} {'+-':>4s} {'TF/s':>6s} {'torch':>8s} {'+-':>4s} {'torch /':>7s}   (times in us)", flush=True)
for key in a.shapes.split(","):
    name, lengths = SHAPES[key]
    lengths = [int(v) for v in lengths]
    B, L, max_len = len(lengths), sum(lengths), max(lengths)
    off = np.concatenate([[0], np.cumsum(lengths)])
    offsets = torch.tensor(off, dtype=torch.int64, device=dev)
    idx = torch.tensor(np.concatenate([b * max_len + np.arange(n) for b, n in enumerate(lengths)]), dtype=torch.int64, device=dev)
    for KN in (int(d) for d in a.dims.split(",")):
        K = N = KN
        jagged = torch.randn(L, K, device=dev).bfloat16().requires_grad_(True)
        dense = (torch.randn(B, K, N, device=dev) / K ** 0.5).bfloat16().requires_grad_(True)
        bias = torch.randn(B, N, device=dev).bfloat16().requires_grad_(True)
        g = torch.randn(L, N, device=dev).bfloat16()
        leaves = [jagged, dense, bias]

        def hip_fwd():
            return triton_jagged_dense_bmm_broadcast_add(max_len, offsets, jagged, dense, bias)

        def torch_fwd():
            padded = jagged.new_zeros(B * max_len, K).index_copy(0, idx, jagged).view(B, max_len, K)
            return torch.baddbmm(bias[:, None, :], padded, dense).view(B * max_len, N).index_select(0, idx)

        def hip_both():
            return torch.autograd.grad(hip_fwd(), leaves, g)

        def torch_both():
            return torch.autograd.grad(torch_fwd(), leaves, g)

        # faster and different is not faster: the two paths agree to the rounding of bf16 before anything is timed
        with torch.no_grad():
            torch.testing.assert_close(hip_fwd().float(), torch_fwd().float(), rtol=2 ** -6, atol=2 ** -6)
        for x, y in zip(hip_both(), torch_both()):
            torch.testing.assert_close(x.float(), y.float(), rtol=2 ** -5, atol=2 ** -5 * float(y.float().abs().max()))
        with torch.no_grad():
            (hf, hfs), (tf, tfs) = alternate([hip_fwd, torch_fwd], a.reps, a.windows)
        (hb, hbs), (tb, tbs) = alternate([hip_both, torch_both], a.reps, a.windows)
        flops = 2.0 * L * K * N
        print(f"{name:28s} {KN:4d} {L:6d} {B * max_len:7d} | {hf:8.1f} {hfs:4.2f} {flops / hf / 1e6:6.1f} {tf:8.1f} {tfs:4.2f} {tf / hf:7.2f} | "
              f"{hb:8.1f} {hbs:4.2f} {3 * flops / hb / 1e6:6.1f} {tb:8.1f} {tbs:4.2f} {tb / hb:7.2f}", flush=True)
