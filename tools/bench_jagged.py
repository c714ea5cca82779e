"""Jagged concat (hstu_cuda_ops.jagged_2D_tensor_concat): forward and backward times next to two yardsticks timed in the same
process (HIP events, warmed up, --reps calls per window):

  clone   torch.clone of a contiguous tensor of the merged size: the copy ceiling of the machine for these bytes
  eager   the same concat as torch statements: per-sample slices into one torch.cat; the slice bounds are host integers, so
          no sync is charged to it.  Its backward is what autograd makes of those statements.
  launch  the C-ABI call alone, into a pre-allocated output (torch.ops.hstu_cuda_ops.concat_2D_jagged_tensors_forward)

"/ clone" is the time over the clone's (1.0 = the ceiling), "eager /" the eager time over the kernel path's (> 1: faster than
eager).  The forward time is the whole call (the sum of the offsets, the output allocation, one launch); the backward times
are torch.autograd.grad through the retained graph, for the kernel path (n allocations, one launch) and for the eager one.  TB/s counts the merged bytes once read and once
written.

Shapes: the attention configurations of tools/bench_hstu_fp8.py -- 32 samples x 512 rows, 8 x 4096, and the 32 Zipf(1.2)
lengths in [32, 4096] -- at D = 256 and 1024, bf16.  n = 2 splits every sample into item and action halves; n = 9 puts 8
contextual features of 0 or 1 rows in front of the full-length sequence.

    python tools/bench_jagged.py [--reps 50] [--shapes 32x512,8x4096,zipf] [--dims 256,1024]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hstu_cuda_ops import jagged_2D_tensor_concat  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--shapes", default="32x512,8x4096,zipf")
ap.add_argument("--dims", default="256,1024")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_jagged.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")

SHAPES = {
    "32x512": ("32 x 512", [512] * 32),
    "8x4096": ("8 x 4096", [4096] * 8),
    "zipf": ("zipf(1.2) 32 in [32, 4096]", np.clip(np.random.default_rng(1).zipf(1.2, 32) + 31, 32, 4096)),
}


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def tensor_lengths(seq, n):
    """[n, B] lengths of the n tensors"""
    seq = np.asarray(seq, dtype=np.int64)
    if n == 2:
        return np.stack([(seq + 1) // 2, seq // 2])
    ctx = np.random.default_rng(2).integers(0, 2, size=(n - 1, len(seq)))
    return np.concatenate([ctx, seq[None, :]], 0)


print(f"{'shape':28s} {'n':>2s} {'D':>5s} {'rows':>6s} {'MB':>6s} | {'clone':>8s} {'launch':>8s} | {'fwd':>8s} {'TB/s':>5s} {'/ clone':>7s} {'eager':>8s} "
      f"{'eager /':>7s} | {'bwd':>8s} {'TB/s':>5s} {'/ clone':>7s} {'eager':>8s} {'eager /':>7s}   (times in us)", flush=True)
for key in a.shapes.split(","):
    name, seq = SHAPES[key]
    for n in (2, 9):
        L = tensor_lengths(seq, n)
        B = L.shape[1]
        off = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(L, 1)], 1)
        moff = off.sum(0)
        offsets = [torch.tensor(o, dtype=torch.int64, device=dev) for o in off]
        max_seqlens = [int(r.max()) for r in L]
        for D in (int(d) for d in a.dims.split(",")):
            values = [torch.randn(int(r.sum()), D, device=dev).bfloat16().requires_grad_(True) for r in L]
            total = int(L.sum())
            nbytes = total * D * 2
            g = torch.randn(total, D, device=dev).bfloat16()
            plain = [v.detach() for v in values]

            # host integers for the eager slices: the yardstick pays for its launches, not for numpy scalars
            lo, ln = off.tolist(), L.tolist()
            starts = [[int(moff[b]) + sum(ln[u][b] for u in range(t)) for b in range(B)] for t in range(n)]

            def eager_fwd():
                return torch.cat([plain[t][lo[t][b]:lo[t][b + 1]] for b in range(B) for t in range(n)], 0)

            def split_g():
                return [torch.cat([g[starts[t][b]:starts[t][b] + ln[t][b]] for b in range(B)], 0) for t in range(n)]

            out, _ = jagged_2D_tensor_concat(values, offsets, max_seqlens)
            assert torch.equal(out, eager_fwd())
            grads = torch.autograd.grad(out, values, g, retain_graph=True)
            assert all(torch.equal(x, y) for x, y in zip(grads, split_g()))
            eager_out = torch.cat([values[t][lo[t][b]:lo[t][b + 1]] for b in range(B) for t in range(n)], 0)
            buf, moff_t = torch.empty_like(out), torch.stack(offsets).sum(0)
            raw = torch.ops.hstu_cuda_ops.concat_2D_jagged_tensors_forward
            t_clone = timeit(lambda: g.clone(), a.reps)
            t_fwd = timeit(lambda: jagged_2D_tensor_concat(values, offsets, max_seqlens), a.reps)
            t_efwd = timeit(eager_fwd, a.reps)
            t_bwd = timeit(lambda: torch.autograd.grad(out, values, g, retain_graph=True), a.reps)
            t_ebwd = timeit(lambda: torch.autograd.grad(eager_out, values, g, retain_graph=True), a.reps)
            t_raw = timeit(lambda: raw(plain, offsets, 1, 1, 1, 1, 1, moff_t, buf, moff_t), a.reps)
            tbs = lambda us: 2 * nbytes / (us * 1e-6) / 1e12   # noqa: E731
            print(f"{name:28s} {n:2d} {D:5d} {total:6d} {nbytes / 1e6:6.1f} | {t_clone:8.1f} {t_raw:8.1f} | {t_fwd:8.1f} {tbs(t_fwd):5.2f} "
                  f"{t_fwd / t_clone:7.2f} {t_efwd:8.1f} {t_efwd / t_fwd:7.2f} | {t_bwd:8.1f} {tbs(t_bwd):5.2f} "
                  f"{t_bwd / t_clone:7.2f} {t_ebwd:8.1f} {t_ebwd / t_bwd:7.2f}", flush=True)
