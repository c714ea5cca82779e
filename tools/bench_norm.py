"""HSTU layer norms (hstu_norm): layer norm and layer-norm-mul-dropout, forward and backward, next to two yardsticks timed
in the same process (HIP events, warmed up, --reps calls per window):

  clone   torch.clone of one [rows, D] bf16 tensor, times the number of row tensors the op must move (ln fwd: x, y = 2;
          ln bwd: dy, x, dx = 3; lmd fwd: x, u, y = 3; lmd bwd: dy, x, u, dx, du = 5; a clone itself moves 2).  "/ floor" is
          the op's time over that floor: 1.0 would be the copy rate of the machine
  eager   the PyTorch-ROCm composition: F.layer_norm (* u, F.dropout) and its autograd backward

"eager /" is the eager time over the HIP path's (> 1: the HIP path is faster; < 1: eager wins, and the row says so).  Times
are HIP-event times of whole calls, launches, allocations and the host work of the Python layer included; no kernel trace is
taken here.  lmd runs with training=True, p = 0.2 (dropout on); rows, weights and gradients are bf16 on both paths.

    python tools/bench_norm.py [--reps 50] [--rows 16384,32768] [--dims 256,1024,4096]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import hstu_norm as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rows", default="16384,32768")
ap.add_argument("--dims", default="256,1024,4096")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_norm.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")
EPS, P = 1e-5, 0.2
SHAPE_NAME = {16384: "32 x 512", 32768: "8 x 4096"}


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


print(f"{'op':8s} {'shape':9s} {'rows':>6s} {'D':>5s} {'MB':>6s} | {'clone':>7s} {'floor':>7s} | {'hip':>7s} {'/ floor':>7s} "
      f"{'eager':>7s} {'eager /':>7s}   (times in us)", flush=True)
for rows in (int(r) for r in a.rows.split(",")):
    for D in (int(d) for d in a.dims.split(",")):
        x = torch.randn(rows, D, device=dev).bfloat16().requires_grad_(True)
        u = torch.randn(rows, D, device=dev).bfloat16().requires_grad_(True)
        g = torch.randn(rows, D, device=dev).bfloat16()
        w = (1 + 0.1 * torch.randn(D, device=dev)).bfloat16().requires_grad_(True)
        b = (0.1 * torch.randn(D, device=dev)).bfloat16().requires_grad_(True)
        t_clone = timeit(lambda: g.clone(), a.reps)

        def hip_ln():
            return H.layer_norm(x, w, b, EPS)

        def eager_ln():
            return F.layer_norm(x, (D,), w, b, EPS)

        def hip_lmd():
            return H.norm_mul_dropout(x, u, w, b, EPS, P, True, seed=7)

        def eager_lmd():
            return F.dropout(F.layer_norm(x, (D,), w, b, EPS) * u, P, True)

        for op, hip, eager, wrt, moved_fwd, moved_bwd in (("ln", hip_ln, eager_ln, (x, w, b), 2, 3),
                                                          ("lmd", hip_lmd, eager_lmd, (x, u, w, b), 3, 5)):
            out, ref = hip(), eager()
            if op == "ln":   # the two paths compute one thing (the dropout streams of lmd differ by design)
                assert torch.allclose(out.float(), ref.float(), rtol=2 ** -6, atol=2 ** -6), op
            got, want = torch.autograd.grad(out, wrt, g, retain_graph=True), torch.autograd.grad(ref, wrt, g, retain_graph=True)
            if op == "ln":
                for gg, ww in zip(got, want):
                    assert torch.allclose(gg.float(), ww.float(), rtol=2 ** -5, atol=1.0), op

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        return fn()
                return run

            for phase, t_hip, t_eager, moved in (
                    ("fwd", timeit(no_grad(hip), a.reps), timeit(no_grad(eager), a.reps), moved_fwd),
                    ("bwd", timeit(lambda: torch.autograd.grad(out, wrt, g, retain_graph=True), a.reps),
                     timeit(lambda: torch.autograd.grad(ref, wrt, g, retain_graph=True), a.reps), moved_bwd)):
                floor = t_clone * moved / 2
                print(f"{op + ' ' + phase:8s} {SHAPE_NAME.get(rows, ''):9s} {rows:6d} {D:5d} {rows * D * 2 / 1e6:6.1f} | {t_clone:7.1f} "
                      f"{floor:7.1f} | {t_hip:7.1f} {t_hip / floor:7.2f} {t_eager:7.1f} {t_eager / t_hip:7.2f}", flush=True)
