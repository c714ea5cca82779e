"""HSTU norm family (hstu_norm): group norm mul dropout, swish layer norm and RMS norm, forward and backward, each next to the
op of csrc/norm_ops.hip that moves the same row bytes, timed in the same process on the same tensors (HIP events, warmed up,
--reps raw calls per window, bf16, weights bf16):

  gn      triton_group_norm_mul_dropout_fwd / _bwd   against  triton_layer_norm_mul_dropout_fwd / _bwd   (training, p = 0.2)
  swish   triton_swish_layer_norm_fwd / _bwd         against  triton_weighted_layer_norm_fwd / _bwd
  rms     triton_rms_norm_fwd / _bwd                 against  triton_weighted_layer_norm_fwd / _bwd

The baseline is measured twice, before and after the op; "spread" is the difference of its two times and the margin of the
comparison: "slower" means the op took longer than the slower baseline window by more than that spread.  The general layout
of the group norm (no time target) is reported at (H, L) = (6, 12) and (3, 344) against the same baseline.  Times are
HIP-event times of whole calls: launches, allocations and the host work of the Python layer included.

    python tools/bench_norm_family.py [--reps 50] [--rows 16384,32768]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import torch  # noqa: E402

import hstu_norm as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rows", default="16384,32768")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_norm_family.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")
EPS, P, SEED = 1e-5, 0.2, 7
FAST = [(4, 128), (8, 128), (8, 256)]
GENERAL = [(6, 12), (3, 344)]


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


def row(op, phase, layout, rows, h, l, base, new):
    b1 = timeit(base, a.reps)
    t = timeit(new, a.reps)
    b2 = timeit(base, a.reps)
    spread, hi = abs(b1 - b2), max(b1, b2)
    verdict = "slower" if t > hi + spread else "faster" if t < min(b1, b2) - spread else "within"
    print(f"{op + ' ' + phase:10s} {layout:8s} {rows:6d} {h:3d} {l:4d} {h * l:5d} | {b1:7.1f} {b2:7.1f} {spread:6.1f} | {t:7.1f} "
          f"{t / ((b1 + b2) / 2):6.2f}  {verdict}", flush=True)


print(f"{'op':10s} {'layout':8s} {'rows':>6s} {'H':>3s} {'L':>4s} {'D':>5s} | {'base 1':>7s} {'base 2':>7s} {'spread':>6s} | {'new':>7s} "
      f"{'/ base':>6s}  (times in us)", flush=True)
with torch.no_grad():
    for rows in (int(r) for r in a.rows.split(",")):
        for layout, shapes in (("fast", FAST), ("general", GENERAL)):
            for h, l in shapes:
                D = h * l
                bf = lambda *s: torch.randn(*s, device=dev).bfloat16()   # noqa: E731
                x, u, g = bf(rows, D), bf(rows, D), bf(rows, D)
                wd, bd, wh, bh = 1 + 0.1 * bf(D), 0.1 * bf(D), 1 + 0.1 * bf(h), 0.1 * bf(h)
                _, m_ln, r_ln, bD, nw, _ = H.triton_layer_norm_mul_dropout_fwd(x, u, wd, bd, EPS, P, True, False, SEED)
                _, m_gn, r_gn, gD, gH, gw, _ = H.triton_group_norm_mul_dropout_fwd(x, u, wh, bh, EPS, P, True, False, h, l, SEED)
                row("gn", "fwd", layout, rows, h, l,
                    lambda: H.triton_layer_norm_mul_dropout_fwd(x, u, wd, bd, EPS, P, True, False, SEED),
                    lambda: H.triton_group_norm_mul_dropout_fwd(x, u, wh, bh, EPS, P, True, False, h, l, SEED))
                row("gn", "bwd", layout, rows, h, l,
                    lambda: H.triton_layer_norm_mul_dropout_bwd(g, x, u, wd, bd, m_ln, r_ln, bD, nw, EPS, True, P, SEED),
                    lambda: H.triton_group_norm_mul_dropout_bwd(g, x, u, wh, bh, m_gn, r_gn, gD, gH, gw, EPS, True, P, SEED, False,
                                                                h, l))
                if layout != "fast":
                    continue
                _, m_w, r_w, bD, nw = H.triton_weighted_layer_norm_fwd(x, wd, bd, EPS)
                _, m_s, r_s = H.triton_swish_layer_norm_fwd(x, wd, bd, EPS)
                _, r_r = H.triton_rms_norm_fwd(x, wd, EPS)
                base_f = lambda: H.triton_weighted_layer_norm_fwd(x, wd, bd, EPS)   # noqa: E731
                base_b = lambda: H.triton_weighted_layer_norm_bwd(g, x, wd, bd, m_w, r_w, True, EPS, bD, nw)   # noqa: E731
                row("swish", "fwd", "rows", rows, 1, D, base_f, lambda: H.triton_swish_layer_norm_fwd(x, wd, bd, EPS))
                row("swish", "bwd", "rows", rows, 1, D, base_b, lambda: H.triton_swish_layer_norm_bwd(g, x, wd, bd, m_s, r_s))
                row("rms", "fwd", "rows", rows, 1, D, base_f, lambda: H.triton_rms_norm_fwd(x, wd, EPS))
                row("rms", "bwd", "rows", rows, 1, D, base_b, lambda: H.triton_rms_norm_bwd(g, x, wd, r_r))
