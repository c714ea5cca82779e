"""HSTU positional encoder (hstu_position): add_position_embeddings and add_timestamp_positional_embeddings, forward and
backward, next to two yardsticks timed in the same process (HIP events, warmed up, --reps calls per window):

  clone   torch.clone of the [rows, D] bf16 tensor: the copy floor of the machine for the bytes every forward must move
  eager   the same arithmetic as torch statements: the index tensors built on the device (repeat_interleave with a known output
          size, no host read), index_select for the forward, index_add_ into an fp32 table gradient for the backward

"/ clone" is a time over the clone's, "eager /" the eager time over the HIP path's (> 1: the HIP path is faster; < 1: eager
wins, and the row says so).  fwd = the call under no_grad (one launch); fwd+g = the call that records for autograd (the timestamp
op also writes its two index vectors and sorts them, as the reference does); bwd = torch.autograd.grad through the retained graph.
Times are HIP-event times of whole calls, launches and allocations included; no kernel trace is taken here.

Shapes: 32 sequences x 512 rows, 8 x 4096, and 32 Zipf(1.2) lengths in [32, 4096], at D = 256 and 1024, bf16 rows, fp32 tables
of 8192 position rows and 2049 timestamp rows, 16 targets per sequence, timestamps spread over 30 days.

    python tools/bench_position.py [--reps 50] [--shapes 32x512,8x4096,zipf] [--dims 256,1024]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hstu_position as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--shapes", default="32x512,8x4096,zipf")
ap.add_argument("--dims", default="256,1024")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_position.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")
K, NT, TARGETS = 8192, 2048, 16
sixty = torch.tensor(60.0, device=dev)

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


print(f"{'op':4s} {'shape':28s} {'D':>5s} {'rows':>6s} {'MB':>6s} | {'clone':>7s} | {'fwd':>7s} {'/ clone':>7s} {'eager':>7s} {'eager /':>7s} | "
      f"{'fwd+g':>7s} | {'bwd':>7s} {'/ clone':>7s} {'eager':>8s} {'eager /':>7s}   (times in us)", flush=True)
for key in a.shapes.split(","):
    name, seq = SHAPES[key]
    lengths = torch.tensor(np.asarray(seq, dtype=np.int64), device=dev)
    B, rows = lengths.numel(), int(lengths.sum())
    offsets = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    offsets[1:] = lengths.cumsum(0)
    targets = torch.full((B,), TARGETS, dtype=torch.int64, device=dev)
    high = (lengths - targets).clamp(max=K - 1)
    rng = torch.Generator(device=dev).manual_seed(7)
    # per sequence ascending timestamps within 30 days of its last row
    dt = torch.randint(0, 30 * 86400, (rows,), device=dev, generator=rng)
    seq_of = torch.repeat_interleave(torch.arange(B, device=dev), lengths, output_size=rows)
    order = torch.argsort(seq_of * (1 << 32) + ((1 << 31) - dt))
    stamps = (1_700_000_000 - dt)[order]

    def index_maps():
        b = torch.repeat_interleave(torch.arange(B, device=dev), lengths, output_size=rows)
        n = torch.arange(rows, device=dev) - offsets[b]
        return b, n

    def pos_idx():
        b, n = index_maps()
        h = high[b]
        return torch.where(n >= h, h, n).clamp(0, K - 1)

    def ts_idx():
        b, n = index_maps()
        h = (lengths - targets)[b]
        p = (h - torch.minimum(n, h)).clamp(0, K - 1)
        d = (stamps[offsets[1:][b] - 1] - stamps).float().clamp(min=1e-6) / sixty   # (a tensor divisor: a true division)
        return p, torch.sqrt(d).to(torch.int32).clamp(0, NT).long()

    for D in (int(d) for d in a.dims.split(",")):
        scale = D ** 0.5
        x = torch.randn(rows, D, device=dev).bfloat16().requires_grad_(True)
        g = torch.randn(rows, D, device=dev).bfloat16()
        pos = (torch.randn(K, D, device=dev) * 0.02).requires_grad_(True)
        ts = (torch.randn(NT + 1, D, device=dev) * 0.02).requires_grad_(True)
        nbytes = rows * D * 2
        t_clone = timeit(lambda: g.clone(), a.reps)

        def hip_pos():
            return P.add_position_embeddings(x, offsets, high, 4096, pos, scale)

        def eager_pos():
            return (x.float() * scale + pos.index_select(0, pos_idx())).to(torch.bfloat16)

        def eager_pos_bwd():
            return (g.float() * scale).to(torch.bfloat16), torch.zeros(K, D, device=dev).index_add_(0, pos_idx(), g.float())

        def hip_ts():
            return P.add_timestamp_positional_embeddings(x, offsets, pos, ts, stamps, 4096, 0, lengths, targets, False, "sqrt")

        def eager_ts():
            p, t = ts_idx()
            return x + (pos.index_select(0, p) + ts.index_select(0, t)).to(torch.bfloat16)

        def eager_ts_bwd():
            p, t = ts_idx()
            gf = g.float()
            return torch.zeros(K, D, device=dev).index_add_(0, p, gf), torch.zeros(NT + 1, D, device=dev).index_add_(0, t, gf)

        for op, hip, eager, eager_bwd, wrt in (("pos", hip_pos, eager_pos, eager_pos_bwd, (x, pos)),
                                               ("ts", hip_ts, eager_ts, eager_ts_bwd, (x, pos, ts))):
            out = hip()
            with torch.no_grad():
                ref = eager()
            assert torch.allclose(out.float(), ref.float(), rtol=2 ** -7, atol=1e-3), op   # the two paths compute one thing
            got = torch.autograd.grad(out, wrt, g, retain_graph=True)[1:]
            want = eager_bwd()[-len(got):]
            for gg, ww in zip(got, want):
                assert torch.allclose(gg, ww, rtol=1e-3, atol=1e-2), op

            def fwd_nograd():
                with torch.no_grad():
                    return hip()

            def eager_nograd():
                with torch.no_grad():
                    return eager()

            t_fwd = timeit(fwd_nograd, a.reps)
            t_efwd = timeit(eager_nograd, a.reps)
            t_fwdg = timeit(hip, a.reps)
            t_bwd = timeit(lambda: torch.autograd.grad(out, wrt, g, retain_graph=True), a.reps)
            t_ebwd = timeit(eager_bwd, a.reps)
            print(f"{op:4s} {name:28s} {D:5d} {rows:6d} {nbytes / 1e6:6.1f} | {t_clone:7.1f} | {t_fwd:7.1f} {t_fwd / t_clone:7.2f} "
                  f"{t_efwd:7.1f} {t_efwd / t_fwd:7.2f} | {t_fwdg:7.1f} | {t_bwd:7.1f} {t_bwd / t_clone:7.2f} {t_ebwd:8.1f} "
                  f"{t_ebwd / t_bwd:7.2f}", flush=True)
