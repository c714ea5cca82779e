"""Delta-q backward (hstu_varlen_bwd_kv: the queries are the last Lq of every sequence's Lk keys) against the workaround it
replaces -- the self-attention backward on q / dout padded with zero rows up to Lk (hstu_varlen_bwd with its P / dS exchange, the
default path of a training call; the self-attention kernels are the same instructions as before the delta-q mode existed).
Backward only, causal mask, median of --reps timed calls after --warmup.
    python tools/bench_hstu_delta_q.py [--batch 8] [--lk 4096] [--heads 4] [--reps 20] > profiles/hstu_delta_q_bwd.txt"""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd")); sys.path.insert(0, ROOT)
import torch
from hstu import hstu_varlen_bwd, hstu_varlen_bwd_kv

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8); ap.add_argument("--lk", type=int, default=4096); ap.add_argument("--heads", type=int, default=4)
ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
dev = torch.device("cuda")
B, Lk, H = a.batch, a.lk, a.heads


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


print(f"delta-q backward vs padded self-attention backward: {B} sequences, Lk {Lk}, H {H}, causal, bf16; ms = median (min .. max) of {a.reps}")
for d in (256, 128):
    for Lq in (Lk // 8, Lk):
        g = torch.Generator(device=dev); g.manual_seed(d + Lq)
        mk = lambda n: torch.randn(n, H, d, device=dev, generator=g).mul_(0.5).to(torch.bfloat16)
        q, dout, k, v = mk(B * Lq), mk(B * Lq), mk(B * Lk), mk(B * Lk)
        cu_q = torch.arange(0, B * Lq + 1, Lq, dtype=torch.int32, device=dev)
        cu_k = torch.arange(0, B * Lk + 1, Lk, dtype=torch.int32, device=dev)
        qp, dp = torch.zeros(B, Lk, H, d, dtype=torch.bfloat16, device=dev), torch.zeros(B, Lk, H, d, dtype=torch.bfloat16, device=dev)
        qp[:, Lk - Lq:] = q.view(B, Lq, H, d); dp[:, Lk - Lq:] = dout.view(B, Lq, H, d)
        qp, dp = qp.view(B * Lk, H, d), dp.view(B * Lk, H, d)
        alpha = 1.0 / d ** 0.5
        new = lambda: hstu_varlen_bwd_kv(dout, q, k, v, cu_q, cu_k, Lq, Lk, Lk, None, None, 1, -1, 0, alpha)
        pad = lambda: hstu_varlen_bwd(dp, qp, k, v, cu_k, Lk, Lk, None, None, 1, True, alpha)
        r_new, r_pad = new(), pad()
        torch.cuda.synchronize()
        err = max(float((x.float() - y.float()).abs().max()) for x, y in ((r_new[0], r_pad[0].view(B, Lk, H, d)[:, Lk - Lq:].reshape(B * Lq, H, d)),
                                                                          (r_new[1], r_pad[1]), (r_new[2], r_pad[2])))
        del r_new, r_pad
        tn, tp = timed(new), timed(pad)
        print(f"d {d:3d}  Lq {Lq:4d}: delta-q {tn[0]:7.3f} ({tn[1]:.3f} .. {tn[2]:.3f})   padded {tp[0]:7.3f} ({tp[1]:.3f} .. {tp[2]:.3f})   "
              f"padded / delta-q {tp[0] / tn[0]:5.2f} x   max |difference| of dq / dk / dv {err:.2e}")
