"""FP8 HSTU attention: quantiser and forward times per quant_mode next to the bf16 forward (one process, HIP events); with
--bwd, quantize_for_backward and varlen_bwd per quant_mode next to the bf16 backward instead.

Shapes: C3 (32 x 512, H 4, d 256), dense 8 x 4096 at d 128 and 256, and bench.py's jagged C4 (32 Zipf(1.2) lengths in
[32, 4096], H 4, d 256); all causal, alpha 1 / sqrt(d).  TFLOP/s use bench.hstu_flops (the reference's FLOP model).  The
quantisers' rate counts the bytes of one pass over q, k and v (2 bytes read + 1 written per element) against 8 TB/s;
modes 3 / 4 / 5 read their input twice (amax, then cast), so their true traffic is 5/3 of the counted one.

The backward's TFLOP/s count 2.5 x the forward's FLOPs (five GEMMs to two), however many GEMMs a kernel recomputes.

    python tools/bench_hstu_fp8.py [--reps 10] [--shapes c3,8x4096_d128,8x4096_d256,c4] [--bwd]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import hstu  # noqa: E402
from hstu import hstu_fp8, hstu_varlen_bwd, hstu_varlen_fwd  # noqa: E402

HBM_PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--shapes", default="c3,8x4096_d128,8x4096_d256,c4")
ap.add_argument("--bwd", action="store_true", help="time the FP8 backward (quantize_for_backward, varlen_bwd) instead")
a = ap.parse_args()
dev = torch.device("cuda")


def timeit(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps   # ms


SHAPES = {
    "c3": ("C3 dense 32 x 512, d 256", [512] * 32, 256),
    "8x4096_d128": ("dense 8 x 4096, d 128", [4096] * 8, 128),
    "8x4096_d256": ("dense 8 x 4096, d 256", [4096] * 8, 256),
    "c4": ("C4 jagged zipf(1.2) 32 seq, d 256", np.clip(np.random.default_rng(1).zipf(1.2, 32) + 31, 32, 4096), 256),
}

for key in a.shapes.split(","):
    name, lengths, d = SHAPES[key]
    H = 4
    lengths = [int(x) for x in lengths]
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32, device=dev)
    T, L = int(cu[-1]), max(lengths)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    q, k, v = (torch.empty(T, H, d, device=dev).uniform_(-1, 1, generator=g).bfloat16() for _ in range(3))
    alpha = 1.0 / d ** 0.5
    fl = bench.hstu_flops(lengths, H, d)
    qbytes = 3.0 * T * H * d * 3
    if a.bwd:
        dout = torch.empty(T, H, d, device=dev).uniform_(-1, 1, generator=g).bfloat16()
        fb = 2.5 * fl
        tb = timeit(lambda: hstu_varlen_bwd(dout, q, k, v, cu, L, L, None, None, 1, True, alpha), a.reps)
        print(f"{name:36s} tokens {T:6d}  bf16 bwd {tb * 1e3:8.1f} us {fb / tb / 1e9:6.0f} TF", flush=True)
        for mode in range(6):
            tq = timeit(lambda: hstu_fp8.quantize_for_backward(q, k, v, dout, cu, mode), a.reps)
            kw = hstu_fp8.quantize_for_backward(q, k, v, dout, cu, mode)
            tf = timeit(lambda: hstu.varlen_bwd(dq=None, dk=None, dv=None, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=L,
                                                max_seqlen_k=L, scaling_seqlen=L, num_contexts=None, num_targets=None,
                                                target_group_size=1, window_size_left=-1, window_size_right=0, alpha=alpha,
                                                quant_mode=mode, **kw), a.reps)
            print(f"{'':36s} mode {mode}: quantise q,k,v,dout {tq * 1e3:8.1f} us   fp8 bwd {tf * 1e3:8.1f} us "
                  f"{fb / tf / 1e9:6.0f} TF  ({tb / tf:4.2f} x bf16)", flush=True)
        continue
    tb = timeit(lambda: hstu_varlen_fwd(q, k, v, cu, L, L, None, None, 1, True, alpha), a.reps)
    print(f"{name:36s} tokens {T:6d}  bf16 fwd {tb * 1e3:8.1f} us {fl / tb / 1e9:6.0f} TF", flush=True)
    for mode in range(6):
        tq = timeit(lambda: hstu_fp8.quantize_qkv(q, k, v, cu, mode), a.reps)
        kw = hstu_fp8.quantize_qkv(q, k, v, cu, mode)
        tf = timeit(lambda: hstu.varlen_fwd(cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=L, max_seqlen_k=L, scaling_seqlen=L,
                                            num_contexts=None, num_targets=None, target_group_size=1, window_size_left=-1,
                                            window_size_right=0, alpha=alpha, rab=None, func=None, quant_mode=mode, **kw),
                    a.reps)
        bw = qbytes / (tq * 1e-3)
        print(f"{'':36s} mode {mode}: quantise q,k,v {tq * 1e3:8.1f} us {bw / 1e12:5.2f} TB/s ({100 * bw / HBM_PEAK:4.1f} % of HBM "
              f"peak)   fp8 fwd {tf * 1e3:8.1f} us {fl / tf / 1e9:6.0f} TF  ({tb / tf:4.2f} x bf16)", flush=True)
