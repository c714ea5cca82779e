"""Softmax attention backward (softmax_attn._backward: dq, dk, dv in two launches) next to the backward of
torch.nn.functional.scaled_dot_product_attention on the same device and the same random data, timed in one process: HIP
events, every shape warmed up, --windows windows per path with the paths alternating window by window, the median window
reported with the spread (max - min) / median.  The BACKWARD ALONE is timed on both sides: the forward results (out, lse /
the autograd graph) are made once, outside the windows.

  sdpa    torch.autograd.grad through a retained graph of F.scaled_dot_product_attention (q / k / v as [B, H, S, D] views,
          is_causal=True, enable_gqa=True when Hkv < Hq; or attn_mask = the dense boolean mask of the arbitrary function).
  hip     mi355_softmax_attn_bwd with preallocated dq / dk / dv.

The shapes are those of tools/bench_prefill_attn.py.  "TF/s" counts 7 GEMMs (14 D flops) per VISIBLE (query, key) pair per
query head over the hip time -- the two-pass design recomputes S and dP, so it executes 7 products where a one-pass backward
executes 5 --; "of 1900" is that rate over the 1 900 TFLOP/s sustained bf16 MFMA rate (tools/ubench_mfma.hip); "sdpa /" is the
sdpa time over the hip time (> 1: hip is faster).  The gradients of the two paths are compared before anything is timed.

    python tools/bench_softmax_attn_bwd.py [--windows 3] [--quick]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import softmax_attn as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--window-ms", type=float, default=20.0, help="device time one timing window aims at")
ap.add_argument("--quick", action="store_true", help="the smallest dense shape and a 2048-token arbitrary batch only")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_softmax_attn_bwd.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")
HQ = 16
MFMA_TFLOPS = 1900.0


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def alternate(fns, windows):
    """median and spread of each function's windows; the functions take turns; repetitions sized from a first estimate"""
    reps = []
    for fn in fns:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        reps.append(max(3, min(500, int(a.window_ms * 1e3 / max(window(fn, 3), 1.0)))))
    times = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            times[i].append(window(fn, reps[i]))
    return [(statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for t in times]


def make(B, S_, Hkv, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(dev).bfloat16()   # noqa: E731
    return r(B, S_, HQ, D), r(B, S_, Hkv, D), r(B, S_, Hkv, D), r(B, S_, HQ, D)


def sdpa_graph(q, k, v, **kw):
    """the retained autograd graph of one SDPA forward: -> (out, leaves)"""
    leaves = tuple(t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ql, kl, vl = leaves
    o = F.scaled_dot_product_attention(ql.transpose(1, 2), kl.transpose(1, 2), vl.transpose(1, 2),
                                       enable_gqa=k.shape[2] != q.shape[2], **kw)
    return o.transpose(1, 2), leaves


def close(got, want, what):
    """faster and different is not faster: the two paths agree to the rounding of bf16, on the scale of each tensor"""
    for g, w, n in zip(got, want, ("dq", "dk", "dv")):
        g, w = g.float(), w.float()
        tol = 2.0 ** -6 * w.abs() + 2.0 ** -6 * max(1.0, float(w.abs().max()))
        worst = float(((g - w).abs() / tol).max())
        assert worst <= 1.0, f"{what}: {n} differs from sdpa's, worst |diff| / tolerance {worst:.2f}"


def hip_backward(q, k, v, do, mask, func, skip=True):
    """-> a closure that runs the backward alone, and its (dq, dk, dv)"""
    scale = 1.0 / math.sqrt(q.shape[-1])
    if func is not None:
        out, lse = S.flash_attn_func(q, k, v, arbitrary=True, aux_tensors=[func], return_lse=True)
    else:
        out, lse = S.flash_attn_func(q, k, v, causal=True, return_lse=True)
    grads = tuple(torch.empty_like(t) for t in (q, k, v))
    fn = lambda: S._backward(q, k, v, out, lse, do, None, None, 0, 0, mask, func, scale, skip_tiles=skip, grads=grads)  # noqa: E731
    return fn, grads


print(f"Hq {HQ}, bf16, random normal q / k / v / dO; backward alone; times in us, median of {a.windows} alternating windows "
      "(+- = (max - min) / median)")
print("dense causal")
print(f"{'B':>3s} {'S':>5s} {'Hkv':>3s} {'D':>4s} | {'hip':>9s} {'+-':>4s} {'sdpa':>10s} {'+-':>4s} {'sdpa /':>6s} | "
      f"{'TF/s':>6s} {'of 1900':>7s}", flush=True)
lost = []
dense = [(8, 512), (8, 2048), (2, 8192)] if not a.quick else [(8, 512)]
for D in (64, 128):
    for Hkv in (16, 4):
        for B, S_ in dense:
            q, k, v, do = make(B, S_, Hkv, D, B * 3 + S_ + Hkv * 11 + D)
            hip, grads = hip_backward(q, k, v, do, S.MASK_CAUSAL, None)
            o, leaves = sdpa_graph(q, k, v, is_causal=True)
            ref = lambda: torch.autograd.grad(o, leaves, do, retain_graph=True)   # noqa: E731
            hip()
            close(grads, ref(), f"dense causal B {B} S {S_} Hkv {Hkv} D {D}")
            (h, hs), (t, ts) = alternate([hip, ref], a.windows)
            tf = 14.0 * B * HQ * D * (S_ * (S_ + 1) / 2) / h / 1e6
            print(f"{B:3d} {S_:5d} {Hkv:3d} {D:4d} | {h:9.1f} {hs:4.2f} {t:10.1f} {ts:4.2f} {t / h:6.2f} | "
                  f"{tf:6.1f} {tf / MFMA_TFLOPS:7.3f}", flush=True)
            if t < h:
                lost.append(f"dense causal B {B} S {S_} Hkv {Hkv} D {D}: hip {h:.1f} us, sdpa {t:.1f} us")
            del q, k, v, do, o, leaves, grads

total = 8192 if not a.quick else 2048
g = torch.Generator().manual_seed(5)
lens, rank = [], 1
while sum(lens) < total:   # sequence lengths ~ (total / 4) / rank^1.1, at least 16 tokens each (tools/bench_prefill_attn.py)
    lens.append(min(max(16, int(total / 4 / rank ** 1.1)), total - sum(lens)))
    rank += 1
lens = [lens[i] for i in torch.randperm(len(lens), generator=g).tolist()]
off = torch.tensor([0] + lens).cumsum(0)
pos = torch.arange(total)
start = off[torch.searchsorted(off[1:], pos, right=True)]
func = torch.zeros(1, 1, 3, total + 256, dtype=torch.int32)        # the jagged-causal function: visible(q) = [start, q + 1)
func[0, 0, 1, :total], func[0, 0, 2, :total] = start.int(), (pos + 1).int()
mask = ((pos[None, :] >= start[:, None]) & (pos[None, :] <= pos[:, None]))[None, None].to(dev)
pairs = float(sum(n * (n + 1) // 2 for n in lens))
func = func.to(dev)
print(f"arbitrary, flattened: B 1, {total} tokens in {len(lens)} sequences (longest {max(lens)}), Hkv 4; "
      f"{pairs / (total * (total + 1) / 2):.3f} of the causal pairs are visible")
print(f"{'D':>4s} | {'hip skip':>9s} {'+-':>4s} {'hip all':>9s} {'+-':>4s} {'sdpa mask':>10s} {'+-':>4s} {'sdpa /':>6s} {'all /':>6s} | "
      f"{'TF/s':>6s} {'of 1900':>7s}", flush=True)
for D in (64, 128):
    q, k, v, do = make(1, total, 4, D, 77 + D)
    on, g_on = hip_backward(q, k, v, do, S.MASK_FUNC, func)
    offf, g_off = hip_backward(q, k, v, do, S.MASK_FUNC, func, skip=False)
    o, leaves = sdpa_graph(q, k, v, attn_mask=mask)
    ref = lambda: torch.autograd.grad(o, leaves, do, retain_graph=True)   # noqa: E731
    on()
    offf()
    close(g_on, ref(), f"arbitrary D {D}")
    assert all(torch.equal(x, y) for x, y in zip(g_on, g_off))
    (h, hs), (n, ns), (t, ts) = alternate([on, offf, ref], a.windows)
    tf = 14.0 * HQ * D * pairs / h / 1e6
    print(f"{D:4d} | {h:9.1f} {hs:4.2f} {n:9.1f} {ns:4.2f} {t:10.1f} {ts:4.2f} {t / h:6.2f} {n / h:6.2f} | "
          f"{tf:6.1f} {tf / MFMA_TFLOPS:7.3f}", flush=True)
    if t < h:
        lost.append(f"arbitrary D {D}: hip {h:.1f} us, sdpa {t:.1f} us")
    del q, k, v, do, o, leaves
print(f"shapes where sdpa's backward is faster than hip's: {len(lost)}")
for row in lost:
    print("  lost " + row)
