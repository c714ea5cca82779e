"""Softmax prefill attention (prefill_attn.flash_attn_func) next to torch.nn.functional.scaled_dot_product_attention on the
same device and the same random data, timed in one process: HIP events, every shape warmed up, --windows windows per path
with the paths alternating window by window, the median window reported with the spread (max - min) / median.

  sdpa    what the reference's TorchSDPAPrefillBackend falls back to without flash-attn: q / k / v as [B, H, S, D] views,
          is_causal=True (enable_gqa=True when Hkv < Hq), or attn_mask = the dense boolean mask of the arbitrary function.
  hip     the function of this package: one launch.

Dense causal: B x S in {8 x 512, 8 x 2048, 2 x 8192}, Hq = 16, Hkv in {16, 4}, D in {64, 128}, bf16.  Arbitrary: one flattened
batch (B = 1, 8192 tokens from seeded Zipf lengths, the jagged-causal function), Hkv = 4, with the tile skipping on and off.
"TF/s" counts 4 D flops per VISIBLE (query, key) pair per head over the hip time; "sdpa /" is the sdpa time over the hip time
(> 1: hip is faster).  The outputs of the two paths are compared before anything is timed.

    python tools/bench_prefill_attn.py [--windows 3] [--quick]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from prefill_attn import flash_attn_func  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--window-ms", type=float, default=20.0, help="device time one timing window aims at")
ap.add_argument("--quick", action="store_true", help="the smallest dense shape and a 2048-token arbitrary batch only")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_prefill_attn.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")
HQ = 16


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


def make(B, S, Hkv, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(dev).bfloat16()   # noqa: E731
    return r(B, S, HQ, D), r(B, S, Hkv, D), r(B, S, Hkv, D)


def sdpa(q, k, v, **kw):
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                       enable_gqa=k.shape[2] != q.shape[2], **kw)
    return o.transpose(1, 2)


def zipf_lengths(total, seed):
    """sequence lengths ~ (total / 4) / rank^1.1 in a seeded random order, at least 16 tokens each, summing to `total`"""
    g = torch.Generator().manual_seed(seed)
    lens, rank = [], 1
    while sum(lens) < total:
        lens.append(min(max(16, int(total / 4 / rank ** 1.1)), total - sum(lens)))
        rank += 1
    lens = [lens[i] for i in torch.randperm(len(lens), generator=g).tolist()]
    assert sum(lens) == total
    return lens


print(f"Hq {HQ}, bf16, random normal q / k / v; times in us, median of {a.windows} alternating windows (+- = (max - min) / median)")
print("dense causal")
print(f"{'B':>3s} {'S':>5s} {'Hkv':>3s} {'D':>4s} {'blocks':>6s} | {'hip':>9s} {'+-':>4s} {'sdpa':>10s} {'+-':>4s} "
      f"{'sdpa /':>6s} | {'TF/s':>6s}", flush=True)
lost = []
dense = [(8, 512), (8, 2048), (2, 8192)] if not a.quick else [(8, 512)]
for D in (64, 128):
    for Hkv in (16, 4):
        for B, S in dense:
            q, k, v = make(B, S, Hkv, D, B * 3 + S + Hkv * 11 + D)
            hip = lambda: flash_attn_func(q, k, v, causal=True)                    # noqa: E731
            ref = lambda: sdpa(q, k, v, is_causal=True)                            # noqa: E731
            # faster and different is not faster: the paths agree to the rounding of bf16 before anything is timed
            torch.testing.assert_close(hip().float(), ref().float(), rtol=2 ** -6, atol=2 ** -6)
            (h, hs), (t, ts) = alternate([hip, ref], a.windows)
            flops = 4.0 * B * HQ * D * (S * (S + 1) / 2)
            print(f"{B:3d} {S:5d} {Hkv:3d} {D:4d} {B * HQ * -(-S // 128):6d} | {h:9.1f} {hs:4.2f} {t:10.1f} {ts:4.2f} "
                  f"{t / h:6.2f} | {flops / h / 1e6:6.1f}", flush=True)
            if t < h:
                lost.append(f"dense causal B {B} S {S} Hkv {Hkv} D {D}: hip {h:.1f} us, sdpa {t:.1f} us")
            del q, k, v

total = 8192 if not a.quick else 2048
lens = zipf_lengths(total, 5)
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
print(f"{'D':>4s} | {'hip skip':>9s} {'+-':>4s} {'hip all':>9s} {'+-':>4s} {'sdpa mask':>10s} {'+-':>4s} {'sdpa /':>6s} {'all /':>6s} | {'TF/s':>6s}",
      flush=True)
for D in (64, 128):
    q, k, v = make(1, total, 4, D, 77 + D)
    on = lambda: flash_attn_func(q, k, v, arbitrary=True, aux_tensors=[func])                        # noqa: E731
    offf = lambda: flash_attn_func(q, k, v, arbitrary=True, aux_tensors=[func], skip_tiles=False)    # noqa: E731
    ref = lambda: sdpa(q, k, v, attn_mask=mask)                                                      # noqa: E731
    torch.testing.assert_close(on().float(), ref().float(), rtol=2 ** -6, atol=2 ** -6)
    assert torch.equal(on(), offf())
    (h, hs), (n, ns), (t, ts) = alternate([on, offf, ref], a.windows)
    print(f"{D:4d} | {h:9.1f} {hs:4.2f} {n:9.1f} {ns:4.2f} {t:10.1f} {ts:4.2f} {t / h:6.2f} {n / h:6.2f} | "
          f"{4.0 * HQ * D * pairs / h / 1e6:6.1f}", flush=True)
    if t < h:
        lost.append(f"arbitrary D {D}: hip {h:.1f} us, sdpa {t:.1f} us")
    del q, k, v
print(f"shapes where sdpa is faster than hip: {len(lost)}")
for row in lost:
    print("  lost " + row)
