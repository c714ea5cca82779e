"""Mask functions beside a relative bias: the in-kernel path (mi355_hstu_attn_{fwd_kv,bwd}_rab_func) against the dense statement it
replaces (the functions as a 0 / -1e9 bias added to rab in torch, through the rab kernels), both through hstu_attn_varlen_func in one
process, switched by hstu.hstu_attn_interface._FUNC_DENSE (what MI355_HSTU_FUNC_DENSE=1 sets).  Causal mask, per-head rab, has_drab,
bf16; forward and backward timed apart with HIP events, median of --reps after --warmup; the torch time of building the dense bias
(func_mask_bias + add + clamp, part of the dense path's forward) once more on its own; peak memory above the inputs per path.
    python tools/bench_hstu_func_rab.py [--heads 4] [--reps 10] > profiles/hstu_func_rab.txt"""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd")); sys.path.insert(0, ROOT)
import torch
import hstu.hstu_attn_interface as hi
from hstu import hstu_attn_varlen_func

ap = argparse.ArgumentParser()
ap.add_argument("--heads", type=int, default=4); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", default="8x4096,32x512"); ap.add_argument("--dims", default="256,128")
a = ap.parse_args()
dev = torch.device("cuda")
H = a.heads
GiB = float(1 << 30)


def functions(kind, B, L):
    """int32 [1, n_func, B L]: `sink_window` = the first 64 keys and a causal window of L / 4 keys; `two_bands` = a band of 128 keys
    half a sequence back and a causal window of L / 8 keys"""
    pos = torch.arange(B * L, device=dev) % L
    z = torch.zeros_like(pos)
    if kind == "sink_window":
        f = [torch.minimum(pos + 1, torch.full_like(pos, 64)), (pos - L // 4).clamp(min=0), pos + 1]
    else:
        f = [z, (pos - L // 2 - 64).clamp(min=0), (pos - L // 2 + 64).clamp(min=0), (pos - L // 8).clamp(min=0), pos + 1]
    return torch.stack(f).view(1, len(f), B * L).to(torch.int32).contiguous()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def med(ts):
    return f"{statistics.median(ts):8.3f} ({min(ts):.3f} .. {max(ts):.3f})"


print(f"func beside rab, in-kernel vs dense statement: H {H}, causal, per-head rab, has_drab, bf16; ms = median (min .. max) of {a.reps}; "
      "memory = peak above the inputs (q, k, v, dout, rab, func)")
for shape in a.shapes.split(","):
    B, L = (int(x) for x in shape.split("x"))
    for d in (int(x) for x in a.dims.split(",")):
        g = torch.Generator(device=dev); g.manual_seed(d + L)
        mk = lambda *s: torch.randn(*s, device=dev, generator=g).mul_(0.5).to(torch.bfloat16)
        q, k, v, dout = mk(B * L, H, d), mk(B * L, H, d), mk(B * L, H, d), mk(B * L, H, d)
        rab = mk(B, H, L, L)
        cu = torch.arange(0, B * L + 1, L, dtype=torch.int32, device=dev)
        alpha = 1.0 / d ** 0.5
        for kind in ("sink_window", "two_bands"):
            func = functions(kind, B, L)
            res, line = {}, {}
            for path in ("kernel", "dense"):
                hi._FUNC_DENSE = path == "dense"
                tf, tb, peak = [], [], 0
                for it in range(a.warmup + a.reps):
                    qq, kk, vv, rr = (t.detach().requires_grad_(True) for t in (q, k, v, rab))
                    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
                    t_f, out = events(lambda: hstu_attn_varlen_func(qq, kk, vv, cu, cu, None, None, L, L, L, None, None, window_size=(-1, 0),
                                                                    alpha=alpha, rab=rr, has_drab=True, func=func))
                    t_b, _ = events(lambda: out.backward(dout))
                    peak = max(peak, torch.cuda.max_memory_allocated() - base)
                    if it >= a.warmup:
                        tf.append(t_f); tb.append(t_b)
                    res[path] = (out.detach(), qq.grad, kk.grad, vv.grad, rr.grad)
                    del out, qq, kk, vv, rr
                line[path] = (tf, tb, peak)
            hi._FUNC_DENSE = False
            same = all(torch.equal(x, y) for x, y in zip(res["kernel"], res["dense"]))
            del res
            tbias = [events(lambda: (rab + hi.func_mask_bias(func, cu, cu, L, torch.bfloat16)).clamp_(min=torch.finfo(torch.bfloat16).min))[0]
                     for _ in range(a.warmup + a.reps)][a.warmup:]
            print(f"{B} x {L}  d {d:3d}  {kind}")
            for path in ("kernel", "dense"):
                tf, tb, peak = line[path]
                print(f"    {path:6s}  fwd {med(tf)}   bwd {med(tb)}   peak {peak / GiB:6.3f} GiB")
            print(f"    dense bias built in torch (inside the dense fwd): {med(tbias)}   fwd + bwd dense / kernel "
                  f"{(statistics.median(line['dense'][0]) + statistics.median(line['dense'][1])) / (statistics.median(line['kernel'][0]) + statistics.median(line['kernel'][1])):5.2f} x"
                  f"   results bit-equal: {same}")
            torch.cuda.empty_cache()
