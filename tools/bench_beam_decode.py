"""Beam-search decode attention (beam_decode_attn.beam_decode_attn) over a subset of the reference's benchmark grid, next to a
plain-torch bf16 statement timed in the same process: HIP events, every shape warmed up, --windows windows per path with the
two paths alternating window by window, the median window reported with the spread (max - min) / median.

  torch   scores of the shared context by one batched matmul per kv head (the G heads of a group stacked on the rows, no
          expanded K), the beam keys gathered through the index list and scored, the two score blocks concatenated, one fp32
          softmax, then the context matmul plus the gathered beam values.  It is the only baseline on this hardware.
  hip     the function of this package: two launches (context flash-decoding with `ns` KV splits, beam + merge).

Grid: W in {128, 512, 1024}, ctx in {256, 2048, 4096}, decode_nums in {1, 16}, Hkv in {1, 16} with Hq = 16, D in {64, 128},
bf16, batch --batch.  "torch /" is the torch time over the hip time (> 1: hip is faster).  "roof" is the larger of two floors
over the hip time: 4 B W Hq (Sk + dn) D flops at the sustained bf16 MFMA rate (--mfma-tflops, from tools/ubench_mfma.hip on
256 CUs) and the K / V bytes (context once, beam rows once) at the HBM rate (--hbm-tbs, a measured copy rate); "by" names
the floor that is the larger.  The outputs of the two paths are compared before anything is timed.

--sweep times the hip path for _num_splits in {1, 2, 4, 8, 16, 32} (capped by the key tiles) on every shape whose unsplit
launch has fewer workgroups than CUs: the split rule of beam_decode_attn.num_splits is read off that table.

    python tools/bench_beam_decode.py [--batch 2] [--windows 3] [--sweep] [--only W,ctx,dn,Hkv,D]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import torch  # noqa: E402

from beam_decode_attn import KEY_TILE, ROW_TILE, beam_decode_attn, num_splits  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--window-ms", type=float, default=15.0, help="device time one timing window aims at")
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--only", default="", help="one shape: W,ctx,dn,Hkv,D")
ap.add_argument("--mfma-tflops", type=float, default=1900.0)
ap.add_argument("--hbm-tbs", type=float, default=6.29)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_beam_decode.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")
HQ = 16
if a.only:
    GRID = [tuple(int(v) for v in a.only.split(","))]
else:
    GRID = [(W, ctx, dn, Hkv, D) for D in (64, 128) for Hkv in (1, 16) for W in (128, 512, 1024) for ctx in (256, 2048, 4096)
            for dn in (1, 16)]


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


def make(B, W, ctx, dn, Hkv, D):
    g = torch.Generator(device="cpu").manual_seed(W * 7 + ctx * 3 + dn + Hkv * 11 + D)
    r = lambda *s: torch.randn(*s, generator=g).to(dev).bfloat16()   # noqa: E731
    q, kc, vc = r(B, 1, W, HQ, D), r(B, ctx, Hkv, D), r(B, ctx, Hkv, D)
    kb, vb = r(B, dn * W, Hkv, D), r(B, dn * W, Hkv, D)
    tk = torch.randint(0, dn * W, (B, 1, Hkv, dn, W), generator=g, dtype=torch.int32).repeat_interleave(HQ // Hkv, dim=2).to(dev)
    return q, kc, vc, kb, vb, tk


def torch_statement(q, kc, vc, kb, vb, tk, dn):
    B, _, W, Hq, D = q.shape
    Hkv, Sk, G = kc.shape[2], kc.shape[1], q.shape[3] // kc.shape[2]
    scale = 1.0 / math.sqrt(D)
    qg = q[:, 0].view(B, W, Hkv, G, D).permute(0, 2, 3, 1, 4)                     # [B, Hkv, G, W, D]
    s_ctx = torch.matmul(qg.reshape(B, Hkv, G * W, D), kc.permute(0, 2, 3, 1))   # [B, Hkv, G W, Sk]
    idx = tk[:, 0, ::G, :dn].long()                                              # [B, Hkv, dn, W]
    bi = torch.arange(B, device=q.device)[:, None, None, None]
    hi = torch.arange(Hkv, device=q.device)[None, :, None, None]
    kg, vg = kb[bi, idx, hi], vb[bi, idx, hi]                                    # [B, Hkv, dn, W, D]
    s_beam = torch.einsum("bhgwd,bhnwd->bhgwn", qg, kg).reshape(B, Hkv, G * W, dn)
    p = torch.softmax(torch.cat([s_ctx, s_beam], dim=-1).float() * scale, dim=-1).to(q.dtype)
    o = torch.matmul(p[..., :Sk], vc.permute(0, 2, 1, 3))
    o = o.view(B, Hkv, G, W, D) + torch.einsum("bhgwn,bhnwd->bhgwd", p[..., Sk:].reshape(B, Hkv, G, W, dn), vg)
    return o.permute(0, 3, 1, 2, 4).reshape(B, 1, W, Hq, D)


B = a.batch
print(f"batch {B}, Hq {HQ}, bf16; MFMA floor at {a.mfma_tflops:.0f} TFLOP/s, HBM floor at {a.hbm_tbs:.2f} TB/s; times in us")
print(f"{'W':>5s} {'ctx':>5s} {'dn':>3s} {'Hkv':>3s} {'D':>4s} {'blocks':>6s} {'ns':>3s} | {'hip':>8s} {'+-':>4s} {'torch':>9s} {'+-':>4s} "
      f"{'torch /':>7s} | {'TF/s':>6s} {'roof':>5s} {'by':>4s}", flush=True)
lost = []
for (W, ctx, dn, Hkv, D) in GRID:
    q, kc, vc, kb, vb, tk = make(B, W, ctx, dn, Hkv, D)
    G = HQ // Hkv
    blocks = B * Hkv * -(-(W * G) // ROW_TILE)
    ns = num_splits(B, W, HQ, Hkv, D, ctx)
    hip = lambda: beam_decode_attn(q, kc, vc, kb, vb, tk, dn)[0]                  # noqa: E731
    ref = lambda: torch_statement(q, kc, vc, kb, vb, tk, dn)                      # noqa: E731
    # faster and different is not faster: the two paths agree to the rounding of bf16 before anything is timed
    torch.testing.assert_close(hip().float(), ref().float(), rtol=2 ** -6, atol=2 ** -6)
    (h, hs), (t, ts) = alternate([hip, ref], a.windows)
    flops = 4.0 * B * W * HQ * (ctx + dn) * D
    kv_bytes = 2.0 * 2 * B * Hkv * D * (ctx + dn * W)
    f_mfma, f_hbm = flops / (a.mfma_tflops * 1e6), kv_bytes / (a.hbm_tbs * 1e6)   # us
    floor, by = (f_mfma, "mfma") if f_mfma >= f_hbm else (f_hbm, "hbm")
    print(f"{W:5d} {ctx:5d} {dn:3d} {Hkv:3d} {D:4d} {blocks:6d} {ns:3d} | {h:8.1f} {hs:4.2f} {t:9.1f} {ts:4.2f} {t / h:7.2f} | "
          f"{flops / h / 1e6:6.1f} {floor / h:5.3f} {by:>4s}", flush=True)
    if t < h:
        lost.append((W, ctx, dn, Hkv, D, h, t))
    if a.sweep and blocks < 256:
        tiles = -(-ctx // KEY_TILE)
        cand = [n for n in (1, 2, 4, 8, 16, 32) if n <= tiles]
        fns = [(lambda n=n: beam_decode_attn(q, kc, vc, kb, vb, tk, dn, _num_splits=n)[0]) for n in cand]
        res = alternate(fns, a.windows)
        print("      sweep _num_splits: " + "  ".join(f"{n}: {m:.1f}" for n, (m, _) in zip(cand, res))
              + f"   (best {cand[min(range(len(cand)), key=lambda i: res[i][0])]}, rule {ns})", flush=True)
    del q, kc, vc, kb, vb, tk
print(f"shapes where torch is faster than hip: {len(lost)}")
for row in lost:
    print("  lost W %d ctx %d dn %d Hkv %d D %d: hip %.1f us, torch %.1f us" % row)
