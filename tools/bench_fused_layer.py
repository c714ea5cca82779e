"""The fused HSTU layer (fused_hstu_op) and its two activation kernels (csrc/act_ops.hip), timed in one process with HIP
events: every call has its own event pair, the candidates of a comparison alternate call by call, --reps calls each after a
warm-up, and the MEDIAN is reported (times in us).

  1. silu fwd / silu bwd + dbias beside their floor: torch.clone of one [rows, N] bf16 tensor (one read + one write = 2 passes)
     scaled by the kernel's passes over two (forward 2: z, s; backward 3: g, z, dz).  GB/s = bytes from the shapes over the
     time; "of peak" is against 8 TB/s.
  2. the same two beside the eager pair: F.silu, and aten.silu_backward + sum(0) (4 passes: it reads dz again).
  3. the whole layer, forward and forward + backward, and each stage on its own (the stage rows are separate calls of the same
     pieces on the same data, so they need not add up to the whole: the whole also pays autograd and the allocator).

Shapes: 32 x 512 tokens and 8 x 4096 tokens, H = 4, d = 256, hidden 1024 (uvqk width 4096), bf16, causal, dropout 0.2.

    python tools/bench_fused_layer.py [--reps 50]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fused_hstu_op as L  # noqa: E402
import hstu_addmm as A  # noqa: E402
import hstu_norm as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_fused_layer.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")
HEADS, D, HIDDEN, EPS, P, PEAK = 4, 256, 1024, 1e-5, 0.2, 8e12
SHAPES = (("32 x 512", 32, 512), ("8 x 4096", 8, 4096))


def medians(fns, reps):
    """median time in us of each function; the functions alternate call by call"""
    for _ in range(5):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    pairs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for i, fn in enumerate(fns):
            pairs[i][r][0].record()
            fn()
            pairs[i][r][1].record()
    torch.cuda.synchronize()
    return [statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in p) for p in pairs]


def rate(passes, nbytes, us):
    bps = passes * nbytes / (us * 1e-6)
    return f"{bps / 1e9:7.0f} GB/s {100 * bps / PEAK:5.1f} % of peak"


for name, batch, seqlen in SHAPES:
    T, N = batch * seqlen, 4 * HEADS * D
    z = torch.randn(T, N, device=dev).bfloat16()
    g = torch.randn(T, N, device=dev).bfloat16()
    nbytes = T * N * 2
    print(f"== {name} tokens: rows {T}, N {N}, {nbytes / 1e6:.1f} MB a tensor ==", flush=True)

    def eager_bwd():
        dz = torch.ops.aten.silu_backward(g, z)
        return dz, dz.sum(0)

    dz, db = A.silu_bwd_dbias(g, z)
    edz, edb = eager_bwd()
    assert torch.allclose(dz.float(), edz.float(), rtol=2 ** -6, atol=2 ** -6)
    assert torch.allclose(db.float(), edb.float(), rtol=2 ** -5, atol=2.0)
    t_clone, t_fwd, t_efwd, t_bwd, t_ebwd = medians(
        [lambda: g.clone(), lambda: A.triton_silu_fwd(z), lambda: F.silu(z), lambda: A.silu_bwd_dbias(g, z), eager_bwd], a.reps)
    print(f"clone            {t_clone:8.1f} us  {rate(2, nbytes, t_clone)}")
    for label, t, passes, t_eager, eager_passes in (("silu fwd", t_fwd, 2, t_efwd, 2), ("silu bwd + dbias", t_bwd, 3, t_ebwd, 4)):
        floor = t_clone * passes / 2
        print(f"{label:16s} {t:8.1f} us  {rate(passes, nbytes, t)} | floor {floor:7.1f} us, hip / floor {t / floor:5.2f} | "
              f"eager {t_eager:8.1f} us ({eager_passes} passes), hip / eager {t / t_eager:5.2f}", flush=True)
    del dz, db, edz, edb

    # ---- the layer ----
    x = torch.randn(T, HIDDEN, device=dev).bfloat16().requires_grad_(True)
    w_uvqk = (torch.randn(HIDDEN, N, device=dev) * (2.0 / (HIDDEN + N)) ** 0.5).bfloat16().requires_grad_(True)
    b_uvqk = (0.1 * torch.randn(N, device=dev)).bfloat16().requires_grad_(True)
    w_proj = (torch.randn(HEADS * D, HIDDEN, device=dev) * (1.0 / HIDDEN) ** 0.5).bfloat16().requires_grad_(True)
    norm = [(1 + 0.1 * torch.randn(n, device=dev)).bfloat16().requires_grad_(True) if i % 2 == 0 else
            (0.1 * torch.randn(n, device=dev)).bfloat16().requires_grad_(True) for i, n in enumerate((HIDDEN, HIDDEN, HEADS * D, HEADS * D))]
    offsets = torch.arange(0, T + 1, seqlen, device=dev, dtype=torch.int64)
    dout = torch.randn(T, HIDDEN, device=dev).bfloat16()
    params = (x, w_uvqk, b_uvqk, w_proj, *norm)

    def layer():
        return L.fused_hstu_op(x, offsets, seqlen, seqlen, w_uvqk, b_uvqk, w_proj, HEADS, D, D, EPS, P, True, *norm, seed=7)

    def layer_fwd_only():
        with torch.no_grad():
            return layer()

    def layer_fwd_bwd():
        return torch.autograd.grad(layer(), params, dout)

    t_f, t_fb = medians([layer_fwd_only, layer_fwd_bwd], a.reps)
    print(f"layer fwd        {t_f:8.1f} us\nlayer fwd + bwd  {t_fb:8.1f} us   (bwd by difference {t_fb - t_f:8.1f} us)", flush=True)

    # the stages, each on the data the layer would hand it
    import hstu  # noqa: F401,E402
    from hstu import hstu_attn_interface as AT  # noqa: E402

    with torch.no_grad():
        cu = offsets.to(torch.int32)
        xn, mean, rstd, bd, nw = H.triton_weighted_layer_norm_fwd(x, norm[0], norm[1], EPS)
        zz, act = A.triton_addmm_silu_fwd(xn, w_uvqk, b_uvqk, True)
        u, v, q, k = L._split(act, HEADS, D)
        o = AT.hstu_varlen_fwd(q, k, v, cu, seqlen, seqlen, None, None, 1, True, 1.0).view(T, HEADS * D)
        y, omean, orstd, obd, onw, seed = H.triton_layer_norm_mul_dropout_fwd(o, u, norm[2], norm[3], EPS, P, True, False, 7)
        duvqk = torch.empty_like(zz)
        du, dv, dq, dk = L._split(duvqk, HEADS, D)
        gy = torch.randn(T, HEADS * D, device=dev).bfloat16()
        go = torch.randn(T, HEADS, D, device=dev).bfloat16()
        stages = (
            ("fwd input layer norm", lambda: H.triton_weighted_layer_norm_fwd(x, norm[0], norm[1], EPS)),
            ("fwd uvqk addmm + silu", lambda: A.triton_addmm_silu_fwd(xn, w_uvqk, b_uvqk, True)),
            ("fwd attention", lambda: AT.hstu_varlen_fwd(q, k, v, cu, seqlen, seqlen, None, None, 1, True, 1.0)),
            ("fwd ln-mul-dropout", lambda: H.triton_layer_norm_mul_dropout_fwd(o, u, norm[2], norm[3], EPS, P, True, False, 7)),
            ("fwd proj addmm + residual", lambda: A.triton_addmm_silu_fwd(y, w_proj, x, False)),
            ("bwd proj GEMMs", lambda: A.triton_addmm_silu_bwd(y, w_proj, None, dout, False)),
            ("bwd ln-mul-dropout", lambda: H.triton_layer_norm_mul_dropout_bwd(gy, o, u, norm[2], norm[3], omean, orstd, obd, onw, EPS,
                                                                             True, P, seed, False, False, None, du)),
            ("bwd attention", lambda: AT.hstu_varlen_bwd(go, q, k, v, cu, seqlen, seqlen, None, None, 1, True, 1.0, dq=dq, dk=dk, dv=dv)),
            ("bwd silu + dbias + GEMMs", lambda: A.triton_addmm_silu_bwd(xn, w_uvqk, zz, g, True, True)),
            ("bwd input layer norm", lambda: H.triton_weighted_layer_norm_bwd(dout, x, norm[0], norm[1], mean, rstd, True, EPS, bd, nw, dout)),
        )
        times = medians([fn for _, fn in stages], a.reps)
    for (label, _), t in zip(stages, times):
        print(f"  {label:28s} {t:8.1f} us", flush=True)
    print(f"  {'sum of the fwd stages':28s} {sum(times[:5]):8.1f} us\n  {'sum of the bwd stages':28s} {sum(times[5:]):8.1f} us", flush=True)
    del stages, act, zz, duvqk
