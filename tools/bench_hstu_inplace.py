"""What handing the backward its gradient buffers costs or saves: torch.ops.fbgemm.hstu_varlen_bwd_80 with dq / dk / dv given
as views of one duvqk-shaped (T, 4 H d) buffer (the fused layer's call, fused_hstu_op.py:932-1006) and with dq = dk = dv = None,
at C3 (32 x 512) and at 8 x 4096, H = 4, d = 256, causal, bf16.  HIP events around every call, median (min .. max) of --reps
timed calls after --warmup, everything in one process.  Run the SAME script on two commits on one box (up to 8 % lies between
boxes) and repeat each to see the run-to-run spread; --repo points the imports at another checkout, --label names the rows:
    timeout -k 10 300 python tools/bench_hstu_inplace.py --label "this commit <id>" >> profiles/hstu_bwd_inplace.txt"""
import argparse, os, statistics, sys
ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default=""); ap.add_argument("--reps", type=int, default=60); ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--legs", default="views,None,views,None")   # (each leg twice: the spread within a run; one leg alone under rocprofv3 --kernel-trace)
a = ap.parse_args()
sys.path.insert(0, os.path.join(a.repo, "recsys-examples_amd")); sys.path.insert(0, a.repo)
import torch
import hstu  # noqa: F401  (registers torch.ops.fbgemm.hstu_varlen_*)

assert a.reps >= 50, "fewer than 50 timed calls say little"
dev = torch.device("cuda")
H, d = 4, 256


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


print(f"# {a.label}: hstu_varlen_bwd_80, H {H}, d {d}, causal, bf16; us = median (min .. max) of {a.reps} calls after {a.warmup}")
for B, L in ((32, 512), (8, 4096)):
    T = B * L
    g = torch.Generator(device=dev); g.manual_seed(B + L)
    mk = lambda: torch.randn(T, H, d, device=dev, generator=g).mul_(0.5).to(torch.bfloat16)
    q, k, v, dout = mk(), mk(), mk(), mk()
    cu = torch.arange(0, T + 1, L, dtype=torch.int32, device=dev)
    duvqk = torch.empty(T, 4 * H * d, dtype=torch.bfloat16, device=dev)
    _, dv, dq, dk = (t.view(-1, H, d) for t in duvqk.split([H * d] * 4, dim=-1))   # (duvqk.split of the fused layer: u, v, q, k)
    alpha = 1.0 / d ** 0.5
    call = lambda gq, gk, gv: torch.ops.fbgemm.hstu_varlen_bwd_80(dout, q, k, v, cu, cu, None, None, L, L, float(L), gq, gk, gv, None, None,
                                                                  1, -1, 0, alpha, None, False, None, False)
    views, none = (lambda: call(dq, dk, dv)), (lambda: call(None, None, None))
    with torch.no_grad():
        r = none()
        same = all(torch.equal(x, y) for x, y in zip(views()[:3], r[:3]))
        del r
        for leg in a.legs.split(","):
            t = timed({"views": views, "None": none}[leg])
            print(f"{B:3d} x {L:4d}  dq/dk/dv {leg:5s}: {t[0]:9.1f} ({t[1]:.1f} .. {t[2]:.1f}) us   views == None bit for bit: {same}")
