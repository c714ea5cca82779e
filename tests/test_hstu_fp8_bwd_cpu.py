"""FP8 HSTU attention backward, the parts that need no device: an fp64 emulation of `hstu.varlen_bwd` on dequantised
operands, its error bound, and the argument checks that run before any launch.  tests/test_hstu_fp8_bwd_gpu.py uses the
emulation and the bound.

The emulation dequantises each product's operands as the reference's backward reads them (mode 1: q / k / dout per token
for S = alpha Q K^T and dP = dO V^T, dout_t for dV, qt for dK, kt for dQ; mode 2: 64-token q / dout blocks, 128-token k / v
blocks), takes the exact SiLU and SiLU', and keeps P and dS unquantised:

    dV = P^T dO~ / N,   dS = dP SiLU'(S) alpha / N,   dK = dS^T Q~,   dQ = dS K~

The kernel rounds P and dS to e4m3 after dividing them by a group scale s <= s_max = max|X| / 448 over the (sequence, head)
(s = 1 in mode 0).  An e4m3 value is off by at most 2^-4 of itself when normal and half the subnormal step 2^-9, times s,
when not, so each gradient g = sum X Y~ (X = P or dS, Y~ its dequantised partner, /N for dV) meets, elementwise,

    |g - emu| <= 2^-4 sum|X||Y~| + 2^-10 s_max sum|Y~| + 2^-11 |emu| + 2^-16 sum|X||Y~| + 1e-6

(/N on the first, second and fourth terms of dV): e4m3's relative rounding of X, its subnormal step, the fp16 rounding of
the gradient, and the fp32 arithmetic of S, dP, SiLU' and the accumulation.  The bound holds for any group the kernel picks.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("hstu_fp8_gpu_suite", os.path.join(HERE, "test_hstu_fp8_gpu.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

FP8_MAX = 448.0
GRADS = ("dq", "dk", "dv")
_KEY = dict(q="q", k="k", v="v", do="dout", qt="q_t", kt="k_t", dot="dout_t")


# ---------------------------------------------------------------------------------------------------- emulation (fp64)

def _seq_pos(off, T, device):
    off = [int(o) for o in off]
    B = len(off) - 1
    seq = torch.repeat_interleave(torch.arange(B), torch.tensor([off[b + 1] - off[b] for b in range(B)])).to(device)
    pos = torch.arange(T, device=device) - torch.tensor(off[:-1], device=device)[seq]
    return seq, pos, B


def dequantize_bwd(kw, mode, off, which):
    """float64 [T, H, d] value of the operand `which` of varlen_bwd(**kw): 'q', 'k', 'v', 'do' or the transposed
    directions 'qt', 'kt', 'dot' (mode 1 reads q_t / k_t / dout_t for them; the other modes reuse q / k / dout)"""
    if mode != 1 and which in ("qt", "kt", "dot"):
        which = which[:-1]
    x = kw[_KEY[which]].to(torch.float64)
    T, H, D = x.shape
    if mode == 0:
        return x
    seq, pos, B = _seq_pos(off, T, x.device)
    d = kw["descale_" + which].to(device=x.device, dtype=torch.float64)
    if mode == 1 and which in ("qt", "kt", "dot"):
        cu = kw["cu_seqlens_descale_kt" if which == "kt" else "cu_seqlens_descale_qt"].to(x.device).long()
        return x * d[cu[seq] + pos // 128]
    if mode == 1:
        return x * d[:, :T].t()[:, :, None]
    if mode == 2:
        bs = 64 if which in ("q", "do") else 128
        cu = kw["cu_seqlens_q_block_descale" if which in ("q", "do") else "cu_seqlens_kv_block_descale"].to(x.device).long()
        return x * d[:, cu[seq] + pos // bs].t()[:, :, None]
    if mode == 3:
        return x * d.view(B, H)[seq][:, :, None]
    if mode == 4:
        return x * d.view(B)[seq][:, None, None]
    return x * d.view(1)[0]


def _dequantize_all(kw, mode, off):
    return {w: dequantize_bwd(kw, mode, off, w) for w in ("q", "k", "v", "do", "qt", "kt", "dot")}


def _fields(deq, lo, hi, h, alpha, scaling, m):
    """P, dS and the partners of one (sequence, head), fp64"""
    op = {w: x[lo:hi, h] for w, x in deq.items()}
    s = alpha * (op["q"] @ op["k"].t())
    sg = torch.sigmoid(s)
    zero = torch.zeros_like(s)
    p = torch.where(m, s * sg, zero)
    ds = torch.where(m, (op["do"] @ op["v"].t()) * sg * (1 + s * (1 - sg)) * alpha / scaling, zero)
    return p, ds, op


def _bound(x, y, emu, mode, div=1.0):
    xy = x.abs() @ y.abs() / div
    s_max = max(float(x.abs().max()), 1e-6) / FP8_MAX if mode else 1.0
    return 2.0 ** -4 * xy + 2.0 ** -10 * s_max * y.abs().sum(0)[None, :] / div + 2.0 ** -11 * emu.abs() + 2.0 ** -16 * xy + 1e-6


def _masks(off, nc, nt, g, window, device):
    off = [int(o) for o in off]
    for b in range(len(off) - 1):
        lo, hi = off[b], off[b + 1]
        if hi > lo:
            yield b, lo, hi, G.seq_mask(hi - lo, b, nc, nt, g, window, device)


def emulate_bwd(kw, mode, off, alpha, scaling, num_contexts=None, num_targets=None, target_group_size=1,
                window=(-1, 0)):
    """{'dq' | 'dk' | 'dv': (emu, bound)} float64 [T, H, d] of varlen_bwd(**kw) (on kw's device)"""
    x = kw["q"]
    T, H, D = x.shape
    res = {n: (torch.zeros(T, H, D, dtype=torch.float64, device=x.device),
               torch.zeros(T, H, D, dtype=torch.float64, device=x.device)) for n in GRADS}
    deq = _dequantize_all(kw, mode, off)
    for b, lo, hi, m in _masks(off, num_contexts, num_targets, target_group_size, window, x.device):
        for h in range(H):
            p, ds, op = _fields(deq, lo, hi, h, alpha, scaling, m)
            for n, xx, y, div in (("dv", p.t(), op["dot"], scaling), ("dk", ds.t(), op["qt"], 1.0), ("dq", ds, op["kt"], 1.0)):
                g = xx @ y / div
                res[n][0][lo:hi, h] = g
                res[n][1][lo:hi, h] = _bound(xx, y, g, mode, div)
    return res


def violations(got, emu, bound):
    return (got.to(torch.float64) - emu).abs() > bound


def assert_within(grads, res, what=""):
    for n, g in zip(GRADS, grads):
        emu, bound = res[n]
        assert g.dtype == torch.float16 and g.shape == emu.shape, f"{what} {n}: {g.dtype} {tuple(g.shape)}"
        assert torch.isfinite(g).all(), f"{what} {n}: NaN / Inf"
        bad = violations(g, emu, bound)
        if bad.any():
            i = tuple(int(t) for t in torch.nonzero(bad)[0])
            raise AssertionError(f"{what} {n}: {int(bad.sum())} of {bad.numel()} outside the bound; first {i}: got "
                                 f"{float(g[i])} emu {float(emu[i])} bound {float(bound[i])}")


# ------------------------------------------------------------------------------------------ operands with exact values

def _pow2(shape, gen, device, lo=-3, hi=3):
    return torch.pow(2.0, torch.randint(lo, hi, shape, generator=gen).double()).float().to(device)


def exact_kw(mode, lengths, H, d, gen, device="cpu"):
    """varlen_bwd keyword arguments of exact e4m3 values and power-of-two descales in every layout of `mode`.  Mode 1's
    transposed directions carry the same bytes as q / k / dout but descales of their own, so that a product that reads the
    wrong direction is off by powers of two."""
    off = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32)
    T, B = int(off[-1]), len(lengths)
    kw = {_KEY[w]: G._fp8_values((T, H, d), gen, device) for w in ("q", "k", "v", "do")}
    kw.update(q_t=None, k_t=None, dout_t=None)
    cu = lambda bs: torch.tensor([0] + list(np.cumsum([-(-L // bs) for L in lengths])), dtype=torch.int32, device=device)
    if mode == 1:
        for w in ("q", "k", "v", "do"):
            kw["descale_" + w] = _pow2((H, T + 128), gen, device)
        kw["q_t"], kw["k_t"], kw["dout_t"] = kw["q"], kw["k"], kw["dout"]
        kw["cu_seqlens_descale_qt"], kw["cu_seqlens_descale_kt"] = cu(128), cu(128)
        for w in ("qt", "kt", "dot"):
            kw["descale_" + w] = _pow2((int(cu(128)[-1]), H, d), gen, device, 2, 5)
    elif mode == 2:
        kw["cu_seqlens_q_block_descale"], kw["cu_seqlens_kv_block_descale"] = cu(64), cu(128)
        for w in ("q", "do"):
            kw["descale_" + w] = _pow2((H, int(cu(64)[-1])), gen, device)
        for w in ("k", "v"):
            kw["descale_" + w] = _pow2((H, int(cu(128)[-1])), gen, device)
    elif mode >= 3:
        shape = {3: (B, H), 4: (B,), 5: (1,)}[mode]
        for w in ("q", "k", "v", "do"):
            kw["descale_" + w] = _pow2(shape, gen, device)
    return kw, off.to(device)


# --------------------------------------------------------------------------------------- a simulated fp8 backward

def _e4m3_groups(x, rows, cols, scaled):
    """x rounded to e4m3 per rows x cols group (divided by max(1e-6, max|x|) / 448 first when scaled)"""
    y = torch.empty_like(x)
    for i in range(0, x.shape[0], rows):
        for j in range(0, x.shape[1], cols):
            blk = x[i:i + rows, j:j + cols]
            s = max(float(blk.abs().max()), 1e-6) / FP8_MAX if scaled else 1.0
            y[i:i + rows, j:j + cols] = (blk / s).clamp(-FP8_MAX, FP8_MAX).float().to(torch.float8_e4m3fn).double() * s
    return y


def simulate(kw, mode, off, alpha, scaling, plant=None, window=(-1, 0)):
    """dq, dk, dv (fp16) of a backward that rounds P and dS to e4m3 per 32-query x 64-key group, or one with a planted
    error: 'dk_from_q' (mode 1's dK from q instead of qt), 'no_1_over_n', 'unscaled_ds', 'dv_from_v'"""
    x = kw["q"]
    T, H, D = x.shape
    out = [torch.zeros(T, H, D, dtype=torch.float64) for _ in GRADS]
    deq = _dequantize_all(kw, mode, off)
    for b, lo, hi, m in _masks(off, None, None, 1, window, "cpu"):
        for h in range(H):
            p, ds, op = _fields(deq, lo, hi, h, alpha, scaling, m)
            if plant == "no_1_over_n":
                ds = ds * scaling
            pq = _e4m3_groups(p, 32, 64, mode != 0)
            dsq = _e4m3_groups(ds, 32, 64, mode != 0 and plant != "unscaled_ds")
            qt = op["q"] if plant == "dk_from_q" else op["qt"]
            do = op["v"] if plant == "dv_from_v" else op["dot"]
            out[0][lo:hi, h] = dsq @ op["kt"]
            out[1][lo:hi, h] = dsq.t() @ qt
            out[2][lo:hi, h] = pq.t() @ do / (1.0 if plant == "no_1_over_n" else scaling)
    return [o.to(torch.float16) for o in out]


# ------------------------------------------------------------------------------------------------------------- tests

def _mode5_kw(lengths, H, d, seed):
    """mode 5 quantisation of random inputs on the CPU (the reference's per-tensor statement)"""
    gen = torch.Generator().manual_seed(seed)
    off = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32)
    T = int(off[-1])
    kw = {}
    for w in ("q", "k", "v", "do"):
        x = (torch.rand(T, H, d, generator=gen) * 2 - 1)
        ds = torch.clamp(x.abs().max() / FP8_MAX, min=1e-6)
        kw[_KEY[w]], kw["descale_" + w] = (x / ds).to(torch.float8_e4m3fn), ds.view(1)
    return kw, off


@pytest.mark.parametrize("window", [(-1, 0), (-1, -1), (9, 3)])
def test_emulation_is_the_autograd_of_the_fp64_attention(window):
    """mode 5 (one descale set for every product): the emulated gradients are torch.autograd's of the fp64 attention on
    the dequantised operands"""
    lengths, H, d, alpha = [37, 70, 5], 2, 64, 0.3
    kw, off = _mode5_kw(lengths, H, d, 3)
    scaling = 70.0
    res = emulate_bwd(kw, 5, off, alpha, scaling, window=window)
    q, k, v = (G.dequantize(dict(kw, vt=kw["v"]), 5, off, w).requires_grad_(True) for w in ("q", "k", "v"))
    do = dequantize_bwd(kw, 5, off, "do")
    outs = []
    for b, lo, hi, m in _masks(off, None, None, 1, window, "cpu"):
        s = alpha * torch.einsum("ihd,jhd->hij", q[lo:hi], k[lo:hi])
        p = torch.where(m[None], torch.nn.functional.silu(s), torch.zeros_like(s))
        outs.append(torch.einsum("hij,jhd->ihd", p, v[lo:hi]) / scaling)
    torch.cat(outs).backward(do)
    for n, t in zip(GRADS, (q, k, v)):
        emu = res[n][0]
        assert float((emu - t.grad).abs().max()) <= 1e-12 * float(t.grad.abs().max()), n


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 5])
def test_bound_accepts_a_simulated_fp8_backward(mode):
    gen = torch.Generator().manual_seed(100 + mode)
    kw, off = exact_kw(mode, [70, 200, 3], 2, 64, gen)
    alpha, scaling = 0.125, 200.0
    res = emulate_bwd(kw, mode, off, alpha, scaling)
    got = simulate(kw, mode, off, alpha, scaling)
    assert_within(got, res, f"mode {mode}")
    assert all(float(g.abs().max()) > 0 for g in got)


@pytest.mark.parametrize("plant,mode,grad", [("dk_from_q", 1, "dk"), ("no_1_over_n", 3, "dv"), ("no_1_over_n", 3, "dk"),
                                             ("unscaled_ds", 3, "dk"), ("unscaled_ds", 3, "dq"), ("dv_from_v", 2, "dv")])
def test_bound_rejects_planted_errors(plant, mode, grad):
    gen = torch.Generator().manual_seed(200 + mode)
    kw, off = exact_kw(mode, [70, 200, 3], 2, 64, gen)
    alpha, scaling = 0.125, 200.0
    res = emulate_bwd(kw, mode, off, alpha, scaling)
    got = dict(zip(GRADS, simulate(kw, mode, off, alpha, scaling, plant)))
    assert violations(got[grad], *res[grad]).any(), f"{plant}: the bound accepts it"


def _cpu_fp8(T=40, H=2, d=64, dtype=torch.float8_e4m3fn):
    return torch.zeros(T, H, d).to(dtype)


def _bwd_kw(**over):
    t = _cpu_fp8()
    off = torch.tensor([0, 25, 40], dtype=torch.int32)
    kw = dict(dout=t, dout_t=None, q=t, q_t=None, k=t, k_t=None, v=t, dq=None, dk=None, dv=None, cu_seqlens_q=off,
              cu_seqlens_k=off, max_seqlen_q=25, max_seqlen_k=25, scaling_seqlen=25, num_contexts=None, num_targets=None,
              target_group_size=1, window_size_left=-1, window_size_right=0, alpha=1.0, quant_mode=0)
    kw.update(over)
    return kw


def test_varlen_bwd_argument_errors_raise_before_any_launch():
    import hstu

    assert hstu.get_bm_and_bn_block_size_bwd() == (64, 128)
    with pytest.raises(ValueError, match="quant_mode"):
        hstu.varlen_bwd(**_bwd_kw(quant_mode=6))
    with pytest.raises(ValueError, match="quant_mode"):
        hstu.varlen_bwd(**_bwd_kw(quant_mode=-1))
    with pytest.raises(NotImplementedError, match="rab"):
        hstu.varlen_bwd(**_bwd_kw(rab=torch.zeros(2, 2, 25, 25)))
    with pytest.raises(NotImplementedError, match="has_drab"):
        hstu.varlen_bwd(**_bwd_kw(has_drab=True))
    with pytest.raises(NotImplementedError, match="func"):
        hstu.varlen_bwd(**_bwd_kw(func=torch.zeros(1, 1, 40, dtype=torch.int32)))
    with pytest.raises(NotImplementedError, match="e5m2"):
        hstu.varlen_bwd(**_bwd_kw(k=_cpu_fp8(dtype=torch.float8_e5m2)))
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        hstu.varlen_bwd(**_bwd_kw(dout=torch.zeros(40, 2, 64, dtype=torch.bfloat16)))
    with pytest.raises(RuntimeError, match="dout_t"):
        hstu.varlen_bwd(**_bwd_kw(quant_mode=1))
    t32 = _cpu_fp8(d=32)
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        hstu.varlen_bwd(**_bwd_kw(dout=t32, q=t32, k=t32, v=t32))
    with pytest.raises(NotImplementedError, match="delta-q"):
        hstu.varlen_bwd(**_bwd_kw(cu_seqlens_q=torch.tensor([0, 10, 20], dtype=torch.int32), q=_cpu_fp8(T=20),
                                  max_seqlen_q=10))
    with pytest.raises(RuntimeError, match="shaped like q"):
        hstu.varlen_bwd(**_bwd_kw(v=_cpu_fp8(T=39)))
    with pytest.raises(RuntimeError, match="device"):
        hstu.varlen_bwd(**_bwd_kw())


def test_quantize_for_backward_and_fp8_backward_argument_errors():
    import hstu

    x = torch.zeros(40, 2, 64, dtype=torch.bfloat16)
    off = torch.tensor([0, 25, 40], dtype=torch.int32)
    with pytest.raises(ValueError, match="quant_mode"):
        hstu.quantize_for_backward(x, x, x, x, off, 6)
    with pytest.raises(RuntimeError, match="dout"):
        hstu.quantize_for_backward(x, x, x, x[:39], off, 1)
    with pytest.raises(RuntimeError, match="dtype"):
        hstu.quantize_for_backward(x, x, x, x.half(), off, 1)
    x32 = torch.zeros(40, 2, 32, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        hstu.quantize_for_backward(x32, x32, x32, x32, off, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        hstu.quantize_for_backward(x, x, x, x, off, 3)
    with pytest.raises(ValueError, match="fp8_backward"):
        hstu.hstu_attn_varlen_func(x, x, x, off, off, None, None, 25, 25, None, None, None, quant_mode=-1,
                                   fp8_backward=True)
