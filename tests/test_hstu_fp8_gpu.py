"""FP8 (e4m3fn) HSTU attention on the MI355X: the quantisers bit for bit against the reference's PyTorch statements
(tests/golden/hstu_fp8_quant_golden.npz), and the forward within a derived bound of an fp64 FP8 emulation.

The emulation dequantises q / k / v (vt in mode 1) with their descales, takes the exact SiLU, and keeps P unquantised.
The kernel's output must meet, elementwise,

    |out - emu| <= (2^-4 |P||V~| + 2^-10 s_max sum|V~|) / scaling + 2^-11 |emu| + 2^-16 |P||V~| / scaling + 1e-6

with |P||V~| the product of the absolute values, sum|V~| over the sequence's keys and s_max = max|P| / 448 over the
(sequence, head) in modes 1-5 (1 in mode 0): e4m3's relative rounding of P, its subnormal step, the fp16 rounding of the
output and the fp32 accumulation.  The bound holds whatever P group the kernel picks (it is at most one wave's rows x one
key tile, so its scale is at most s_max).
"""
import os
import zlib

import numpy as np
import pytest
import torch

from oracle.hstu_oracle import local_mask, valid_mask

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "hstu_fp8_quant_golden.npz")
FP8_MAX = 448.0


# ---------------------------------------------------------------------------------------------------- emulation (fp64)

def dequantize(kw, mode, off, which):
    """float64 [T, H, d] value of the fp8 operand `which` ('q', 'k' or 'v'; 'v' is vt in mode 1) times its descale"""
    x8 = kw["vt"] if (which == "v" and mode == 1) else kw[which]
    x = x8.to(torch.float64)
    T, H, D = x.shape
    if mode == 0:
        return x
    off = [int(o) for o in off]
    B = len(off) - 1
    seq = torch.repeat_interleave(torch.arange(B), torch.tensor([off[b + 1] - off[b] for b in range(B)])).to(x.device)
    pos = torch.arange(T, device=x.device) - torch.tensor(off[:-1], device=x.device)[seq]
    if mode == 1 and which != "v":
        d = kw["descale_" + which].to(torch.float64)[:, :T].t()          # [T, H]
        return x * d[:, :, None]
    if mode == 1:
        cu = kw["cu_seqlens_descale_vt"].long()
        tile = cu[seq] + pos // 128
        return x * kw["descale_vt"].to(torch.float64)[tile]
    if mode == 2:
        bs = 128 if which == "q" else (128 if D in (64, 128) else 64)
        cu = kw["cu_seqlens_block_descale_q" if which == "q" else "cu_seqlens_block_descale_kv"].long()
        d = kw["descale_" + which].to(torch.float64)                      # [H, blocks]
        return x * d[:, cu[seq] + pos // bs].t()[:, :, None]
    d = kw["descale_" + which].to(torch.float64)
    if mode == 3:
        return x * d.view(B, H)[seq][:, :, None]
    if mode == 4:
        return x * d.view(B)[seq][:, None, None]
    return x * d.view(1)[0]


def seq_mask(L, b, num_contexts, num_targets, target_group_size, window, device):
    wl, wr = window
    if num_contexts is None and num_targets is None:
        m = local_mask(L, wl, wr)
    else:
        m = valid_mask(L, True, None if num_targets is None else int(num_targets[b]),
                       None if num_contexts is None else int(num_contexts[b]), target_group_size)
    return torch.from_numpy(m).to(device)


def emulate(kw, mode, off, alpha, scaling, num_contexts=None, num_targets=None, target_group_size=1, window=(-1, 0)):
    """(emu, bound) float64 [T, H, d] of the FP8 forward on the quantised operands kw"""
    q, k, v = (dequantize(kw, mode, off, w) for w in ("q", "k", "v"))
    emu, bound = torch.zeros_like(q), torch.zeros_like(q)
    off = [int(o) for o in off]
    for b in range(len(off) - 1):
        lo, hi = off[b], off[b + 1]
        if hi == lo:
            continue
        m = seq_mask(hi - lo, b, num_contexts, num_targets, target_group_size, window, q.device)
        for h in range(q.shape[1]):
            s = alpha * (q[lo:hi, h] @ k[lo:hi, h].t())
            p = torch.where(m, s * torch.sigmoid(s), torch.zeros_like(s))
            vv = v[lo:hi, h]
            o = p @ vv / scaling
            pv = p.abs() @ vv.abs() / scaling
            s_max = max(float(p.abs().max()), 1e-6) / FP8_MAX if mode else 1.0
            emu[lo:hi, h] = o
            bound[lo:hi, h] = (2.0 ** -4 * pv + 2.0 ** -10 * s_max * vv.abs().sum(0)[None, :] / scaling
                               + 2.0 ** -11 * o.abs() + 2.0 ** -16 * pv + 1e-6)
    return emu, bound


def violations(out, emu, bound):
    return (out.to(torch.float64) - emu).abs() > bound


def assert_within(out, emu, bound, what=""):
    assert torch.isfinite(out).all(), f"{what}: NaN / Inf in the output"
    bad = violations(out, emu, bound)
    if bad.any():
        i = tuple(int(t) for t in torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first {i}: out "
                             f"{float(out[i])} emu {float(emu[i])} bound {float(bound[i])}")


# ------------------------------------------------------------------------------------------------------------ helpers

def _seed(name):
    torch.manual_seed(zlib.crc32(name.encode()) % (2**31))


def _jagged(lengths, H, d, dt=torch.bfloat16, scale=1.0):
    off = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device="cuda")
    T = int(off[-1])
    mk = lambda: (torch.rand(T, H, d, device="cuda") * 2 - 1).mul_(scale).to(dt)
    return mk(), mk(), mk(), off


def _golden_cases():
    if not os.path.exists(GOLDEN):
        return []
    return [str(c) for c in np.load(GOLDEN)["cases"]]


def _from_raw(a, f16):
    return torch.from_numpy(a.view(np.int16).copy()).view(torch.float16 if f16 else torch.bfloat16).cuda()


def _bits(t):
    t = t.detach().cpu()
    return t.view(torch.uint8).numpy() if t.dtype == torch.float8_e4m3fn else t.numpy()


# -------------------------------------------------------------------------------------------------- 1. quantisers

@pytest.mark.gpu
@pytest.mark.parametrize("case", _golden_cases())
def test_quantisers_are_bit_exact_against_the_reference(case):
    import hstu

    z = np.load(GOLDEN)
    p = case + "/"
    f16, T, H, D = (int(v) for v in z[p + "meta"])
    x = _from_raw(z[p + "x"], f16)
    off = torch.from_numpy(z[p + "offsets"]).cuda()

    def same(got, key):
        want = z[p + key]
        g = _bits(got)
        assert g.shape == want.shape, f"{key}: shape {g.shape} != {want.shape}"
        if g.dtype == np.float32:
            g, want = g.view(np.int32), want.view(np.int32)
        assert np.array_equal(g, want), f"{key}: {int((g != want).sum())} of {g.size} differ"

    same(hstu.hstu_fp8.quantize_qkv(x, x, x, off, 0)["q"], "m0_x")
    xq, xd, xt, xtd, cu = hstu.quantize_for_two_directions(x, off)
    for got, key in ((xq, "m1_x"), (xd, "m1_descale"), (xt, "m1_xt"), (xtd, "m1_descale_xt"), (cu, "m1_cu")):
        same(got, key)
    assert xd.is_contiguous() and xtd.is_contiguous() and cu.dtype == torch.int32
    bm, bn = (int(v) for v in z[p + "m2_blocks"])
    assert hstu.get_bm_and_bn_block_size_fwd(None, D) == (bm, bn)
    for bs in (64, 128):
        xq, xd, cu = hstu.quantize_for_block_scale(x, off, block_size=bs)
        assert xd.is_contiguous()
        for got, key in ((xq, "x"), (xd, "descale"), (cu, "cu")):
            same(got, f"m2_{bs}_{key}")
    for m in (3, 4, 5):
        xq, xd = hstu.quantize_for_head_batch_tensor(x, off, quant_mode=m)
        same(xq, f"m{m}_x")
        same(xd, f"m{m}_descale")


# ------------------------------------------------------------------------------------------------------ 2. forward

MASKS = {
    "causal": dict(window=(-1, 0)),
    "full": dict(window=(-1, -1)),
    "window": dict(window=(37, 5)),
    "ctx_tgt_g1": dict(window=(-1, 0), ctx=True, tgt=1),
    "ctx_tgt_g3": dict(window=(-1, 0), ctx=True, tgt=3),
}


def _run_fp8(q, k, v, off, mode, alpha, scaling, nc=None, nt=None, g=1, window=(-1, 0)):
    import hstu

    N = int((off[1:] - off[:-1]).max())
    out = hstu.hstu_attn_varlen_func(q, k, v, off, off, None, None, N, N, scaling, nc, nt, g, window, alpha,
                                     quant_mode=mode)
    kw = hstu.hstu_fp8.quantize_qkv(q, k, v, off, mode)
    return out, kw, N


@pytest.mark.gpu
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("mode", range(6))
def test_forward_within_the_bound(mode, d, mask):
    name = f"fwd_{mode}_{d}_{mask}"
    _seed(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lengths = [int(x) for x in rng.integers(1, 330, size=3)] + [129]
    H = 2
    q, k, v, off = _jagged(lengths, H, d)
    spec = MASKS[mask]
    nc = nt = None
    if spec.get("ctx"):
        nc = torch.tensor([min(5, L) for L in lengths], dtype=torch.int32, device="cuda")
        nt = torch.tensor([min(L - min(5, L), 7) for L in lengths], dtype=torch.int32, device="cuda")
    g = spec.get("tgt", 1)
    alpha = 1.0 / d ** 0.5
    scaling = float(max(lengths))
    out, kw, _ = _run_fp8(q, k, v, off, mode, alpha, scaling, nc, nt, g, spec["window"])
    assert out.dtype == torch.float16 and out.shape == q.shape
    emu, bound = emulate(kw, mode, off.cpu(), alpha, scaling, None if nc is None else nc.cpu(),
                         None if nt is None else nt.cpu(), g, spec["window"])
    assert_within(out, emu, bound, name)


# ------------------------------------------------------------------------------------------- 3. quantisation applied

@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mode5_q_outlier", "mode4_head_outlier"])
def test_quantisation_is_really_applied(case):
    import hstu

    _seed(case)
    lengths, H, d = [200, 77], 2, 128
    q, k, v, off = _jagged(lengths, H, d)
    if case == "mode5_q_outlier":
        mode = 5
        q[3, 0, 5] = float(q[3, 0, 5:6].abs().float().clamp(min=0.5)) * 1e5
    else:
        mode = 4   # head 1 of sequence 0 carries q 1e5 x head 0's; its v is small so that its output stays inside fp16
        q[:200, 1] *= 1e5
        v[:200, 1] *= 1e-4
    alpha, scaling = 1.0 / d ** 0.5, 200.0
    out, kw, N = _run_fp8(q, k, v, off, mode, alpha, scaling)
    emu, bound = emulate(kw, mode, off.cpu(), alpha, scaling)
    assert_within(out, emu, bound, case)
    plain = hstu.hstu_attn_varlen_func(q, k, v, off, off, None, None, N, N, scaling, None, None, 1, (-1, 0), alpha)
    assert violations(plain, emu, bound).any(), "the unquantised result fits the bound: the test has no teeth"


# ---------------------------------------------------------------------------------------------- 4. descale indexing

def _pow2(shape, gen):
    return torch.pow(2.0, torch.randint(-3, 3, shape, generator=gen).float()).cuda()


def _fp8_values(shape, gen, device="cuda"):
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 0.25, -0.75, 3.0])
    idx = torch.randint(0, len(vals), shape, generator=gen)
    return vals[idx].to(torch.float8_e4m3fn).to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("d", [64, 256])
def test_descale_indexing(mode, d):
    import hstu

    gen = torch.Generator().manual_seed(zlib.crc32(f"idx_{mode}_{d}".encode()))
    lengths, H = [300, 130, 77], 2
    off = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device="cuda")
    T, B = int(off[-1]), len(lengths)
    kw = dict(q=_fp8_values((T, H, d), gen), k=_fp8_values((T, H, d), gen), v=_fp8_values((T, H, d), gen))
    cu = lambda bs: torch.tensor([0] + list(np.cumsum([-(-L // bs) for L in lengths])), dtype=torch.int32, device="cuda")
    if mode == 1:
        kw["vt"] = kw["v"]
        kw["descale_q"], kw["descale_k"] = _pow2((H, T + 128), gen), _pow2((H, T + 128), gen)
        kw["cu_seqlens_descale_vt"] = cu(128)
        kw["descale_vt"] = _pow2((int(kw["cu_seqlens_descale_vt"][-1]), H, d), gen)
    elif mode == 2:
        bn = hstu.get_bm_and_bn_block_size_fwd(None, d)[1]
        kw["cu_seqlens_block_descale_q"], kw["cu_seqlens_block_descale_kv"] = cu(128), cu(bn)
        kw["descale_q"] = _pow2((H, int(cu(128)[-1])), gen)
        kw["descale_k"], kw["descale_v"] = _pow2((H, int(cu(bn)[-1])), gen), _pow2((H, int(cu(bn)[-1])), gen)
    else:
        shape = {3: (B, H), 4: (B,), 5: (1,)}[mode]
        kw["descale_q"], kw["descale_k"], kw["descale_v"] = (_pow2(shape, gen) for _ in range(3))
    alpha, scaling, N = 0.125, 300.0, max(lengths)
    out, _ = hstu.varlen_fwd(cu_seqlens_q=off, cu_seqlens_k=off, max_seqlen_q=N, max_seqlen_k=N, scaling_seqlen=scaling,
                             num_contexts=None, num_targets=None, target_group_size=1, window_size_left=-1,
                             window_size_right=0, alpha=alpha, rab=None, func=None, quant_mode=mode, **kw)
    emu, bound = emulate(kw, mode, off.cpu(), alpha, scaling)
    assert_within(out, emu, bound, f"mode {mode} d {d}")


# ------------------------------------------------------------------------------------------------------- 5. autograd

@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(6))
def test_autograd_forward_is_varlen_fwd_and_gradients_are_the_unquantised_ones(mode):
    import hstu

    _seed(f"autograd_{mode}")
    lengths, H, d = [150, 64, 33], 2, 128
    q0, k0, v0, off = _jagged(lengths, H, d)
    N, alpha, scaling = max(lengths), 1.0 / d ** 0.5, 150.0
    dout = ((torch.rand(int(off[-1]), H, d, device="cuda") * 0.75 + 0.25)
            * torch.where(torch.rand(int(off[-1]), H, d, device="cuda") < 0.5, -1.0, 1.0)).bfloat16()

    def run(m):
        q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
        out = hstu.hstu_attn_varlen_func(q, k, v, off, off, None, None, N, N, scaling, None, None, 1, (-1, 0), alpha,
                                         quant_mode=m)
        out.backward(dout.to(out.dtype))
        return out.detach(), q.grad, k.grad, v.grad

    out, dq, dk, dv = run(mode)
    assert out.dtype == torch.float16
    kw = hstu.hstu_fp8.quantize_qkv(q0, k0, v0, off, mode)
    ref, _ = hstu.varlen_fwd(cu_seqlens_q=off, cu_seqlens_k=off, max_seqlen_q=N, max_seqlen_k=N, scaling_seqlen=scaling,
                             num_contexts=None, num_targets=None, target_group_size=1, window_size_left=-1,
                             window_size_right=0, alpha=alpha, rab=None, func=None, quant_mode=mode, **kw)
    assert torch.equal(out, ref)
    _, dq0, dk0, dv0 = run(-1)
    for a, b in ((dq, dq0), (dk, dk0), (dv, dv0)):
        assert a.dtype == torch.bfloat16 and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------- 6. refusals

@pytest.mark.gpu
def test_refusals_name_the_option():
    import hstu

    q, k, v, off = _jagged([40, 20], 2, 64)
    N = 40
    call = lambda **kw: hstu.hstu_attn_varlen_func(q, k, v, off, off, None, None, N, N, None, None, None,
                                                   **{"quant_mode": 1, **kw})
    rab = torch.zeros(2, 2, N, N, dtype=q.dtype, device="cuda")
    with pytest.raises(NotImplementedError, match="rab"):
        call(rab=rab)
    with pytest.raises(NotImplementedError, match="rab"):
        call(rab=rab, has_drab=True)
    func = torch.full((1, 1, int(off[-1])), N, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError, match="func"):
        call(func=func)
    with pytest.raises(NotImplementedError, match="delta-q"):
        hstu.hstu_attn_varlen_func(q[:30], k, v, torch.tensor([0, 20, 30], dtype=torch.int32, device="cuda"), off, None,
                                   None, 20, N, None, None, None, quant_mode=1)
    q32, k32, v32, _ = _jagged([40, 20], 2, 32)
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        hstu.hstu_attn_varlen_func(q32, k32, v32, off, off, None, None, N, N, None, None, None, quant_mode=3)
    with pytest.raises(ValueError, match="quant_mode"):
        call(quant_mode=6)
    q8 = q.to(torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError, match="fp8"):
        torch.ops.fbgemm.hstu_varlen_fwd_90(q8, k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn), off, off, None,
                                            None, N, N, float(N), None, None, 1, -1, 0, 1.0, None, None, -1, 0)


# ------------------------------------------------------------------------------------------------------ 7. full size

@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", [("8x4096_d256", 1), ("8x4096_d256", 5), ("c4", 3)])
def test_full_size_within_the_bound(shape, mode):
    _seed(f"full_{shape}_{mode}")
    if shape == "c4":   # bench.py's C4: 32 sequences, Zipf(1.2) lengths clipped to [32, 4096], H 4, d 256
        lengths, H, d = [int(x) for x in np.clip(np.random.default_rng(1).zipf(1.2, 32) + 31, 32, 4096)], 4, 256
    else:
        lengths, H, d = [4096] * 8, 4, 256
    q, k, v, off = _jagged(lengths, H, d)
    alpha, scaling = 1.0 / d ** 0.5, float(max(lengths))
    out, kw, _ = _run_fp8(q, k, v, off, mode, alpha, scaling)
    emu, bound = emulate(kw, mode, off.cpu(), alpha, scaling)
    assert_within(out, emu, bound, f"{shape} mode {mode}")
