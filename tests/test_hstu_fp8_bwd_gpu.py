"""FP8 (e4m3fn) HSTU attention backward on the MI355X: `hstu.quantize_for_backward` against the reference's backward
quantisation statements, and `hstu.varlen_bwd` within the derived bound of the fp64 emulation of
tests/test_hstu_fp8_bwd_cpu.py (run on the device), for every mode, head dim and mask; plus outliers that the
straight-through gradients cannot meet, descale indexing, the autograd opt-in, determinism and the refusals."""
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("hstu_fp8_bwd_cpu_suite", os.path.join(HERE, "test_hstu_fp8_bwd_cpu.py"))
E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E)
G = E.G


def _seed(name):
    torch.manual_seed(zlib.crc32(name.encode()) % (2**31))


def _dout(T, H, d, dt=torch.bfloat16):
    return ((torch.rand(T, H, d, device="cuda") * 0.75 + 0.25)
            * torch.where(torch.rand(T, H, d, device="cuda") < 0.5, -1.0, 1.0)).to(dt)


def _bwd(kw, off, N, alpha, scaling, mode, nc=None, nt=None, g=1, window=(-1, 0)):
    import hstu

    return hstu.varlen_bwd(dq=None, dk=None, dv=None, cu_seqlens_q=off, cu_seqlens_k=off, max_seqlen_q=N, max_seqlen_k=N,
                           scaling_seqlen=scaling, num_contexts=nc, num_targets=nt, target_group_size=g,
                           window_size_left=window[0], window_size_right=window[1], alpha=alpha, quant_mode=mode, **kw)[:3]


# -------------------------------------------------------------------------------------------------- 1. quantisers

def _bits(t):
    t = t.detach()
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(6))
def test_quantize_for_backward_is_the_reference_statements(mode):
    import hstu

    _seed(f"qbwd_{mode}")
    lengths, H, d = [200, 77, 129, 5], 2, 128
    q, k, v, off = G._jagged(lengths, H, d)
    dout = _dout(int(off[-1]), H, d)
    kw = hstu.quantize_for_backward(q, k, v, dout, off, mode)
    T = int(off[-1])
    same = lambda a, b: torch.equal(_bits(a), _bits(b))
    if mode == 0:
        assert set(kw) == {"dout", "dout_t", "q", "q_t", "k", "k_t", "v", "descale_q", "descale_k", "descale_v", "descale_do"}
        assert kw["dout_t"] is None and kw["q_t"] is None and kw["k_t"] is None
        assert same(kw["dout"], dout.to(torch.float8_e4m3fn)) and same(kw["q"], q.to(torch.float8_e4m3fn))
        assert all(float(kw[n]) == 1.0 for n in ("descale_q", "descale_k", "descale_v", "descale_do"))
    elif mode == 1:
        for x, a, at in ((q, "q", "q_t"), (k, "k", "k_t"), (dout, "dout", "dout_t")):
            xq, xd, xt, xtd, cu = hstu.quantize_for_two_directions(x, off)
            ds, dts = ("descale_do", "descale_dot") if a == "dout" else ("descale_" + a, "descale_" + a + "t")
            assert same(kw[a], xq) and same(kw[at], xt) and kw[at].shape == (T, H, d)
            assert same(kw[ds][:, :T], xd[:, :T]) and same(kw[dts][:int(cu[-1])], xtd)
        assert same(kw["cu_seqlens_descale_qt"], cu) and same(kw["cu_seqlens_descale_kt"], cu)
        vq, vd, _, _, _ = hstu.quantize_for_two_directions(v, off)
        assert same(kw["v"], vq) and same(kw["descale_v"][:, :T], vd[:, :T])
        assert "vt" not in kw and "descale_vt" not in kw
    elif mode == 2:
        assert hstu.get_bm_and_bn_block_size_bwd() == (64, 128)
        for x, a, ds, bs, cuk in ((q, "q", "descale_q", 64, "cu_seqlens_q_block_descale"),
                                  (dout, "dout", "descale_do", 64, "cu_seqlens_q_block_descale"),
                                  (k, "k", "descale_k", 128, "cu_seqlens_kv_block_descale"),
                                  (v, "v", "descale_v", 128, "cu_seqlens_kv_block_descale")):
            xq, xd, cu = hstu.quantize_for_block_scale(x, off, block_size=bs)
            assert same(kw[a], xq) and same(kw[cuk], cu) and same(kw[ds][:, :xd.shape[1]], xd), a
    else:
        for x, a, ds in ((q, "q", "descale_q"), (k, "k", "descale_k"), (v, "v", "descale_v"), (dout, "dout", "descale_do")):
            xq, xd = hstu.quantize_for_head_batch_tensor(x, off, quant_mode=mode)
            assert same(kw[a], xq) and same(kw[ds], xd), a


# ------------------------------------------------------------------------------------------------------ 2. the bound

def _mask_args(spec, lengths):
    nc = nt = None
    if spec.get("ctx"):
        nc = torch.tensor([min(5, L) for L in lengths], dtype=torch.int32, device="cuda")
        nt = torch.tensor([min(L - min(5, L), 7) for L in lengths], dtype=torch.int32, device="cuda")
    return nc, nt, spec.get("tgt", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("mask", list(G.MASKS))
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("mode", range(6))
def test_backward_within_the_bound(mode, d, mask):
    import hstu

    name = f"bwd_{mode}_{d}_{mask}"
    _seed(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lengths = [int(x) for x in rng.integers(1, 330, size=3)] + [129, 17]
    H = 2
    q, k, v, off = G._jagged(lengths, H, d)
    dout = _dout(int(off[-1]), H, d)
    spec = G.MASKS[mask]
    nc, nt, g = _mask_args(spec, lengths)
    alpha, scaling, N = 1.0 / d ** 0.5, float(max(lengths)), max(lengths)
    kw = hstu.quantize_for_backward(q, k, v, dout, off, mode)
    grads = _bwd(kw, off, N, alpha, scaling, mode, nc, nt, g, spec["window"])
    res = E.emulate_bwd(kw, mode, off.cpu(), alpha, scaling, nc, nt, g, spec["window"])
    E.assert_within(grads, res, name)


# ------------------------------------------------------------------------------------------- 3. quantisation applied

@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mode5_q_dout_outlier", "mode4_head_outlier"])
def test_fp8_backward_is_really_quantised(case):
    import hstu

    _seed(case)
    lengths, H, d = [200, 77], 2, 128
    q, k, v, off = G._jagged(lengths, H, d)
    dout = _dout(int(off[-1]), H, d)
    if case == "mode5_q_dout_outlier":
        mode = 5
        q[3, 0, 5] = float(q[3, 0, 5:6].abs().float().clamp(min=0.5)) * 1e5
        dout[11, 1, 7] = 3e3
    else:
        mode = 4   # head 1 of sequence 0 carries q 1e5 x head 0's, and a small v to keep the gradients inside fp16; the dout
        q[:200, 1] *= 1e5   # outlier goes to head 0 (times head 1's P it would overflow dv's fp16)
        v[:200, 1] *= 1e-4
        dout[11, 0, 7] = 3e3
    alpha, scaling, N = 1.0 / d ** 0.5, 200.0, 200
    kw = hstu.quantize_for_backward(q, k, v, dout, off, mode)
    res = E.emulate_bwd(kw, mode, off.cpu(), alpha, scaling)
    E.assert_within(_bwd(kw, off, N, alpha, scaling, mode), res, case)
    qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = hstu.hstu_attn_varlen_func(qs, ks, vs, off, off, None, None, N, N, scaling, None, None, 1, (-1, 0), alpha,
                                     quant_mode=mode)
    out.backward(dout.to(out.dtype))
    assert any(E.violations(t.grad, *res[n]).any() for n, t in zip(E.GRADS, (qs, ks, vs))), \
        "the straight-through gradients fit the bound: the test has no teeth"


# ---------------------------------------------------------------------------------------------- 4. descale indexing

@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("d", [64, 256])
def test_descale_indexing(mode, d):
    gen = torch.Generator().manual_seed(zlib.crc32(f"bidx_{mode}_{d}".encode()))
    lengths, H = [300, 130, 77], 2
    kw, off = E.exact_kw(mode, lengths, H, d, gen, "cuda")
    alpha, scaling, N = 0.125, 300.0, max(lengths)
    grads = _bwd(kw, off, N, alpha, scaling, mode)
    E.assert_within(grads, E.emulate_bwd(kw, mode, off.cpu(), alpha, scaling), f"mode {mode} d {d}")


# ------------------------------------------------------------------------------------------------------- 5. autograd

@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(6))
def test_autograd_fp8_backward_is_varlen_bwd(mode):
    import hstu

    _seed(f"bwd_autograd_{mode}")
    lengths, H, d = [150, 64, 33], 2, 128
    q0, k0, v0, off = G._jagged(lengths, H, d)
    N, alpha, scaling = max(lengths), 1.0 / d ** 0.5, 150.0
    dout = _dout(int(off[-1]), H, d)

    def run(m, fp8_backward):
        q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
        out = hstu.hstu_attn_varlen_func(q, k, v, off, off, None, None, N, N, scaling, None, None, 1, (-1, 0), alpha,
                                         quant_mode=m, fp8_backward=fp8_backward)
        out.backward(dout.to(out.dtype))
        return q.grad, k.grad, v.grad

    got = run(mode, True)
    kw = hstu.quantize_for_backward(q0, k0, v0, dout.to(torch.float16).to(q0.dtype), off, mode)
    ref = _bwd(kw, off, N, alpha, scaling, mode)
    for a, b in zip(got, ref):
        assert a.dtype == torch.bfloat16 and torch.equal(a, b.to(torch.bfloat16))
    for a, b in zip(run(mode, False), run(-1, False)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- 6. determinism

@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 3])
def test_two_calls_are_bit_identical(mode):
    import hstu

    _seed(f"det_{mode}")
    lengths, H, d = [1000, 333, 129], 4, 256
    q, k, v, off = G._jagged(lengths, H, d)
    kw = hstu.quantize_for_backward(q, k, v, _dout(int(off[-1]), H, d), off, mode)
    a = _bwd(kw, off, 1000, 1.0 / 16, 1000.0, mode)
    b = _bwd(kw, off, 1000, 1.0 / 16, 1000.0, mode)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------- 7. refusals

@pytest.mark.gpu
def test_refusals_name_the_option():
    import hstu

    q, k, v, off = G._jagged([40, 20], 2, 64)
    kw = hstu.quantize_for_backward(q, k, v, _dout(60, 2, 64), off, 3)
    call = lambda **over: hstu.varlen_bwd(**{**dict(dq=None, dk=None, dv=None, cu_seqlens_q=off, cu_seqlens_k=off,
                                                      max_seqlen_q=40, max_seqlen_k=40, scaling_seqlen=40.0,
                                                      num_contexts=None, num_targets=None, target_group_size=1,
                                                      window_size_left=-1, window_size_right=0, alpha=1.0, quant_mode=3),
                                             **kw, **over})
    with pytest.raises(NotImplementedError, match="rab"):
        call(rab=torch.zeros(2, 2, 40, 40, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(NotImplementedError, match="has_drab"):
        call(has_drab=True)
    with pytest.raises(NotImplementedError, match="func"):
        call(func=torch.full((1, 1, 60), 40, dtype=torch.int32, device="cuda"))
    with pytest.raises(NotImplementedError, match="delta-q"):
        call(cu_seqlens_q=torch.tensor([0, 20, 30], dtype=torch.int32, device="cuda"), max_seqlen_q=20)
    with pytest.raises(NotImplementedError, match="e5m2"):
        call(v=kw["v"].float().to(torch.float8_e5m2))
    q32, k32, v32, _ = G._jagged([40, 20], 2, 32)
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        hstu.quantize_for_backward(q32, k32, v32, q32, off, 3)
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        call(**{n: kw[n][..., :32].contiguous() for n in ("dout", "q", "k", "v")})
    with pytest.raises(ValueError, match="fp8_backward"):
        hstu.hstu_attn_varlen_func(q, k, v, off, off, None, None, 40, 40, None, None, None, quant_mode=-1,
                                   fp8_backward=True)


# ------------------------------------------------------------------------------------------------------ 8. full size

@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 5])
def test_full_size_within_the_bound(mode):
    import hstu

    _seed(f"bwd_full_{mode}")
    lengths, H, d = [4096] * 8, 4, 256
    q, k, v, off = G._jagged(lengths, H, d)
    dout = _dout(int(off[-1]), H, d)
    alpha, scaling = 1.0 / d ** 0.5, 4096.0
    kw = hstu.quantize_for_backward(q, k, v, dout, off, mode)
    grads = _bwd(kw, off, 4096, alpha, scaling, mode)
    E.assert_within(grads, E.emulate_bwd(kw, mode, off.cpu(), alpha, scaling), f"8x4096 mode {mode}")
