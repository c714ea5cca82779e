"""Softmax attention backward on the GPU (softmax_attn.py / csrc/softmax_attn_bwd.hip) against the float64 twin, element by
element under the twin's derived bound (tests/softmax_attn_bwd_twin.py), on the shapes of the forward's test plus the edges of
the key-owning pass; tests/test_softmax_attn_bwd_cpu.py checks on the same shapes that the bound can be met and that it catches
mistakes."""
import functools
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from prefill_attn_cases import golden  # noqa: E402
from prefill_attn_twin import sequences, visible_mask  # noqa: E402
from softmax_attn_bwd_twin import BWD_CASE_BY_NAME, BWD_CASES, compare_grads, make_dout, make_inputs, twin_of  # noqa: E402

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(HERE), "recsys-examples_amd")
_TENSORS = ("q", "k", "v", "func", "cu_seqlens_q", "cu_seqlens_k")


def _to_gpu(inp):
    """the same values on the GPU, strides kept (the unbind(2) views of the packed buffer stay views of ONE buffer)"""
    out = dict(inp)
    bases = {}
    for n in _TENSORS:
        t = inp[n]
        if t is None:
            continue
        if t._base is not None and not t.is_contiguous():
            key = id(t._base)
            if key not in bases:
                bases[key] = t._base.cuda()
            out[n] = bases[key].as_strided(t.shape, t.stride(), t.storage_offset())
        else:
            out[n] = t.cuda()
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs, dO and the twin of a case: computed once, shared by the tests, never modified"""
    case = BWD_CASE_BY_NAME[name]
    inp = make_inputs(case)
    dout = make_dout(case, inp)
    return case, inp, dout, twin_of(case, inp, dout)


def _mask_of(g):
    import softmax_attn as S

    return S.MASK_FUNC if g["func"] is not None else (S.MASK_CAUSAL if g["causal"] else S.MASK_NONE)


def _forward(g, module=None, **kw):
    """(out, lse) through the public functions of softmax_attn (or of `module`)"""
    import softmax_attn as S

    m = module or S
    if g["cu_seqlens_q"] is not None:
        return m.flash_attn_varlen_func(g["q"], g["k"], g["v"], g["cu_seqlens_q"], g["cu_seqlens_k"], g["max_seqlen_q"],
                                        g["max_seqlen_k"], causal=g["causal"], return_lse=True, **kw)
    if g["func"] is not None:
        return m.flash_attn_func(g["q"], g["k"], g["v"], arbitrary=True, aux_tensors=[g["func"]], return_lse=True, **kw)
    return m.flash_attn_func(g["q"], g["k"], g["v"], causal=g["causal"], return_lse=True, **kw)


def _poisoned(g):
    return tuple(torch.full(g[n].shape, math.nan, device="cuda", dtype=g[n].dtype) for n in ("q", "k", "v"))


def _backward(g, out, lse, dout, skip_tiles=True, grads=None):
    import softmax_attn as S

    return S._backward(g["q"], g["k"], g["v"], out, lse, dout, g["cu_seqlens_q"], g["cu_seqlens_k"], g["max_seqlen_q"],
                       g["max_seqlen_k"], _mask_of(g), g["func"], 1.0 / math.sqrt(g["q"].shape[-1]), skip_tiles=skip_tiles,
                       grads=grads)


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c.name)
def test_against_the_twin(case):
    case, inp, dout, twin = _case(case.name)
    g = _to_gpu(inp)
    if case.form == "strided":   # still three views of one packed buffer: nothing was copied on the way to the kernels
        assert not g["q"].is_contiguous() and not g["k"].is_contiguous() and not g["v"].is_contiguous()
        assert g["q"]._base is g["k"]._base is g["v"]._base and g["q"]._base is not None
        from mi355_native import rows_aligned as _rows_aligned
        assert all(_rows_aligned(g[n]) is g[n] for n in ("q", "k", "v"))
    out, lse = _forward(g)
    do = dout.cuda()
    grads = _backward(g, out, lse, do, grads=_poisoned(g))
    for t, n in zip(grads, ("q", "k", "v")):
        assert t.shape == inp[n].shape and t.dtype == inp[n].dtype and t.is_contiguous()
        assert not torch.isnan(t).any(), f"d{n} has NaN (an element the kernels did not write, or a bad row)"
    r = compare_grads(grads, twin)
    print(f"{case.name}: worst |err| / bound dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}")
    assert max(r) <= 1                                     # (a bound of 0 asks for an exact 0: compare_grads)
    again = _backward(g, out, lse, do, grads=_poisoned(g))   # bitwise reproducible
    assert all(torch.equal(a, b) for a, b in zip(grads, again))
    if case.mask != "none":                                # skipping tiles changes no bit
        full = _backward(g, out, lse, do, skip_tiles=False, grads=_poisoned(g))
        assert all(torch.equal(a, b) for a, b in zip(grads, full))
    if case.name in ("causal_97x33", "func_random_D64_bf16_fh1", "jagged_causal_qk_differ", "bwd_jagged_causal_edges"):
        assert int((twin[3] == 0).all(-1).sum()) > 0       # rows that see nothing: dq exactly 0
    if case.name in ("jagged_causal_qk_differ", "bwd_jagged_causal_edges"):
        assert int((twin[4] == 0).all(-1).sum()) > 0       # keys nobody sees: dk = dv exactly 0


@pytest.mark.parametrize("name", ["none_70x130_D64_bf16", "causal_mqa_S129", "func_target_aware_D64_fp16_fh4",
                                  "jagged_causal_qk_differ", "strided_causal_D64_bf16"])
def test_autograd_path(name):
    """out.backward(dO) through the public functions gives the bits of _backward; a packed leaf receives one gradient"""
    case, inp, dout, _ = _case(name)
    g = _to_gpu(inp)
    do = dout.cuda()
    out0, lse0 = _forward(g)
    want = _backward(g, out0, lse0, do)
    if case.form == "strided":
        qkv = g["q"]._base.clone().requires_grad_(True)
        q, k, v = qkv.unbind(2)
        leaves = None
    else:
        q, k, v = (g[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
        leaves = (q, k, v)
    out, lse = _forward(dict(g, q=q, k=k, v=v))
    assert torch.equal(out, out0) and torch.equal(lse, lse0)
    assert out.requires_grad and not lse.requires_grad     # lse carries no grad
    out.backward(do)
    if leaves is None:
        assert qkv.grad is not None and qkv.grad.shape == qkv.shape
        got = qkv.grad.unbind(2)
    else:
        got = tuple(t.grad for t in leaves)
    for a, b, n in zip(got, want, "qkv"):
        assert a is not None and torch.equal(a, b), f"d{n}"


@pytest.mark.parametrize("name", ["causal_33x97", "causal_97x33", "jagged_causal_qk_differ", "func_random_D64_bf16_fh1",
                                  "func_random_D128_fp16_fh4"])
def test_mask_column_probe_for_dv(name):
    """q = 0 and dO[i, i mod D] = 1: P is 1 / n_i on the visible keys, so dV[j, c] = sum over the (head of the group, row i =
    c mod D that sees j) of 1 / n_i: every summand is non-negative, the twin's bound is relative (about 2 u), and one wrong
    (query, key) pair moves an element by a whole summand out of at most G ceil(S / D)"""
    case = BWD_CASE_BY_NAME[name]
    inp = dict(make_inputs(case))
    D, Hq, Hkv = case.D, case.Hq, case.Hkv
    jagged = case.form == "jagged"
    inp["q"] = torch.zeros_like(inp["q"])
    dout = torch.zeros_like(inp["q"])
    want = torch.zeros(inp["v"].shape, dtype=torch.float64)
    for b, q0, Lq, k0, Lk in sequences(inp["q"], inp["k"], inp["cu_seqlens_q"], inp["cu_seqlens_k"]):
        i = torch.arange(Lq)
        if jagged:
            dout[q0 + i, :, i % D] = 1
        else:
            dout[b, i, :, i % D] = 1
        if Lq == 0 or Lk == 0:
            continue
        onehot = torch.nn.functional.one_hot(i % D, D).double()
        for h in range(Hq):
            fr = None if inp["func"] is None else inp["func"][b, h if inp["func"].shape[1] > 1 else 0]
            vis = visible_mask(Lq, Lk, causal=inp["causal"], func_rows=fr).double()
            add = (vis / vis.sum(-1).clamp_min(1)[:, None]).t() @ onehot           # [Lk, D]
            if jagged:
                want[k0:k0 + Lk, h // (Hq // Hkv)] += add
            else:
                want[b, :, h // (Hq // Hkv)] += add
    twin = twin_of(case, inp, dout)
    assert float((twin[2] - want).abs().max()) <= 1e-12    # the twin states what the docstring states
    assert float((twin[5] / want.clamp_min(1e-300)).max()) <= 2.5 * 2.0 ** (-8 if case.dtype == "bf16" else -11)   # relative
    g = _to_gpu(inp)
    out, lse = _forward(g)
    grads = _backward(g, out, lse, dout.cuda(), grads=_poisoned(g))
    r = compare_grads(grads, twin)
    print(f"{name}: probe worst |err| / bound dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}")
    assert max(r) <= 1


def test_jagged_causal_function_equals_the_varlen_call():
    """the same tokens as one flattened batch under build_jagged_causal_arbitrary_func and as a jagged batch under
    flash_attn_varlen_func(causal=True): dq, dk, dv within the sum of the two bounds (they are the same bound)"""
    import softmax_attn as S

    case, inp, dout, twin = _case("func_jagged_causal_D64_bf16_fh1")
    g = _to_gpu(inp)
    do = dout.cuda()
    out_f, lse_f = _forward(g)
    g_f = _backward(g, out_f, lse_f, do)
    offsets = torch.from_numpy(golden()["offsets"]).to(torch.int32)
    cu = offsets.cuda()
    max_len = int((offsets[1:] - offsets[:-1]).max())
    q, k, v = g["q"][0], g["k"][0], g["v"][0]
    out_v, lse_v = S.flash_attn_varlen_func(q, k, v, cu, cu, max_len, max_len, causal=True, return_lse=True)
    g_v = S._backward(q, k, v, out_v, lse_v, do[0], cu, cu, max_len, max_len, S.MASK_CAUSAL, None, 1.0 / math.sqrt(case.D))
    for a, b, bound, n in zip(g_f, g_v, twin[3:], "qkv"):
        d = (a[0].cpu().double() - b.cpu().double()).abs()
        print(f"func vs varlen d{n}: worst |diff| / (2 bound) {float((d / (2 * bound[0]).clamp_min(1e-300)).max()):.3f}")
        assert torch.all(d <= 2 * bound[0]), f"d{n}"


def test_stand_in_trains_through_its_import_names():
    """a JaggedGPTLayer-shaped call through flash_attn.cute.interface: a flattened [1, total, H, D] batch under an
    arbitrary_func, back-propagated; and the flash-attn 2 names"""
    import softmax_attn as S

    case, inp, dout, _ = _case("func_target_aware_D64_fp16_fh4")
    g = _to_gpu(inp)
    do = dout.cuda()
    out0, lse0 = _forward(g)
    want = _backward(g, out0, lse0, do)
    before = set(sys.modules)
    path = os.path.join(PKG, "flash_attn_gfx950")
    sys.path.insert(0, path)
    try:
        import flash_attn
        import flash_attn.cute.interface as cute

        assert flash_attn.__file__.startswith(path) and cute._P is S
        q, k, v = (g[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
        out, lse = cute.flash_attn_func(q, k, v, softmax_scale=1.0 / math.sqrt(case.D), causal=False, arbitrary=True,
                                        linear_k_block_sparse_tensors=None, linear_q_block_sparse_tensors=None,
                                        aux_tensors=[g["func"]])
        assert torch.equal(out, out0) and torch.equal(lse, lse0)
        out.backward(do)
        assert all(torch.equal(t.grad, w) for t, w in zip((q, k, v), want))
        c2, i2, d2, _ = _case("causal_mqa_S129")
        g2 = _to_gpu(i2)
        o2, l2 = _forward(g2)
        w2 = _backward(g2, o2, l2, d2.cuda())
        q, k, v = (g2[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
        flash_attn.flash_attn_func(q, k, v, dropout_p=0.0, causal=True).backward(d2.cuda())
        assert all(torch.equal(t.grad, w) for t, w in zip((q, k, v), w2))
    finally:
        sys.path.remove(path)
        for name in set(sys.modules) - before:
            if name == "flash_attn" or name.startswith("flash_attn."):
                del sys.modules[name]


def test_captured_in_a_graph():
    """two launches, no host read, no allocation inside the native call: the backward replays from a captured graph"""
    case, inp, dout, _ = _case("jagged_causal_D64_bf16")
    g = _to_gpu(inp)
    do = dout.cuda()
    out, lse = _forward(g)
    want = _backward(g, out, lse, do)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _backward(g, out, lse, do)                         # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _backward(g, out, lse, do)
    for t in got:
        t.fill_(math.nan)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
