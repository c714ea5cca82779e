"""Softmax prefill attention on the GPU (prefill_attn.py / csrc/prefill_attn.hip) against the float64 twin, element by element
under the twin's derived bound (tests/prefill_attn_twin.py).  The shapes (tests/prefill_attn_cases.py) are the smallest that
cross every edge of the kernel; tests/test_prefill_attn_cpu.py checks on the same shapes that the bound can be met and that it
catches mistakes."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from prefill_attn_cases import CASE_BY_NAME, CASES, golden, make_inputs  # noqa: E402
from prefill_attn_twin import compare, prefill_attn_twin, sequences, visible_mask  # noqa: E402

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(HERE), "recsys-examples_amd")
_TENSORS = ("q", "k", "v", "func", "cu_seqlens_q", "cu_seqlens_k")
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


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


def _twin(inp):
    return prefill_attn_twin(inp["q"], inp["k"], inp["v"], causal=inp["causal"], func=inp["func"],
                             cu_seqlens_q=inp["cu_seqlens_q"], cu_seqlens_k=inp["cu_seqlens_k"])


def _run(g, **kw):
    from prefill_attn import flash_attn_func, flash_attn_varlen_func

    if g["cu_seqlens_q"] is not None:
        return flash_attn_varlen_func(g["q"], g["k"], g["v"], g["cu_seqlens_q"], g["cu_seqlens_k"], g["max_seqlen_q"],
                                      g["max_seqlen_k"], causal=g["causal"], return_lse=True, **kw)
    if g["func"] is not None:
        return flash_attn_func(g["q"], g["k"], g["v"], arbitrary=True, aux_tensors=[g["func"]], return_lse=True, **kw)
    return flash_attn_func(g["q"], g["k"], g["v"], causal=g["causal"], return_lse=True, **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_against_the_twin(case):
    inp = make_inputs(case)
    g = _to_gpu(inp)
    if case.form == "strided":   # still three views of one packed buffer: nothing was copied on the way to the kernel
        assert not g["q"].is_contiguous() and not g["k"].is_contiguous() and not g["v"].is_contiguous()
        assert g["q"]._base is g["k"]._base is g["v"]._base and g["q"]._base is not None
        from mi355_native import rows_aligned as _rows_aligned
        assert all(_rows_aligned(g[n]) is g[n] for n in ("q", "k", "v"))
    out, lse = _run(g)
    Hq = case.Hq
    assert out.shape == inp["q"].shape and out.dtype == inp["q"].dtype and out.is_contiguous()
    want = (Hq, inp["q"].shape[0]) if case.form == "jagged" else (inp["q"].shape[0], Hq, inp["q"].shape[1])
    assert lse.shape == want and lse.dtype == torch.float32
    twin = _twin(inp)
    r_out, r_lse = compare(out, lse, twin)
    print(f"{case.name}: worst |err| / bound out {r_out:.3f} lse {r_lse:.3f}")
    assert r_out <= 1 and r_lse <= 1
    out2, lse2 = _run(g)                                   # bitwise reproducible
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    if case.mask != "none":                                # skipping key tiles changes no bit
        out3, lse3 = _run(g, skip_tiles=False)
        assert torch.equal(out, out3) and torch.equal(lse, lse3)
    empty = torch.isinf(twin[1])
    if case.name in ("causal_97x33", "func_random_D64_bf16_fh1", "jagged_causal_qk_differ"):
        assert int(empty.sum()) > 0                        # rows that see nothing: exact zeros and -inf, no NaN
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()
    assert torch.all(lse.cpu()[empty] == -math.inf)


@pytest.mark.parametrize("name", ["causal_33x97", "causal_97x33", "jagged_causal_qk_differ", "jagged_causal_D64_bf16",
                                  "func_random_D64_bf16_fh1", "func_random_D128_fp16_fh4"])
def test_count_probe(name):
    """q = 0 and V[j, d] = 1 if j % D == d: lse[i] = ln(n_i) pins the visible count of every row exactly (ln(n + 1) - ln(n) >=
    1.9e-3 for n <= 512), and out[i, d] = (visible keys j with j % D == d) / n_i within one rounding of the output type"""
    case = CASE_BY_NAME[name]
    inp = make_inputs(case)
    D, Hq = case.D, case.Hq
    inp["q"] = torch.zeros_like(inp["q"])
    v = torch.zeros_like(inp["v"])
    jagged = case.form == "jagged"
    for b, q0, Lq, k0, Lk in sequences(inp["q"], inp["k"], inp["cu_seqlens_q"], inp["cu_seqlens_k"]):
        j = torch.arange(Lk)
        if jagged:
            v[k0 + j, :, j % D] = 1
        else:
            v[b, j, :, j % D] = 1
    inp["v"] = v
    out, lse = _run(_to_gpu(inp))
    out, lse = out.cpu().double(), lse.cpu().double()
    u = UNIT[inp["q"].dtype]
    for b, q0, Lq, k0, Lk in sequences(inp["q"], inp["k"], inp["cu_seqlens_q"], inp["cu_seqlens_k"]):
        if Lq == 0:
            continue
        onehot = torch.nn.functional.one_hot(torch.arange(Lk) % D, D).double() if Lk else torch.zeros(0, D, dtype=torch.float64)
        for h in range(Hq):
            fr = None if inp["func"] is None else inp["func"][b, h if inp["func"].shape[1] > 1 else 0]
            vis = visible_mask(Lq, Lk, causal=inp["causal"], func_rows=fr).double()
            n = vis.sum(-1)
            got_lse = lse[h, q0:q0 + Lq] if jagged else lse[b, h]
            got_out = out[q0:q0 + Lq, h] if jagged else out[b, :, h]
            has = n > 0
            assert torch.all(got_lse[~has] == -math.inf) and torch.all(got_out[~has] == 0)
            assert float((got_lse[has] - n[has].log()).abs().max() if has.any() else 0.0) <= 1e-5, (name, b, h)
            want = (vis @ onehot) / n.clamp_min(1)[:, None]
            err = (got_out - want).abs()
            assert torch.all(err <= u * want + 1e-7), (name, b, h, float(err.max()))   # one rounding; 1e-7: the fp32 1 / n


def test_jagged_causal_function_equals_the_varlen_call():
    """the same tokens as one flattened batch under build_jagged_causal_arbitrary_func and as a jagged batch under
    flash_attn_varlen_func(causal=True): within the sum of the two bounds (they are the same bound)"""
    from prefill_attn import flash_attn_varlen_func

    case = CASE_BY_NAME["func_jagged_causal_D64_bf16_fh1"]
    inp = make_inputs(case)
    g = _to_gpu(inp)
    out_f, lse_f = _run(g)
    offsets = torch.from_numpy(golden()["offsets"]).to(torch.int32)
    cu = offsets.cuda()
    max_len = int((offsets[1:] - offsets[:-1]).max())
    out_v, lse_v = flash_attn_varlen_func(g["q"][0], g["k"][0], g["v"][0], cu, cu, max_len, max_len, causal=True, return_lse=True)
    _, _, b_out, b_lse = _twin(inp)
    d_out = (out_f[0].cpu().double() - out_v.cpu().double()).abs()
    d_lse = (lse_f[0].cpu().double() - lse_v.cpu().double()).abs()
    print(f"func vs varlen: worst |diff| / (2 bound) out {float((d_out / (2 * b_out[0])).max()):.3f} "
          f"lse {float((d_lse / (2 * b_lse[0])).max()):.3f}")
    assert torch.all(d_out <= 2 * b_out[0]) and torch.all(d_lse <= 2 * b_lse[0])


def test_surface():
    import prefill_attn as P

    inp = make_inputs(CASE_BY_NAME["causal_S129_D64_bf16"])
    g = _to_gpu(inp)
    q, k, v = g["q"], g["k"], g["v"]
    out, lse = P.flash_attn_func(q, k, v, causal=True, return_lse=True)
    assert torch.equal(P.flash_attn_func(q, k, v, causal=True), out)
    before = set(sys.modules)
    path = os.path.join(PKG, "flash_attn_gfx950")
    sys.path.insert(0, path)
    try:
        import flash_attn
        import flash_attn.cute.interface as cute
        import flash_attn.flash_attn_interface as fa2

        assert flash_attn.__file__.startswith(path)
        o1 = flash_attn.flash_attn_func(q, k, v, dropout_p=0.0, softmax_scale=None, causal=True)        # -> out
        assert isinstance(o1, torch.Tensor) and torch.equal(o1, out)
        o2, l2 = cute.flash_attn_func(q, k, v, softmax_scale=1.0 / math.sqrt(q.shape[-1]), causal=True)  # -> (out, lse)
        assert torch.equal(o2, out) and torch.equal(l2, lse)
        B, S, Hq, D = q.shape
        cu = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=q.device)
        o3 = fa2.flash_attn_varlen_func(q.reshape(B * S, Hq, D), k.reshape(B * S, -1, D), v.reshape(B * S, -1, D), cu, cu, S, S,
                                        causal=True)                                                    # -> out
        assert isinstance(o3, torch.Tensor) and torch.equal(o3.reshape(B, S, Hq, D), out)
        ov, lv = P.flash_attn_varlen_func(q.reshape(B * S, Hq, D), k.reshape(B * S, -1, D), v.reshape(B * S, -1, D), cu, cu, S, S,
                                          causal=True, return_lse=True)
        assert torch.equal(ov, o3) and torch.equal(lv.reshape(Hq, B, S).permute(1, 0, 2), lse)
        fi = _to_gpu(make_inputs(CASE_BY_NAME["func_target_aware_D64_fp16_fh4"]))
        of, lf = _run(fi)
        oc, lc = cute.flash_attn_func(fi["q"], fi["k"], fi["v"], causal=False, arbitrary=True, linear_k_block_sparse_tensors=None,
                                      linear_q_block_sparse_tensors=None, aux_tensors=[fi["func"]])
        assert torch.equal(oc, of) and torch.equal(lc, lf)
        with pytest.raises(P.PrefillAttnError):
            flash_attn.flash_attn_func(q, k, v, dropout_p=0.1, causal=True)
    finally:
        sys.path.remove(path)
        for name in set(sys.modules) - before:
            if name == "flash_attn" or name.startswith("flash_attn."):
                del sys.modules[name]
    assert "flash_attn" not in sys.modules or "flash_attn" in before

    class Inputs:   # the shape of sid-gr-inference's PrefillAttentionInputs
        def __init__(self, q, k, v, causal):
            self.q, self.k, self.v, self.causal, self.layer_idx = q, k, v, causal, 0

    hidden = P.MI355PrefillBackend()(Inputs(q, k, v, True))
    assert torch.equal(hidden, out)
    # forward only
    qg = q.clone().requires_grad_(True)
    o6 = P.flash_attn_func(qg, k, v, causal=True)
    with pytest.raises(NotImplementedError, match="forward-only"):
        o6.float().sum().backward()
    # no CPU path
    with pytest.raises(P.PrefillAttnError, match="GPU tensor"):
        P.flash_attn_func(q.cpu(), k.cpu(), v.cpu(), causal=True)


def test_captured_in_a_graph():
    """one launch, no host read, no allocation inside the kernel call: the call replays from a captured graph"""
    inp = make_inputs(CASE_BY_NAME["jagged_causal_D64_bf16"])
    g = _to_gpu(inp)
    out, lse = _run(g)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(g)                                            # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o2, l2 = _run(g)
    o2.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o2, out) and torch.equal(l2, lse)
