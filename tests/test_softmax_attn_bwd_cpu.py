"""CPU checks of the softmax attention backward: the float64 twin against torch.autograd, the twin's bound against an emulation
of the kernels' arithmetic (it can be met, and it catches mistakes), the C ABI's refusals, and the Python surface."""
import inspect
import math
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from prefill_attn_cases import _emu_mask, emulate  # noqa: E402
from prefill_attn_twin import sequences, visible_mask  # noqa: E402
from softmax_attn_bwd_twin import (BWD_CASE_BY_NAME, BWD_CASES, EXTRA_CASES, compare_grads, make_dout, make_inputs,  # noqa: E402
                                   softmax_attn_bwd_twin, twin_of)

ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "recsys-examples_amd")

MISTAKES = ("no_delta", "delta_other_head", "lse_log2", "no_scale", "group_first_head", "mask_off_by_one", "inclusive_end")


def emulate_bwd(inp, dout, mistake=None):
    """The kernels' arithmetic in torch on the CPU: out / lse from the forward emulation; fp32 scores, P = exp(s - lse) from the
    stored lse, delta = dO . out in fp32 from the stored out, dS = P (dP - delta), P and dS rounded once to the operand type,
    fp32 sums, the scale on the fp32 sums of dq / dk, one output rounding.  -> dq, dk, dv in the operand dtype"""
    assert mistake is None or mistake in MISTAKES
    out, lse = emulate(inp)
    q, k, v, func = inp["q"], inp["k"], inp["v"], inp["func"]
    jagged = inp["cu_seqlens_q"] is not None
    dt = q.dtype
    Hq, D, Hkv = q.shape[-2], q.shape[-1], k.shape[-2]
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    hk_of = torch.arange(Hq) // G
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    zero = torch.zeros(())
    mask_mistake = {"mask_off_by_one": "causal_off_by_one", "inclusive_end": "inclusive_end"}.get(mistake)
    for b, q0, Lq, k0, Lk in sequences(q, k, inp["cu_seqlens_q"], inp["cu_seqlens_k"]):
        if Lq == 0 or Lk == 0:
            continue
        qs, ks = (slice(q0, q0 + Lq), slice(k0, k0 + Lk)) if jagged else (b, b)
        qb, dob, ob = q[qs].float(), dout[qs].float(), out[qs].float()               # [Lq, Hq, D]
        kb, vb = k[ks].float()[:, hk_of], v[ks].float()[:, hk_of]
        ls = lse[:, q0:q0 + Lq] if jagged else lse[b]                                # [Hq, Lq] fp32
        if func is not None:
            fh = func.shape[1]
            vis = torch.stack([_emu_mask(Lq, Lk, False, func[b, h if fh > 1 else 0], mask_mistake) for h in range(Hq)])
        else:
            vis = _emu_mask(Lq, Lk, inp["causal"], None, mask_mistake)[None].expand(Hq, Lq, Lk)
        has = torch.isfinite(ls)
        off = torch.where(has, ls, zero)
        if mistake == "lse_log2":            # the natural-log lse subtracted from the log2-scaled score
            off = off * math.log(2.0)
        s = torch.einsum("ihd,jhd->hij", qb, kb) * scale
        p = torch.where(vis & has[..., None], torch.exp(s - off[..., None]), zero)
        dP = torch.einsum("ihd,jhd->hij", dob, vb)
        delta = (dob * ob).sum(-1).t()                                               # [Hq, Lq]
        if mistake == "no_delta":
            delta = torch.zeros_like(delta)
        if mistake == "delta_other_head":
            delta = delta.roll(1, 0)
        dS = (p * (dP - delta[..., None])).to(dt).float()
        p16 = p.to(dt).float()
        sc = 1.0 if mistake == "no_scale" else scale
        dq_b = torch.einsum("hij,jhd->ihd", dS, kb) * sc
        dk_h = torch.einsum("hij,ihd->jhd", dS, qb).reshape(Lk, Hkv, G, D)
        dv_h = torch.einsum("hij,ihd->jhd", p16, dob).reshape(Lk, Hkv, G, D)
        if mistake == "group_first_head":
            dk_h, dv_h = dk_h[:, :, :1], dv_h[:, :, :1]
        dq[qs], dk[ks], dv[ks] = dq_b.to(dt), (dk_h.sum(2) * sc).to(dt), dv_h.sum(2).to(dt)
    return dq, dk, dv


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c.name)
def test_the_bound_can_be_met(case):
    inp = make_inputs(case)
    dout = make_dout(case, inp)
    r = compare_grads(emulate_bwd(inp, dout), twin_of(case, inp, dout))
    print(f"{case.name}: worst |err| / bound dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}")
    assert max(r) <= 1


def _applies(case, mistake):
    if mistake in ("no_delta", "lse_log2"):
        return True
    if mistake == "no_scale":                        # a row with a single key has dS = 0: dq and dk are 0 under any scale
        return case.form != "dense" or case.sk > 1
    if mistake == "delta_other_head":
        return case.Hq > 1
    if mistake == "group_first_head":
        return case.Hq > case.Hkv
    if mistake == "mask_off_by_one":
        return case.mask == "causal"
    if mistake == "inclusive_end":
        return case.mask == "func"
    raise AssertionError(mistake)


@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_bound_catches_mistakes(mistake):
    checked = 0
    for case in BWD_CASES:
        if not _applies(case, mistake):
            continue
        inp = make_inputs(case)
        dout = make_dout(case, inp)
        r = compare_grads(emulate_bwd(inp, dout, mistake=mistake), twin_of(case, inp, dout))
        assert max(r) > 1, f"{mistake} passes the bound on {case.name}: dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}"
        checked += 1
    assert checked >= 3


@pytest.mark.parametrize("name", ["causal_S129_D64_bf16", "causal_mqa_S129", "causal_97x33", "none_70x130_D128_fp16",
                                  "jagged_causal_qk_differ", "func_random_D128_fp16_fh4", "func_batch2_mqa",
                                  "bwd_causal_130x259_mqa", "bwd_jagged_causal_edges"])
def test_twin_matches_autograd(name):
    """dq / dk / dv of the twin against torch.autograd through a float64 softmax attention under the dense mask"""
    case = BWD_CASE_BY_NAME[name]
    inp = make_inputs(case)
    dout = make_dout(case, inp).double()
    q, k, v = (inp[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    Hq, D, Hkv = q.shape[-2], q.shape[-1], k.shape[-2]
    hk_of = torch.arange(Hq) // (Hq // Hkv)
    jagged = case.form == "jagged"
    loss = 0.0
    for b, q0, Lq, k0, Lk in sequences(q, k, inp["cu_seqlens_q"], inp["cu_seqlens_k"]):
        if Lq == 0 or Lk == 0:
            continue
        qs, ks = (slice(q0, q0 + Lq), slice(k0, k0 + Lk)) if jagged else (b, b)
        if inp["func"] is not None:
            fh = inp["func"].shape[1]
            vis = torch.stack([visible_mask(Lq, Lk, func_rows=inp["func"][b, h if fh > 1 else 0]) for h in range(Hq)])
        else:
            vis = visible_mask(Lq, Lk, causal=inp["causal"])[None].expand(Hq, Lq, Lk)
        s = torch.einsum("ihd,jhd->hij", q[qs], k[ks][:, hk_of]) / math.sqrt(D)
        s = torch.where(vis, s, torch.full_like(s, -1e300))
        p = torch.softmax(s, -1) * vis.any(-1, keepdim=True)                        # a row that sees nothing: out = 0
        loss = loss + (torch.einsum("hij,jhd->ihd", p, v[ks][:, hk_of]) * dout[qs]).sum()
    loss.backward()
    twin = twin_of(case, inp, dout)
    for got, want, n in zip(twin[:3], (q.grad, k.grad, v.grad), ("dq", "dk", "dv")):
        want = torch.zeros_like(got) if want is None else want
        assert float((got - want).abs().max()) <= 1e-10, (name, n)


def test_the_extra_cases_cross_the_edges_of_the_key_pass():
    names = {c.name: c for c in EXTRA_CASES}
    assert names["bwd_none_5x257"].sk == 257 and names["bwd_none_5x257"].Sq == 5
    c = names["bwd_causal_130x259_mqa"]
    assert (c.Sq, c.sk, c.Hq, c.Hkv) == (130, 259, 4, 1)
    c = names["bwd_jagged_causal_edges"]
    assert c.lens_q == (0, 3, 130) and c.lens_k == (70, 129, 1)
    inp = make_inputs(c)
    dout = make_dout(c, inp)
    dq, dk, dv, bq, bk, bv = twin_of(c, inp, dout)
    assert torch.all(dk[:70] == 0) and torch.all(bk[:70] == 0) and torch.all(bv[:70] == 0)   # keys without queries
    assert torch.all(bq[3:3 + 129] == 0)                                                     # 130 rows over 1 key: 129 see nothing


# ---- the C ABI: bad arguments are error codes with a message (no GPU is touched: the checks come first)
_ABI_BUF = []


def _abi(**over):
    import ctypes

    if not _ABI_BUF:
        _ABI_BUF.append((ctypes.c_uint8 * 64)())
    base = (ctypes.addressof(_ABI_BUF[0]) + 15) // 16 * 16
    a = dict(q=base, qs=(640, 256, 64), k=base, ks=(896, 128, 64), v=base, vs=(896, 128, 64), cu_q=None, cu_k=None,
             B=2, Sq=5, Sk=7, total_q=0, total_k=0, Hq=4, Hkv=2, D=64, mask=1, func=None, n_func=0, func_heads=0,
             fs=(0, 0, 0, 0), scale=0.125, skip=1, out=base, dout=base, ds=(1280, 256, 64), lse=base, delta=base,
             dq=base, dk=base, dv=base, dtype=1)
    a.update(over)
    return (a["q"], *a["qs"], a["k"], *a["ks"], a["v"], *a["vs"], a["cu_q"], a["cu_k"], a["B"], a["Sq"], a["Sk"],
            a["total_q"], a["total_k"], a["Hq"], a["Hkv"], a["D"], a["mask"], a["func"], a["n_func"], a["func_heads"],
            *a["fs"], a["scale"], a["skip"], a["out"], a["dout"], *a["ds"], a["lse"], a["delta"], a["dq"], a["dk"], a["dv"],
            a["dtype"], None), base


ABI_BAD = {
    "head_dim_96": (dict(D=96), b"head dim"),
    "heads_not_divisible": (dict(Hq=3), b"multiple of Hkv"),
    "dtype_fp32": (dict(dtype=0), b"dtype"),
    "mask_kind": (dict(mask=3), b"mask"),
    "n_func_even": (dict(mask=2, func="base", n_func=4, func_heads=1), b"odd"),
    "n_func_too_large": (dict(mask=2, func="base", n_func=131, func_heads=1), b"129"),
    "func_heads": (dict(mask=2, func="base", n_func=3, func_heads=3), b"heads"),
    "func_with_causal": (dict(mask=1, func="base", n_func=3, func_heads=1), b"func"),
    "func_with_jagged": (dict(mask=2, func="base", n_func=3, func_heads=1, cu_q="base", cu_k="base", total_q=9, total_k=9), b"dense"),
    "one_cu_only": (dict(cu_q="base", total_q=9), b"cu_seqlens"),
    "misaligned_q": (dict(q="base+2"), b"aligned"),
    "misaligned_k_stride": (dict(ks=(896, 130, 64)), b"align"),
    "misaligned_dout_stride": (dict(ds=(1280, 250, 64)), b"dout"),
    "misaligned_dq": (dict(dq="base+8"), b"aligned"),
    "misaligned_dk": (dict(dk="base+8"), b"align"),
    "null_q": (dict(q=None), b"null"),
    "null_dout": (dict(dout=None), b"null"),
    "null_delta": (dict(delta=None), b"null"),
    "null_dv": (dict(dv=None), b"null"),
    "null_func": (dict(mask=2, func=None, n_func=3, func_heads=1), b"func"),
    "negative_length": (dict(Sk=-1), b"negative"),
    "skip_tiles_2": (dict(skip=2), b"skip_tiles"),
}


@pytest.mark.parametrize("name", sorted(ABI_BAD))
def test_abi_refuses_bad_arguments(name):
    import mi355_native as N

    lib = N.lib()
    over, word = ABI_BAD[name]
    _, base = _abi()
    over = {k: (base if v == "base" else base + int(v[5:]) if isinstance(v, str) and v.startswith("base+") else v)
            for k, v in over.items()}
    args, _ = _abi(**over)
    rc = lib.mi355_softmax_attn_bwd(*args)
    msg = lib.mi355_last_error()
    assert rc == -1 and msg.startswith(b"softmax_attn_bwd") and word in msg, (rc, msg)


def test_abi_is_exported_bound_and_empty_calls_are_ok_without_a_gpu():
    import mi355_native as N

    lib = N.lib()
    assert "mi355_softmax_attn_bwd" in N.exported_symbols() and hasattr(lib, "mi355_softmax_attn_bwd")
    assert "mi355_softmax_attn_bwd" in open(os.path.join(ROOT, "include", "recsys_amd.h")).read()
    args, _ = _abi(B=0)
    assert lib.mi355_softmax_attn_bwd(*args) == 0
    args, _ = _abi(Sq=0, Sk=0)
    assert lib.mi355_softmax_attn_bwd(*args) == 0


# ---- the Python surface
def test_signatures_equal_those_of_prefill_attn():
    import prefill_attn as P
    import softmax_attn as S

    for name in ("flash_attn_func", "flash_attn_varlen_func"):
        assert inspect.signature(getattr(S, name)) == inspect.signature(getattr(P, name)), name
    assert S.PrefillAttnError is P.PrefillAttnError
    assert list(inspect.signature(S._backward).parameters)[-2:] == ["skip_tiles", "grads"]
    assert issubclass(S.SoftmaxAttn, torch.autograd.Function)


def test_validation_and_refusals_are_those_of_prefill_attn():
    import softmax_attn as S

    BF = torch.bfloat16
    q, k = torch.zeros(2, 5, 4, 64, dtype=BF), torch.zeros(2, 7, 2, 64, dtype=BF)
    with pytest.raises(S.PrefillAttnError, match="GPU tensor"):
        S.flash_attn_func(q, k, k, causal=True, dropout_p=0.0)
    with pytest.raises(S.PrefillAttnError, match="dropout_p"):
        S.flash_attn_func(q, k, k, dropout_p=0.1)
    with pytest.raises(S.PrefillAttnError, match=r"\(2, 8, 2, 64\)"):
        S.flash_attn_func(q, k, torch.zeros(2, 8, 2, 64, dtype=BF))
    with pytest.raises(TypeError):
        S.flash_attn_func(q, k, k, no_such_argument=1)
    with pytest.raises(S.PrefillAttnError, match="n_func=131"):
        S.flash_attn_func(q, k, k, arbitrary=True, aux_tensors=[torch.zeros(2, 1, 131, 261, dtype=torch.int32)])
    cu = torch.tensor([0, 4, 9], dtype=torch.int32)
    qj, kj = torch.zeros(9, 4, 64, dtype=BF), torch.zeros(9, 2, 64, dtype=BF)
    with pytest.raises(S.PrefillAttnError, match="max_seqlen"):
        S.flash_attn_varlen_func(qj, kj, kj, cu, cu, 5, -1)
    with pytest.raises(S.PrefillAttnError, match="window_size"):
        S.flash_attn_varlen_func(qj, kj, kj, cu, cu, 5, 5, window_size=(16, 0))
    with pytest.raises(S.PrefillAttnError, match="GPU tensor"):
        S.flash_attn_varlen_func(qj, kj, kj, cu, cu, 5, 5, causal=True)


def _bad_calls():
    """name -> (function name, args, kwargs): calls that both surfaces refuse before any GPU work (all tensors on the CPU)"""
    BF, I32 = torch.bfloat16, torch.int32
    q, k = torch.zeros(2, 5, 4, 64, dtype=BF), torch.zeros(2, 7, 2, 64, dtype=BF)
    fn = lambda *s, dtype=I32: torch.zeros(*s, dtype=dtype)   # noqa: E731
    qj, kj = torch.zeros(9, 4, 64, dtype=BF), torch.zeros(9, 2, 64, dtype=BF)
    cu = torch.tensor([0, 4, 9], dtype=I32)
    D, V = "flash_attn_func", "flash_attn_varlen_func"
    return {
        "non-tensor q": (D, ([[1.0]], k, k), {}),
        "wrong rank": (D, (q[0], k, k), {}),
        "wrong rank, jagged": (V, (q, k, k, cu, cu, 5, 5), {}),
        "v shape differs from k": (D, (q, k, torch.zeros(2, 8, 2, 64, dtype=BF)), {}),
        "Hq no multiple of Hkv": (D, (q, torch.zeros(2, 7, 3, 64, dtype=BF), torch.zeros(2, 7, 3, 64, dtype=BF)), {}),
        "fp32 q": (D, (q.float(), k, k), {}),
        "D = 96": (D, (torch.zeros(2, 5, 4, 96, dtype=BF), torch.zeros(2, 7, 2, 96, dtype=BF), torch.zeros(2, 7, 2, 96, dtype=BF)), {}),
        "stride(-1) != 1": (D, (torch.zeros(2, 5, 4, 128, dtype=BF)[..., ::2], k, k), {}),
        "causal with arbitrary": (D, (q, k, k), dict(causal=True, arbitrary=True, aux_tensors=[fn(2, 1, 3, 5)])),
        "no aux tensor": (D, (q, k, k), dict(arbitrary=True)),
        "zero aux tensors": (D, (q, k, k), dict(arbitrary=True, aux_tensors=[])),
        "two aux tensors": (D, (q, k, k), dict(arbitrary=True, aux_tensors=[fn(2, 1, 3, 5), fn(2, 1, 3, 5)])),
        "func not int32": (D, (q, k, k), dict(arbitrary=True, aux_tensors=[fn(2, 1, 3, 5, dtype=torch.int64)])),
        "func not 4-D": (D, (q, k, k), dict(arbitrary=True, aux_tensors=[fn(2, 3, 5)])),
        "even n_func": (D, (q, k, k), dict(arbitrary=True, aux_tensors=[fn(2, 1, 4, 5)])),
        "func too short for Sq": (D, (q, k, k), dict(arbitrary=True, aux_tensors=[fn(2, 1, 3, 4)])),
        "aux_tensors without arbitrary": (D, (q, k, k), dict(aux_tensors=[fn(2, 1, 3, 5)])),
        "cu_seqlens not int32": (V, (qj, kj, kj, cu.long(), cu, 5, 5), {}),
        "unequal cu lengths": (V, (qj, kj, kj, cu, cu[:2], 5, 5), {}),
        "negative max_seqlen": (V, (qj, kj, kj, cu, cu, 5, -1), {}),
        "unsupported keyword, dense": (D, (q, k, k), dict(dropout_p=0.1)),
        "unsupported keyword, jagged": (V, (qj, kj, kj, cu, cu, 5, 5), dict(window_size=(16, 0))),
        "unknown keyword": (D, (q, k, k), dict(no_such_argument=1)),
        "unknown keyword, jagged": (V, (qj, kj, kj, cu, cu, 5, 5), dict(no_such_argument=1)),
        "CPU tensor": (D, (q, k, k), dict(causal=True)),
        "CPU tensor, func": (D, (q, k, k), dict(arbitrary=True, aux_tensors=[fn(2, 4, 5, 8)])),
        "CPU tensor, jagged": (V, (qj, kj, kj, cu, cu, 5, 5), dict(causal=True)),
    }


def test_both_surfaces_refuse_a_bad_call_with_the_same_exception_and_message():
    """prefill_attn and softmax_attn validate through one function (prefill_attn._validate_dense / _validate_varlen); the
    backward's limit on n_func is the only refusal that softmax_attn adds."""
    import prefill_attn as P
    import softmax_attn as S

    for name, (fname, args, kw) in _bad_calls().items():
        raised = []
        for mod in (P, S):
            with pytest.raises(Exception) as ei:
                getattr(mod, fname)(*args, **kw)
            raised.append(ei.value)
        assert type(raised[0]) is type(raised[1]), name
        assert str(raised[0]) == str(raised[1]) and str(raised[0]), name
        assert isinstance(raised[0], (P.PrefillAttnError, TypeError)), (name, raised[0])
    # n_func = 131: the forward-only surface goes on to ask for GPU tensors, the differentiable one refuses the function
    q, k = torch.zeros(2, 5, 4, 64, dtype=torch.bfloat16), torch.zeros(2, 7, 2, 64, dtype=torch.bfloat16)
    kw = dict(arbitrary=True, aux_tensors=[torch.zeros(2, 1, 131, 5, dtype=torch.int32)])
    with pytest.raises(P.PrefillAttnError, match="GPU tensor"):
        P.flash_attn_func(q, k, k, **kw)
    with pytest.raises(S.PrefillAttnError, match="n_func=131 > 129 is not supported by the backward"):
        S.flash_attn_func(q, k, k, **kw)
    kw = dict(arbitrary=True, aux_tensors=[torch.zeros(2, 1, 129, 5, dtype=torch.int32)])
    with pytest.raises(S.PrefillAttnError, match="GPU tensor"):   # 129 itself is taken
        S.flash_attn_func(q, k, k, **kw)


def test_the_stand_in_import_names_resolve_to_softmax_attn():
    code = (
        "import sys\n"
        f"sys.path.insert(0, {os.path.join(PKG, 'flash_attn_gfx950')!r})\n"
        "import flash_attn, flash_attn.flash_attn_interface as fa2, flash_attn.cute.interface as cute\n"
        "import softmax_attn\n"
        "assert fa2._P is softmax_attn and cute._P is softmax_attn\n"
        "assert flash_attn.flash_attn_func is fa2.flash_attn_func and flash_attn.flash_attn_varlen_func is fa2.flash_attn_varlen_func\n"
        "assert 'forward only' not in flash_attn.__doc__\n"
        "print('ok')\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd="/")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr
