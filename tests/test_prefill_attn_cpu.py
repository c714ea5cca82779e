"""CPU checks of softmax prefill attention: the float64 twin against results recorded from torch's SDPA under the masks the
reference's own arbitrary_func encoders describe, the twin's bound against an emulation of the kernel's arithmetic (it can be
met, and it catches mistakes), the argument validation of the Python surface, and the refusals of the C ABI."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from prefill_attn_cases import CASES, MISTAKES, PAD_VALUE, case_func, emulate, golden, golden_mask, make_inputs  # noqa: E402
from prefill_attn_twin import compare, prefill_attn_twin, visible_mask  # noqa: E402

ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "recsys-examples_amd")


def _twin(inp, **kw):
    return prefill_attn_twin(inp["q"], inp["k"], inp["v"], causal=inp["causal"], func=inp["func"],
                             cu_seqlens_q=inp["cu_seqlens_q"], cu_seqlens_k=inp["cu_seqlens_k"], **kw)


@pytest.mark.parametrize("kind", ["jagged_causal", "target_aware", "random"])
def test_twin_matches_the_recorded_reference(kind):
    g = golden()
    S = int(g["offsets"][-1])
    func = torch.from_numpy(g[f"{kind}_func"])
    n_func = {"jagged_causal": 3, "target_aware": 5}.get(kind)
    assert func.shape[2] % 2 == 1 and func.shape[3] == S + 256 and (n_func is None or func.shape[2] == n_func)
    if kind == "random":
        assert func.shape[2] >= 7
    # the interval decoding gives the dense mask the encoder was given / describes
    mask = golden_mask(kind)
    assert torch.equal(visible_mask(S, S, func_rows=func[0, 0]), mask)
    if kind == "random":
        assert int((~mask.any(-1)).sum()) > 0                                    # rows that see nothing
        assert any(bool(mask[i].any()) and int(mask[i].nonzero()[0]) >= 64 for i in range(S))   # first key past tile 0
    func = func.clone()
    func[..., S:] = PAD_VALUE                                                     # the padding columns have no effect
    q, k, v = (torch.from_numpy(g[n]).view(torch.bfloat16) for n in ("q", "k", "v"))
    twin = prefill_attn_twin(q, k, v, func=func, unit_roundoff=2.0 ** -24)
    r_out, r_lse = compare(torch.from_numpy(g[f"{kind}_out"]), torch.from_numpy(g[f"{kind}_lse"]), twin)
    print(f"golden {kind}: worst |err| / bound out {r_out:.3f} lse {r_lse:.3f}")
    assert r_out <= 1 and r_lse <= 1


def test_twin_causal_alignment_and_empty_rows():
    """the statement itself on a case small enough to read: Lq = 3, Lk = 5 sees keys 0..2 / 0..3 / 0..4; Lq = 5, Lk = 3 leaves
    the first two rows without keys"""
    assert visible_mask(3, 5, causal=True).sum(-1).tolist() == [3, 4, 5]
    assert visible_mask(5, 3, causal=True).sum(-1).tolist() == [0, 0, 1, 2, 3]
    q, k = torch.zeros(1, 5, 1, 64, dtype=torch.bfloat16), torch.zeros(1, 3, 1, 64, dtype=torch.bfloat16)
    out, lse, b_out, _ = prefill_attn_twin(q, k, k + 1, causal=True)
    assert torch.all(out[0, :2] == 0) and torch.all(lse[0, 0, :2] == -float("inf")) and torch.all(b_out[0, :2] == 0)
    assert torch.allclose(lse[0, 0, 2:], torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64).log())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_bound_can_be_met(case):
    inp = make_inputs(case)
    out, lse = emulate(inp)
    r_out, r_lse = compare(out, lse, _twin(inp))
    print(f"{case.name}: worst |err| / bound out {r_out:.3f} lse {r_lse:.3f}")
    assert r_out <= 1 and r_lse <= 1


def _applies(case, mistake):
    if mistake in ("causal_off_by_one", "top_left"):
        if case.mask != "causal":
            return False
        if mistake == "causal_off_by_one":
            return True
        if case.form == "jagged":                    # top-left differs from bottom-right only where Lq != Lk
            return any(a != b and a > 0 and b > 0 for a, b in zip(case.lens_q, case.klens))
        return case.sk != case.Sq
    if mistake in ("inclusive_end", "pad_column"):
        return case.mask == "func"
    if mistake == "wrong_head":                      # h % Hkv differs from h // G for some head
        return case.Hkv > 1 and case.Hq > case.Hkv
    raise AssertionError(mistake)


@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_bound_catches_mistakes(mistake):
    checked = 0
    for case in CASES:
        if not _applies(case, mistake):
            continue
        inp = make_inputs(case)
        out, lse = emulate(inp, mistake=mistake)
        r_out, r_lse = compare(out, lse, _twin(inp))
        assert max(r_out, r_lse) > 1, f"{mistake} passes the bound on {case.name}: out {r_out:.3f} lse {r_lse:.3f}"
        checked += 1
    assert checked >= 3


def test_every_kind_appears_with_every_head_dim_and_dtype():
    seen = {(c.mask, c.D) for c in CASES} | {(c.mask, c.dtype) for c in CASES}
    for mask in ("none", "causal", "func"):
        for x in (64, 128, "bf16", "fp16"):
            assert (mask, x) in seen, (mask, x)
    assert {(c.Hq, c.Hkv) for c in CASES} >= {(4, 2), (4, 1), (2, 2)}
    f = case_func([c for c in CASES if c.func_heads > 1][0])
    assert f.shape[1] == 4 and torch.all(f[..., 300:] == PAD_VALUE) and not torch.equal(f[:, 0], f[:, 3])


# ---- the Python surface: everything below raises before a GPU is needed
BF = torch.bfloat16


def _dense(**over):
    a = dict(q=torch.zeros(2, 5, 4, 64, dtype=BF), k=torch.zeros(2, 7, 2, 64, dtype=BF), v=torch.zeros(2, 7, 2, 64, dtype=BF))
    a.update(over)
    return a


_F = torch.zeros(2, 1, 3, 5 + 256, dtype=torch.int32)
BAD_DENSE = {
    "q_3d": dict(q=torch.zeros(5, 4, 64, dtype=BF)),
    "k_batch": dict(k=torch.zeros(3, 7, 2, 64, dtype=BF), v=torch.zeros(3, 7, 2, 64, dtype=BF)),
    "v_shape": dict(v=torch.zeros(2, 8, 2, 64, dtype=BF)),
    "k_dim": dict(k=torch.zeros(2, 7, 2, 32, dtype=BF), v=torch.zeros(2, 7, 2, 32, dtype=BF)),
    "heads_not_divisible": dict(q=torch.zeros(2, 5, 3, 64, dtype=BF)),
    "q_fp32": dict(q=torch.zeros(2, 5, 4, 64)),
    "mixed_dtypes": dict(v=torch.zeros(2, 7, 2, 64, dtype=torch.float16)),
    "head_dim_32": dict(q=torch.zeros(2, 5, 4, 32, dtype=BF), k=torch.zeros(2, 7, 2, 32, dtype=BF), v=torch.zeros(2, 7, 2, 32, dtype=BF)),
    "q_inner_stride": dict(q=torch.zeros(2, 5, 4, 128, dtype=BF)[..., ::2]),
    "arbitrary_and_causal": dict(arbitrary=True, causal=True, aux_tensors=[_F]),
    "arbitrary_no_aux": dict(arbitrary=True),
    "arbitrary_two_aux": dict(arbitrary=True, aux_tensors=[_F, _F]),
    "aux_without_arbitrary": dict(aux_tensors=[_F]),
    "func_int64": dict(arbitrary=True, aux_tensors=[_F.long()]),
    "func_even": dict(arbitrary=True, aux_tensors=[torch.zeros(2, 1, 4, 261, dtype=torch.int32)]),
    "func_heads": dict(arbitrary=True, aux_tensors=[torch.zeros(2, 2, 3, 261, dtype=torch.int32)]),
    "func_short": dict(arbitrary=True, aux_tensors=[torch.zeros(2, 1, 3, 4, dtype=torch.int32)]),
    "func_batch": dict(arbitrary=True, aux_tensors=[torch.zeros(1, 1, 3, 261, dtype=torch.int32)]),
    "dropout": dict(dropout_p=0.1),
    "window": dict(window_size=(16, 0)),
    "softcap": dict(softcap=30.0),
    "alibi": dict(alibi_slopes=torch.zeros(4)),
    "attn_probs": dict(return_attn_probs=True),
    "cpu_tensors": dict(),
    "cpu_tensors_arbitrary": dict(arbitrary=True, aux_tensors=[_F]),
}


@pytest.mark.parametrize("name", sorted(BAD_DENSE))
def test_validation_dense(name):
    import mi355_native as N
    from prefill_attn import PrefillAttnError, flash_attn_func

    with pytest.raises(N.NativeError) as e:
        flash_attn_func(**_dense(**BAD_DENSE[name]))
    assert str(e.value) and isinstance(e.value, PrefillAttnError) and isinstance(e.value, ValueError)
    if name == "v_shape":
        assert "(2, 8, 2, 64)" in str(e.value)      # the offending shape is in the message


def _jagged(**over):
    a = dict(q=torch.zeros(9, 4, 64, dtype=BF), k=torch.zeros(11, 2, 64, dtype=BF), v=torch.zeros(11, 2, 64, dtype=BF),
             cu_seqlens_q=torch.tensor([0, 4, 9], dtype=torch.int32), cu_seqlens_k=torch.tensor([0, 5, 11], dtype=torch.int32),
             max_seqlen_q=5, max_seqlen_k=6, causal=True)
    a.update(over)
    return a


BAD_JAGGED = {
    "q_4d": dict(q=torch.zeros(1, 9, 4, 64, dtype=BF)),
    "cu_int64": dict(cu_seqlens_q=torch.tensor([0, 4, 9])),
    "cu_lengths_differ": dict(cu_seqlens_k=torch.tensor([0, 5, 8, 11], dtype=torch.int32)),
    "cu_2d": dict(cu_seqlens_q=torch.zeros(1, 3, dtype=torch.int32)),
    "max_seqlen_negative": dict(max_seqlen_q=-1),
    "max_seqlen_tensor": dict(max_seqlen_q=torch.tensor(5)),
    "dropout": dict(dropout_p=0.5),
    "block_table": dict(block_table=torch.zeros(2, 2, dtype=torch.int32)),
    "cpu_tensors": dict(),
}


@pytest.mark.parametrize("name", sorted(BAD_JAGGED))
def test_validation_varlen(name):
    from prefill_attn import PrefillAttnError, flash_attn_varlen_func

    with pytest.raises(PrefillAttnError) as e:
        flash_attn_varlen_func(**_jagged(**BAD_JAGGED[name]))
    assert str(e.value)


def test_unknown_keyword_is_a_type_error_and_defaults_pass_validation():
    from prefill_attn import PrefillAttnError, flash_attn_func

    with pytest.raises(TypeError):
        flash_attn_func(**_dense(no_such_argument=1))
    # what the reference's backend passes (dropout_p=0.0) gets as far as the device check
    with pytest.raises(PrefillAttnError, match="GPU tensor"):
        flash_attn_func(**_dense(dropout_p=0.0, window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False))


def test_backward_is_refused_and_signatures_match():
    import inspect

    from prefill_attn import MI355PrefillBackend, PrefillAttn, flash_attn_func, flash_attn_varlen_func

    with pytest.raises(NotImplementedError, match="forward-only"):
        PrefillAttn.backward(None, None, None)
    names = list(inspect.signature(flash_attn_func).parameters)
    assert names[:9] == ["q", "k", "v", "softmax_scale", "causal", "arbitrary", "linear_k_block_sparse_tensors",
                         "linear_q_block_sparse_tensors", "aux_tensors"]
    names = list(inspect.signature(flash_attn_varlen_func).parameters)
    assert names[:9] == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "softmax_scale", "causal"]
    d = {k: v.default for k, v in inspect.signature(flash_attn_func).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d["softmax_scale"] is None and d["causal"] is False and d["arbitrary"] is False and d["skip_tiles"] is True
    assert callable(MI355PrefillBackend())


def test_import_names_resolve_from_their_directory_alone():
    """what the reference does: `from flash_attn import flash_attn_func`, `from flash_attn.flash_attn_interface import
    flash_attn_varlen_func`, `from flash_attn.cute.interface import flash_attn_func`, in a fresh interpreter that has only
    flash_attn_gfx950/ on its path; flash_attn.cute.block_sparsity is absent on purpose"""
    code = (
        "import sys, importlib\n"
        f"sys.path.insert(0, {os.path.join(PKG, 'flash_attn_gfx950')!r})\n"
        "from flash_attn import flash_attn_func as f2\n"
        "from flash_attn.flash_attn_interface import flash_attn_varlen_func as fv\n"
        "from flash_attn.cute.interface import flash_attn_func as fc\n"
        "assert callable(f2) and callable(fv) and callable(fc) and f2 is not fc\n"
        "try:\n"
        "    importlib.import_module('flash_attn.cute.block_sparsity')\n"
        "    raise SystemExit('block_sparsity must be absent')\n"
        "except ImportError:\n"
        "    pass\n"
        "print('ok')\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd="/")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr
    assert not os.path.exists(os.path.join(PKG, "flash_attn"))       # never first on the path of this package's users


# ---- the C ABI: bad arguments are error codes with a message, not crashes (no GPU is touched: the checks come first)
_ABI_BUF = []   # (a host buffer whose address stands in for every pointer: none of these calls gets as far as a launch)


def _abi(**over):
    import ctypes

    if not _ABI_BUF:
        _ABI_BUF.append((ctypes.c_uint8 * 64)())
    base = (ctypes.addressof(_ABI_BUF[0]) + 15) // 16 * 16
    a = dict(q=base, qs=(640, 256, 64), k=base, ks=(896, 128, 64), v=base, vs=(896, 128, 64), cu_q=None, cu_k=None,
             B=2, Sq=5, Sk=7, total_q=0, total_k=0, Hq=4, Hkv=2, D=64, mask=1, func=None, n_func=0, func_heads=0,
             fs=(0, 0, 0, 0), scale=0.125, skip=1, out=base, lse=base, dtype=1)
    a.update(over)
    return (a["q"], *a["qs"], a["k"], *a["ks"], a["v"], *a["vs"], a["cu_q"], a["cu_k"], a["B"], a["Sq"], a["Sk"],
            a["total_q"], a["total_k"], a["Hq"], a["Hkv"], a["D"], a["mask"], a["func"], a["n_func"], a["func_heads"],
            *a["fs"], a["scale"], a["skip"], a["out"], a["lse"], a["dtype"], None), base


ABI_BAD = {
    "head_dim_96": (dict(D=96), b"head dim"),
    "heads_not_divisible": (dict(Hq=3), b"multiple of Hkv"),
    "dtype_fp32": (dict(dtype=0), b"dtype"),
    "mask_kind": (dict(mask=3), b"mask"),
    "n_func_even": (dict(mask=2, func="base", n_func=4, func_heads=1), b"odd"),
    "func_heads": (dict(mask=2, func="base", n_func=3, func_heads=3), b"heads"),
    "func_with_causal": (dict(mask=1, func="base", n_func=3, func_heads=1), b"func"),
    "func_with_jagged": (dict(mask=2, func="base", n_func=3, func_heads=1, cu_q="base", cu_k="base", total_q=9, total_k=9), b"dense"),
    "one_cu_only": (dict(cu_q="base", total_q=9), b"cu_seqlens"),
    "misaligned_q": (dict(q="base+2"), b"aligned"),
    "misaligned_k_stride": (dict(ks=(896, 130, 64)), b"align"),
    "misaligned_out": (dict(out="base+8"), b"aligned"),
    "null_q": (dict(q=None), b"null"),
    "null_func": (dict(mask=2, func=None, n_func=3, func_heads=1), b"func"),
    "negative_length": (dict(Sk=-1), b"negative"),
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
    rc = lib.mi355_prefill_attn(*args)
    msg = lib.mi355_last_error()
    assert rc == -1 and msg.startswith(b"prefill_attn") and word in msg, (rc, msg)


def test_abi_empty_calls_are_ok_without_a_gpu():
    import mi355_native as N

    lib = N.lib()
    args, _ = _abi(B=0)
    assert lib.mi355_prefill_attn(*args) == 0
    args, _ = _abi(Sq=0)
    assert lib.mi355_prefill_attn(*args) == 0
