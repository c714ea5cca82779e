"""CPU checks of beam-search decode attention: the float64 twin against arrays recorded from the reference's PyTorch
statement, the twin's bound against an emulation of the kernel's arithmetic (it can be met, and it catches mistakes), the
split rule, and the argument validation of the Python surface."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from beam_decode_cases import CASES, emulate, make_inputs  # noqa: E402
from beam_decode_twin import beam_decode_twin, compare  # noqa: E402

ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "recsys-examples_amd")


def _twin(inp, **kw):
    return beam_decode_twin(inp["q"], inp["k_context"], inp["v_context"], inp["k_beam"], inp["v_beam"],
                            inp["topk_indices"], inp["decode_nums"], seqused_k=inp["seqused_k"],
                            cu_seqlens_k=inp["cu_seqlens_k"], **kw)


def test_twin_matches_the_recorded_reference():
    z = np.load(os.path.join(HERE, "golden", "beam_decode_golden.npz"))
    cases = z["cases"]
    assert len(cases) >= 3
    for i, (B, W, Hq, Hkv, D, ctx, dn, max_dn) in enumerate(cases.tolist()):
        t = {n: torch.from_numpy(z[f"c{i}_{n}"]).view(torch.bfloat16) for n in ("q", "k_context", "v_context", "k_beam", "v_beam")}
        assert t["q"].shape == (B, 1, W, Hq, D) and t["k_context"].shape == (B, ctx, Hkv, D)
        twin = beam_decode_twin(t["q"], t["k_context"], t["v_context"], t["k_beam"], t["v_beam"],
                                torch.from_numpy(z[f"c{i}_topk"]), int(dn), unit_roundoff=2.0 ** -24)
        r_out, r_lse = compare(torch.from_numpy(z[f"c{i}_out"]), torch.from_numpy(z[f"c{i}_lse"]), twin)
        print(f"golden case {i}: worst |err| / bound out {r_out:.3f} lse {r_lse:.3f}")
        assert r_out <= 1 and r_lse <= 1


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_bound_can_be_met(case):
    inp = make_inputs(case)
    for ns in (1, 2, 3):
        out, lse = emulate(inp, num_splits=ns)
        r_out, r_lse = compare(out, lse, _twin(inp, num_splits=ns))
        print(f"{case.name} ns={ns}: worst |err| / bound out {r_out:.3f} lse {r_lse:.3f}")
        assert r_out <= 1 and r_lse <= 1


def _applies(case, inp, mistake):
    lens = case.lens if case.lens else (case.ctx,) * case.batch
    if mistake == "drop_top":        # some row must have two keys or more
        return max(lens) + case.dn >= 2
    if mistake == "shift_idx":
        return case.dn > 0 and case.W * case.dn > 1
    if mistake == "wrong_head":      # h % Hkv differs from h // G for some head
        return case.Hkv > 1 and case.Hq > case.Hkv and max(lens) + case.dn > 0
    if mistake == "max_merge":       # two partials or more: a beam phase beside a context, or two key tiles under two splits
        return (case.dn > 0 and max(lens) > 0) or max(lens) > 64
    raise AssertionError(mistake)


@pytest.mark.parametrize("mistake", ["drop_top", "shift_idx", "wrong_head", "max_merge"])
def test_the_bound_catches_mistakes(mistake):
    checked = 0
    for case in CASES:
        inp = make_inputs(case)
        if not _applies(case, inp, mistake):
            continue
        out, lse = emulate(inp, num_splits=2, mistake=mistake)
        r_out, r_lse = compare(out, lse, _twin(inp, num_splits=2))
        assert max(r_out, r_lse) > 1, f"{mistake} passes the bound on {case.name}: out {r_out:.3f} lse {r_lse:.3f}"
        checked += 1
    assert checked >= 10


def test_num_splits_rule():
    from beam_decode_attn import KEY_TILE, num_splits

    for B in (1, 2, 8, 64):
        for W in (1, 128, 512, 1024):
            for Hkv in (1, 4, 16):
                for Sk in (0, 1, 63, 64, 65, 256, 2048, 4096, 100000):
                    ns = num_splits(B, W, 16, Hkv, 128, Sk)
                    tiles = -(-Sk // KEY_TILE)
                    assert isinstance(ns, int) and ns >= 1
                    assert ns <= max(tiles, 1)
                    blocks = B * Hkv * -(-(W * (16 // Hkv)) // 128)
                    if blocks >= 256:
                        assert ns == 1
    assert num_splits(1, 128, 16, 1, 128, 4096) > 1     # a launch of 16 workgroups is split


def _args(**over):
    B, W, Hq, Hkv, D, ctx, dn = 2, 3, 4, 2, 64, 5, 2
    a = dict(q=torch.zeros(B, 1, W, Hq, D, dtype=torch.bfloat16), k_context=torch.zeros(B, ctx, Hkv, D, dtype=torch.bfloat16),
             v_context=torch.zeros(B, ctx, Hkv, D, dtype=torch.bfloat16), k_beam=torch.zeros(B, dn * W, Hkv, D, dtype=torch.bfloat16),
             v_beam=torch.zeros(B, dn * W, Hkv, D, dtype=torch.bfloat16),
             topk_indices=torch.zeros(B, 1, Hq, dn + 1, W, dtype=torch.int32), decode_nums=dn)
    a.update(over)
    return a


BF = torch.bfloat16
BAD = {
    "q_4d": dict(q=torch.zeros(2, 3, 4, 64, dtype=BF)),
    "sq_2": dict(q=torch.zeros(2, 2, 3, 4, 64, dtype=BF), topk_indices=torch.zeros(2, 2, 4, 3, 3, dtype=torch.int32)),
    "k_context_3d": dict(k_context=torch.zeros(10, 2, 64, dtype=BF), v_context=torch.zeros(10, 2, 64, dtype=BF)),
    "k_context_batch": dict(k_context=torch.zeros(3, 5, 2, 64, dtype=BF), v_context=torch.zeros(3, 5, 2, 64, dtype=BF)),
    "v_context_shape": dict(v_context=torch.zeros(2, 6, 2, 64, dtype=BF)),
    "k_context_dim": dict(k_context=torch.zeros(2, 5, 2, 32, dtype=BF), v_context=torch.zeros(2, 5, 2, 32, dtype=BF)),
    "k_beam_shape": dict(k_beam=torch.zeros(2, 7, 2, 64, dtype=BF)),
    "v_beam_shape": dict(v_beam=torch.zeros(2, 6, 1, 64, dtype=BF)),
    "topk_4d": dict(topk_indices=torch.zeros(2, 4, 3, 3, dtype=torch.int32)),
    "topk_heads": dict(topk_indices=torch.zeros(2, 1, 2, 3, 3, dtype=torch.int32)),
    "topk_width": dict(topk_indices=torch.zeros(2, 1, 4, 3, 4, dtype=torch.int32)),
    "decode_nums_past_max": dict(topk_indices=torch.zeros(2, 1, 4, 1, 3, dtype=torch.int32)),
    "heads_not_divisible": dict(q=torch.zeros(2, 1, 3, 3, 64, dtype=BF), topk_indices=torch.zeros(2, 1, 3, 3, 3, dtype=torch.int32)),
    "q_fp32": dict(q=torch.zeros(2, 1, 3, 4, 64)),
    "mixed_dtypes": dict(k_beam=torch.zeros(2, 6, 2, 64, dtype=torch.float16)),
    "topk_fp": dict(topk_indices=torch.zeros(2, 1, 4, 3, 3)),
    "head_dim_32": dict(q=torch.zeros(2, 1, 3, 4, 32, dtype=BF), k_context=torch.zeros(2, 5, 2, 32, dtype=BF),
                        v_context=torch.zeros(2, 5, 2, 32, dtype=BF), k_beam=torch.zeros(2, 6, 2, 32, dtype=BF),
                        v_beam=torch.zeros(2, 6, 2, 32, dtype=BF)),
    "q_inner_stride": dict(q=torch.zeros(2, 1, 3, 4, 128, dtype=BF)[..., ::2]),
    "backend_x": dict(backend="x"),
    "both_lengths": dict(seqused_k=torch.zeros(2, dtype=torch.int32), cu_seqlens_k=torch.zeros(3, dtype=torch.int32)),
    "seqused_int64": dict(seqused_k=torch.zeros(2, dtype=torch.int64)),
    "cu_seqlens_length": dict(k_context=torch.zeros(10, 2, 64, dtype=BF), v_context=torch.zeros(10, 2, 64, dtype=BF),
                              cu_seqlens_k=torch.zeros(2, dtype=torch.int32)),
    "cpu_tensors": dict(),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_validation(name):
    import mi355_native as N
    from beam_decode_attn import beam_decode_attn

    with pytest.raises(N.NativeError) as e:
        beam_decode_attn(**_args(**BAD[name]))
    assert str(e.value)
    if name in ("backend_x", "both_lengths"):
        assert isinstance(e.value, ValueError)
    if name == "k_beam_shape":
        assert "(2, 7, 2, 64)" in str(e.value)      # the offending shape is in the message


def test_backward_is_refused_and_signature_matches():
    import inspect

    from beam_decode_attn import BeamDecodeAttn, beam_decode_attn

    with pytest.raises(NotImplementedError, match="forward-only"):
        BeamDecodeAttn.backward(None, None, None)
    names = list(inspect.signature(beam_decode_attn).parameters)
    assert names[:13] == ["q", "k_context", "v_context", "k_beam", "v_beam", "topk_indices", "decode_nums", "softmax_scale",
                          "return_lse", "out", "backend", "seqused_k", "cu_seqlens_k"]
    d = {k: v.default for k, v in inspect.signature(beam_decode_attn).parameters.items()}
    assert d["softmax_scale"] is None and d["return_lse"] is False and d["out"] is None and d["backend"] == "dsl"


def test_interface_module_resolves_from_its_directory_alone():
    """what sid-gr-inference does: the directory on sys.path, importlib.import_module("interface"); in a fresh interpreter
    that knows nothing of this package, and with cutlass / quack made unimportable"""
    code = (
        "import sys, importlib\n"
        "sys.modules['cutlass'] = None; sys.modules['quack'] = None\n"
        f"sys.path.insert(0, {os.path.join(PKG, 'gr_decode_atten')!r})\n"
        "m = importlib.import_module('interface')\n"
        "assert callable(m.beam_decode_attn) and issubclass(m.BeamDecodeAttn, __import__('torch').autograd.Function)\n"
        "print('ok')\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd="/")
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr
