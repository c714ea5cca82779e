"""Beam-search decode attention on the GPU (beam_decode_attn.py / csrc/beam_decode.hip) against the float64 twin, element by
element under the twin's derived bound (tests/beam_decode_twin.py).  The shapes (tests/beam_decode_cases.py) are the smallest
at which the kernels can go wrong; tests/test_beam_decode_cpu.py checks on the same shapes that the bound can be met and that
it catches mistakes."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from beam_decode_cases import CASE_BY_NAME, CASES, make_inputs  # noqa: E402
from beam_decode_twin import beam_decode_twin, compare  # noqa: E402

pytestmark = pytest.mark.gpu

_TENSORS = ("q", "k_context", "v_context", "k_beam", "v_beam", "topk_indices", "seqused_k", "cu_seqlens_k")


def _to_gpu(inp):
    """the same values on the GPU, strides kept (the layer-select view stays a view)"""
    out = dict(inp)
    for n in _TENSORS:
        t = inp[n]
        if t is None:
            continue
        base = t._base if t._base is not None and not t.is_contiguous() else None
        if base is not None:
            out[n] = base.cuda().as_strided(t.shape, t.stride(), t.storage_offset())
        else:
            out[n] = t.cuda()
    return out


def _twin(inp, ns):
    return beam_decode_twin(inp["q"], inp["k_context"], inp["v_context"], inp["k_beam"], inp["v_beam"], inp["topk_indices"],
                            inp["decode_nums"], seqused_k=inp["seqused_k"], cu_seqlens_k=inp["cu_seqlens_k"], num_splits=ns)


def _run(g, ns=None, **kw):
    from beam_decode_attn import beam_decode_attn

    return beam_decode_attn(g["q"], g["k_context"], g["v_context"], g["k_beam"], g["v_beam"], g["topk_indices"],
                            g["decode_nums"], return_lse=True, seqused_k=g["seqused_k"], cu_seqlens_k=g["cu_seqlens_k"],
                            _num_splits=ns, **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_against_the_twin(case):
    inp = make_inputs(case)
    g = _to_gpu(inp)
    if case.form == "strided":
        assert not g["k_context"].is_contiguous()
    B, _, W, Hq, D = inp["q"].shape
    for ns in case.splits:
        out, lse = _run(g, ns)
        assert out.shape == (B, 1, W, Hq, D) and out.dtype == inp["q"].dtype
        assert lse.shape == (B, 1, W, Hq) and lse.dtype == torch.float32
        r_out, r_lse = compare(out, lse, _twin(inp, ns))
        print(f"{case.name} ns={ns}: worst |err| / bound out {r_out:.3f} lse {r_lse:.3f}")
        assert r_out <= 1 and r_lse <= 1
        out2, lse2 = _run(g, ns)                       # deterministic for a given split count
        assert torch.equal(out, out2) and torch.equal(lse, lse2)
    if case.name == "no_keys":
        assert torch.all(out == 0) and torch.all(lse == -math.inf)


def test_default_split_rule_runs_within_the_bound():
    """the split count the wrapper chooses itself (no _num_splits): a launch small enough that it does split"""
    from beam_decode_attn import num_splits

    case = CASE_BY_NAME["splits_ctx453"]
    inp = make_inputs(case)
    ns = num_splits(case.B, case.W, case.Hq, case.Hkv, case.D, case.ctx)
    out, lse = _run(_to_gpu(inp))
    r_out, r_lse = compare(out, lse, _twin(inp, ns))
    print(f"default split rule ns={ns}: worst |err| / bound out {r_out:.3f} lse {r_lse:.3f}")
    assert r_out <= 1 and r_lse <= 1


def test_surface():
    from beam_decode_attn import beam_decode_attn

    inp = make_inputs(CASE_BY_NAME["beam_dn3_i32"])
    g = _to_gpu(inp)
    args = (g["q"], g["k_context"], g["v_context"], g["k_beam"], g["v_beam"], g["topk_indices"], g["decode_nums"])
    out, lse = beam_decode_attn(*args, return_lse=True)
    o2, none = beam_decode_attn(*args)
    assert none is None and torch.equal(out, o2)
    o3, l3 = beam_decode_attn(*args, return_lse=True, backend="3kernel")
    assert torch.equal(out, o3) and torch.equal(lse, l3)
    buf = torch.full_like(g["q"], float("nan"))
    o4, _ = beam_decode_attn(*args, out=buf)
    assert o4 is buf and torch.equal(buf, out)
    # the interface module sid-gr-inference imports is the same function
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "recsys-examples_amd", "gr_decode_atten"))
    try:
        import interface
    finally:
        sys.path.pop(0)
    o5, l5 = interface.beam_decode_attn(*args, return_lse=True)
    assert torch.equal(out, o5) and torch.equal(lse, l5)
    # forward only
    q = g["q"].clone().requires_grad_(True)
    o6, _ = beam_decode_attn(q, *args[1:])
    with pytest.raises(NotImplementedError, match="forward-only"):
        o6.float().sum().backward()
