"""CPU checks around the fused HSTU layer (fused_hstu_op.py, hstu_addmm.py) that need no GPU:

1. the float64 twin of tests/fused_layer_twin.py: its autograd gradients agree with central finite differences at a tiny
   shape, and its attention stage agrees with oracle.hstu_oracle.hstu_attn_fwd;
2. fused_hstu_op and every hstu_addmm function carry the parameter names, order and defaults recorded from the reference in
   tests/golden/fused_layer_signatures.json (dz_out is the one extra parameter; the enum default is compared by member name);
3. argument errors that are raised before any kernel runs, and the modules import nothing of nvtx / commons / configs / triton."""
import ast
import inspect
import json
import os

import numpy as np
import pytest
import torch

import fused_layer_twin as L
from oracle import hstu_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fused_layer_signatures.json")


def _tiny(**kw):
    return L.config([3, 0, 2], hidden=8, H=2, d=4, **kw)


@pytest.mark.parametrize("case", ["causal", "targets+contexts, dropout, no residual", "plain input norm"])
def test_twin_gradients_agree_with_finite_differences(case):
    cfg = {"causal": _tiny(),
           "targets+contexts, dropout, no residual": _tiny(num_targets=[1, 0, 1], num_contextuals=[1, 0, 0], p=0.3, training=True,
                                                           seed=11, residual=False),
           "plain input norm": _tiny(learnable_input_norm=False)}[case]
    p = L.make_params(cfg, seed=3)
    g = torch.Generator().manual_seed(5)
    dout = torch.randn(cfg.T, cfg.hidden, generator=g, dtype=torch.float64)
    mask, drop = L.dense_mask(cfg), L.dropout_factor(cfg)
    _, grads = L.twin(p, cfg, dout)
    loss = lambda q: float((L.layer(q, cfg, mask, drop) * dout).sum())   # noqa: E731
    h = 1e-6
    for name, grad in grads.items():
        for _ in range(3):
            direction = torch.randn(p[name].shape, generator=g, dtype=torch.float64)
            plus, minus = dict(p), dict(p)
            plus[name], minus[name] = p[name] + h * direction, p[name] - h * direction
            fd = (loss(plus) - loss(minus)) / (2 * h)
            an = float((grad * direction).sum())
            assert abs(fd - an) <= 1e-6 * (1.0 + abs(an)), (case, name, fd, an)
    if cfg.p > 0:
        assert 0.4 < float((drop != 0).double().mean()) < 0.95


@pytest.mark.parametrize("masks", ["causal", "targets", "targets+contexts", "full"])
def test_twin_attention_agrees_with_the_oracle(masks):
    lengths = [0, 1, 9, 14]
    nt = [0, 0, 2, 5] if "targets" in masks else None
    nc = [0, 1, 2, 3] if "contexts" in masks else None
    cfg = L.config(lengths, hidden=8, H=2, d=4, num_targets=nt, num_contextuals=nc, causal=masks != "full")
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(cfg.T, cfg.H, cfg.d, generator=g, dtype=torch.float64) for _ in range(3))
    got = L.attention(q, k, v, L.dense_mask(cfg), cfg.alpha, cfg.scaling_seqlen)
    want = hstu_oracle.hstu_attn_fwd(q.numpy(), k.numpy(), v.numpy(), cfg.offsets, cfg.alpha, cfg.scaling_seqlen, cfg.causal, nt, nc)
    assert np.abs(got.numpy() - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


def _signature(fn):
    out = []
    for name, prm in inspect.signature(fn).parameters.items():
        assert prm.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
        out.append((name, None if prm.default is inspect.Parameter.empty else prm.default))
    return out


def _same_default(ours, literal):
    if literal is None:
        return ours is None
    if literal.startswith("KernelBackend."):
        return getattr(ours, "name", None) == literal.split(".", 1)[1]
    return ours == ast.literal_eval(literal) and type(ours) is type(ast.literal_eval(literal))


def test_signatures_are_the_reference_s():
    import fused_hstu_op as F
    import hstu_addmm as A

    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(["fused_hstu_op", "triton_addmm_silu_fwd", "triton_addmm_silu_bwd", "triton_addmm",
                                     "torch_addmm_silu_fwd", "triton_silu_fwd", "triton_silu_bwd", "triton_silu"])
    assert len(golden["fused_hstu_op"]) == 29
    for name, want in golden.items():
        fn = getattr(F if name == "fused_hstu_op" else A, name)
        got = _signature(fn)
        if name == "triton_addmm_silu_bwd":
            assert got[-1] == ("dz_out", None)
            got = got[:-1]
        assert [g[0] for g in got] == [w[0] for w in want], name
        for (pname, ours), (_, literal) in zip(got, want):
            has_default = inspect.signature(fn).parameters[pname].default is not inspect.Parameter.empty
            assert has_default == (literal is not None), (name, pname)
            if has_default:
                assert _same_default(ours, literal), (name, pname, ours, literal)
    # the autograd function's forward takes the same 29 after ctx
    fwd = list(inspect.signature(F.FusedHSTULayerFunction.forward).parameters)
    assert fwd[0] == "ctx" and fwd[1:] == [w[0] for w in golden["fused_hstu_op"]]
    assert [m for m in F.KernelBackend.__members__] == ["TRITON", "PYTORCH", "CUTLASS"]


def test_modules_import_nothing_the_project_lacks():
    import fused_hstu_op as F
    import hstu_addmm as A

    for mod in (F, A):
        tree = ast.parse(open(mod.__file__).read())
        names = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                names |= {a.name.split(".")[0] for a in node.names}
            elif isinstance(node, ast.ImportFrom):
                names.add((node.module or "").split(".")[0])
        assert not names & {"nvtx", "commons", "configs", "triton", "ops"}, (mod.__name__, names)
        top = {a.name.split(".")[0] for n in tree.body if isinstance(n, ast.Import) for a in n.names} | \
              {(n.module or "").split(".")[0] for n in tree.body if isinstance(n, ast.ImportFrom)}
        assert "hstu" not in top, "import hstu stays inside the call"


def test_argument_errors_come_before_any_kernel():
    import fused_hstu_op as F
    import mi355_native as N

    cfg = L.config([3, 2], hidden=8, H=2, d=32)
    p = {k: (None if t is None else t.to(torch.bfloat16)) for k, t in L.make_params(cfg).items()}
    off = torch.tensor(cfg.offsets, dtype=torch.int64)
    args = lambda **kw: dict(dict(   # noqa: E731
        input=p["x"], seqlen_offsets=off, max_seqlen=cfg.max_seqlen, scaling_seqlen=cfg.max_seqlen, linear_uvqk_weight=p["w_uvqk"],
        linear_uvqk_bias=p["b_uvqk"], linear_proj_weight=p["w_proj"], num_heads=2, linear_dim_per_head=32,
        attention_dim_per_head=32, ln_eps=1e-5, dropout_ratio=0.0, training=False, input_norm_weight=p["w_in"],
        input_norm_bias=p["b_in"], output_norm_weight=p["w_out"], output_norm_bias=p["b_out"]), **kw)
    with pytest.raises(ValueError, match="linear_dim_per_head"):
        F.fused_hstu_op(**args(linear_dim_per_head=16))
    with pytest.raises(ValueError, match="output_norm"):
        F.fused_hstu_op(**args(output_norm_weight=None))
    with pytest.raises(ValueError, match="attn_backend"):
        F.fused_hstu_op(**args(attn_backend="FLASH"))
    with pytest.raises(ValueError, match="target_group_size"):
        F.fused_hstu_op(**args(attn_backend=F.KernelBackend.TRITON, target_group_size=2))
    with pytest.raises(N.NativeError):   # CPU tensors: no eager fallback
        F.fused_hstu_op(**args())
    # T == 0 launches nothing, so it runs anywhere: an empty output, zero parameter gradients of the right shapes
    leaves = {k: (None if t is None else t.clone().requires_grad_(True)) for k, t in p.items()}
    leaves["x"] = torch.zeros(0, 8, dtype=torch.bfloat16, requires_grad=True)
    out = F.fused_hstu_op(**args(input=leaves["x"], seqlen_offsets=torch.zeros(3, dtype=torch.int64), max_seqlen=0,
                                 linear_uvqk_weight=leaves["w_uvqk"], linear_uvqk_bias=leaves["b_uvqk"],
                                 linear_proj_weight=leaves["w_proj"], input_norm_weight=leaves["w_in"],
                                 input_norm_bias=leaves["b_in"], output_norm_weight=leaves["w_out"],
                                 output_norm_bias=leaves["b_out"]))
    assert out.shape == (0, 8) and out.dtype == torch.bfloat16
    out.sum().backward()
    for k, t in leaves.items():
        assert t.grad is not None and t.grad.shape == t.shape and bool((t.grad == 0).all()), k
