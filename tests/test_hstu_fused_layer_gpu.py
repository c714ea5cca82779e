"""GPU checks of the fused HSTU layer (fused_hstu_op.py) against the float64 twin of tests/fused_layer_twin.py.

Criterion: the reference's own rule for this layer (commons/utils/hstu_assert_close.py, as test/test_hstu_op.py:708-712 uses it):
for the output and for every gradient, max |fused - twin| <= 2 x (forward) or 5 x (gradients) max |native - twin|, where
`native` is the same layer from plain torch ops (F.layer_norm, F.linear, F.silu, dense masked attention, the twin's dropout mask)
in the row dtype on the GPU, in the same test.  To keep the rule honest, max |native - twin| must be positive and at most 5 % of
max |twin| for every compared tensor (checked on a CPU with bf16 torch for these seeds before the first GPU run), and no tensor
or element is left out.  Both maxima are printed.

Shapes, the smallest that cross each boundary.  A: hidden 64, H = 2, d = 32 (uvqk width 256), lengths [0, 1, 37, 130] -- an empty
sequence, one token, one past a 32-row tile, two past a 64- and a 128-row tile -- max_seqlen 130, T = 168.  B: hidden 136,
H = 1, d = 64, lengths [70].  The int num_contextuals = 2 case runs on B: a sequence shorter than its contexts (A has two) is
outside what the reference defines."""
import pytest
import torch
import torch.nn.functional as Fn

import fused_layer_twin as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPE_A = dict(lengths=[0, 1, 37, 130], hidden=64, H=2, d=32)
SHAPE_B = dict(lengths=[70], hidden=136, H=1, d=64)
SEED = 0x5EED_0123_4567
NAMES = {"x": "input", "w_uvqk": "linear_uvqk_weight", "b_uvqk": "linear_uvqk_bias", "w_proj": "linear_proj_weight",
         "w_in": "input_norm_weight", "b_in": "input_norm_bias", "w_out": "output_norm_weight", "b_out": "output_norm_bias"}


def _F():
    import fused_hstu_op as F

    return F


def _same(a, b):
    if a is None or b is None:
        return a is b
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _setup(shape, dtype, seed=1, **kw):
    """(cfg, parameters in the row dtype on the GPU, the same values in float64 on the CPU, dout)"""
    cfg = L.config(seed=SEED, **shape, **kw)
    p64 = L.make_params(cfg, seed=seed)
    pd = {k: (None if t is None else t.to(dtype).to(DEV)) for k, t in p64.items()}
    p64 = {k: (None if t is None else t.cpu().double()) for k, t in pd.items()}
    g = torch.Generator().manual_seed(seed + 100)
    dout = torch.randn(cfg.T, cfg.hidden, generator=g).to(dtype).to(DEV)
    return cfg, pd, p64, dout


def _fused(cfg, pd, dout, backend=None, contextuals="tensor", **flags):
    """(out, {name: grad}) of fused_hstu_op"""
    F = _F()
    leaves = {k: (None if t is None else t.detach().clone().requires_grad_(True)) for k, t in pd.items()}
    nc = cfg.num_contextuals
    if nc is not None and contextuals == "tensor":
        nc = torch.tensor(nc, dtype=torch.int64, device=DEV)
    elif nc is not None:
        assert len(set(nc)) == 1
        nc = int(nc[0])
    out = F.fused_hstu_op(
        input=leaves["x"], seqlen_offsets=torch.tensor(cfg.offsets, dtype=torch.int64, device=DEV), max_seqlen=cfg.max_seqlen,
        scaling_seqlen=cfg.scaling_seqlen, linear_uvqk_weight=leaves["w_uvqk"], linear_uvqk_bias=leaves["b_uvqk"],
        linear_proj_weight=leaves["w_proj"], num_heads=cfg.H, linear_dim_per_head=cfg.d, attention_dim_per_head=cfg.d,
        ln_eps=cfg.eps, dropout_ratio=cfg.p, training=cfg.training, input_norm_weight=leaves["w_in"],
        input_norm_bias=leaves["b_in"], output_norm_weight=leaves["w_out"], output_norm_bias=leaves["b_out"],
        attn_backend=backend or F.KernelBackend.CUTLASS,
        num_targets=None if cfg.num_targets is None else torch.tensor(cfg.num_targets, dtype=torch.int64, device=DEV),
        num_contextuals=nc, target_group_size=cfg.target_group_size, alpha=cfg.alpha, causal=cfg.causal, seed=cfg.seed,
        residual=cfg.residual, **flags)
    names = [k for k in L.PARAMS if leaves[k] is not None]
    grads = torch.autograd.grad(out, [leaves[k] for k in names], dout)
    return out.detach(), dict(zip(names, grads))


def _native(cfg, pd, dout):
    """the same layer from torch's own ops in the row dtype on the GPU"""
    mask, drop = L.dense_mask(cfg).to(DEV), L.dropout_factor(cfg).to(dout.dtype).to(DEV)
    ln = lambda x, w, b, eps: Fn.layer_norm(x, (x.size(1),), w, b, eps)   # noqa: E731
    linear = lambda x, w, b: Fn.linear(x, w.t(), b)   # noqa: E731
    return L.run(lambda q: L.layer(q, cfg, mask, drop, ln=ln, linear=linear, silu=Fn.silu), pd, dout)


def _judge(tag, fused, native, twin, factor):
    f, n, t = (a.detach().cpu().double() for a in (fused, native, twin))
    assert f.shape == t.shape and n.shape == t.shape, tag
    if t.numel() == 0:
        return
    ef, en, mt = float((f - t).abs().max()), float((n - t).abs().max()), float(t.abs().max())
    print(f"{tag}: max |fused - twin| = {ef:.3e}, max |native - twin| = {en:.3e}, max |twin| = {mt:.3e}, "
          f"ratio {ef / en if en > 0 else float('inf'):.2f} (allowed {factor})")
    assert bool(torch.isfinite(f).all()), tag
    assert en > 0.0, tag + ": the native layer equals the twin, the rule would be empty"
    assert en <= 0.05 * mt, tag + f": the native layer is {en / mt:.3f} of max |twin| off, the rule would be loose"
    assert ef <= factor * en, tag + f": {ef:.3e} > {factor} x {en:.3e}"


TARGETS_CONTEXTS = dict(num_targets=[0, 0, 5, 9], num_contextuals=[0, 1, 2, 3])
CASES = {
    "A bf16 causal eval": (SHAPE_A, torch.bfloat16, {}, {}),
    "A fp16 causal training p=0.3": (SHAPE_A, torch.float16, dict(training=True, p=0.3), {}),
    "B bf16 causal plain input norm, no residual, training p=0": (
        SHAPE_B, torch.bfloat16, dict(training=True, p=0.0, learnable_input_norm=False, residual=False), {}),
    "A bf16 targets + tensor contexts training p=0.3": (SHAPE_A, torch.bfloat16, dict(training=True, p=0.3, **TARGETS_CONTEXTS), {}),
    "A fp16 targets + tensor contexts eval, no residual": (SHAPE_A, torch.float16, dict(residual=False, **TARGETS_CONTEXTS), {}),
    "B bf16 int contexts 2 under TRITON eval": (SHAPE_B, torch.bfloat16, dict(num_contextuals=[2]),
                                                dict(backend="TRITON", contextuals="int")),
    "B bf16 int contexts 2 under TRITON training p=0.3": (SHAPE_B, torch.bfloat16, dict(num_contextuals=[2], training=True, p=0.3),
                                                          dict(backend="TRITON", contextuals="int")),
    "A bf16 plain input norm training p=0.3 targets": (
        SHAPE_A, torch.bfloat16, dict(training=True, p=0.3, learnable_input_norm=False, num_targets=[0, 0, 5, 9]), {}),
    "A bf16 causal training p=0 PYTORCH": (SHAPE_A, torch.bfloat16, dict(training=True, p=0.0), dict(backend="PYTORCH")),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fused_layer_against_the_twin(case):
    shape, dtype, kw, how = CASES[case]
    cfg, pd, p64, dout = _setup(shape, dtype, **kw)
    how = dict(how)
    if "backend" in how:
        how["backend"] = _F().KernelBackend[how["backend"]]
    out_f, g_f = _fused(cfg, pd, dout, **how)
    out_n, g_n = _native(cfg, pd, dout)
    out_t, g_t = L.twin(p64, cfg, dout)
    assert out_f.dtype == dtype and out_f.shape == (cfg.T, cfg.hidden)
    _judge(f"{case}: out", out_f, out_n, out_t, 2.0)
    assert sorted(g_f) == sorted(g_t) == sorted(g_n)
    for name in g_t:
        assert g_f[name].dtype == dtype
        _judge(f"{case}: d {NAMES[name]}", g_f[name], g_n[name], g_t[name], 5.0)
    if cfg.training and cfg.p == 0.0:
        # nothing dropped: the same bits as training=False
        cfg2, pd2, _, _ = _setup(shape, dtype, **dict(kw, training=False))
        assert _same(_fused(cfg2, pd2, dout, **how)[0], out_f)


def _training_a(**kw):
    return _setup(SHAPE_A, torch.bfloat16, training=True, p=0.3, **kw)


def _gemm_repeatable(m, k, n, dtype=torch.bfloat16):
    a, b = torch.randn(m, k, device=DEV).to(dtype), torch.randn(k, n, device=DEV).to(dtype)
    return _same(torch.mm(a, b), torch.mm(a, b))


def test_recompute_flags_change_no_bit():
    cfg, pd, _, dout = _training_a(**TARGETS_CONTEXTS)
    runs = {(ln, silu): _fused(cfg, pd, dout, recompute_input_layernorm=ln, recompute_input_silu=silu)
            for ln in (False, True) for silu in (False, True)}
    base_out, base_g = runs[(False, False)]
    repeatable = _gemm_repeatable(cfg.T, cfg.hidden, 4 * cfg.H * cfg.d) and _gemm_repeatable(cfg.hidden, cfg.T, 4 * cfg.H * cfg.d)
    for key, (out, grads) in runs.items():
        assert _same(out, base_out), f"output differs with recompute flags {key} (torch.mm repeatable at these shapes: {repeatable})"
    for ln in (False, True):
        for name, g in runs[(ln, True)][1].items():
            assert _same(g, runs[(ln, False)][1][name]), \
                f"d {NAMES[name]} differs with recompute_input_silu (layernorm {ln}; torch.mm repeatable: {repeatable})"


def _saved_bytes(cfg, pd, **flags):
    seen = {}

    def pack(t):
        seen[(t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape))] = t.numel() * t.element_size()
        return t

    F = _F()
    leaves = {k: (None if t is None else t.detach().clone().requires_grad_(True)) for k, t in pd.items()}
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = F.fused_hstu_op(leaves["x"], torch.tensor(cfg.offsets, dtype=torch.int64, device=DEV), cfg.max_seqlen,
                              cfg.scaling_seqlen, leaves["w_uvqk"], leaves["b_uvqk"], leaves["w_proj"], cfg.H, cfg.d, cfg.d, cfg.eps,
                              cfg.p, cfg.training, leaves["w_in"], leaves["b_in"], leaves["w_out"], leaves["b_out"], seed=cfg.seed,
                              **flags)
    del out
    return sum(seen.values())


def test_recompute_flags_save_the_bytes_they_promise():
    cfg, pd, _, _ = _training_a()
    item = 2
    base = _saved_bytes(cfg, pd)
    silu = _saved_bytes(cfg, pd, recompute_input_silu=True)
    ln = _saved_bytes(cfg, pd, recompute_input_layernorm=True)
    both = _saved_bytes(cfg, pd, recompute_input_layernorm=True, recompute_input_silu=True)
    print(f"bytes saved for backward: {base} plain, {silu} recompute silu, {ln} recompute layernorm, {both} both")
    assert base - silu >= cfg.T * 4 * cfg.H * cfg.d * item
    assert base - ln == cfg.T * cfg.hidden * item
    assert base - both >= cfg.T * (4 * cfg.H * cfg.d + cfg.hidden) * item


def test_side_stream_gives_the_same_bits():
    cfg, pd, _, dout = _training_a(**TARGETS_CONTEXTS)
    out0, g0 = _fused(cfg, pd, dout)
    stream, event = torch.cuda.Stream(), torch.cuda.Event()
    out1, g1 = _fused(cfg, pd, dout, wgrad_stream=stream, wgrad_event=event)
    event.synchronize()
    torch.cuda.synchronize()
    assert _same(out0, out1)
    for name in g0:
        assert _same(g0[name], g1[name]), f"d {NAMES[name]} differs with a weight-gradient stream"


def test_same_seed_same_bits_other_seed_other_mask():
    cfg, pd, _, dout = _training_a()
    out0, g0 = _fused(cfg, pd, dout)
    out1, g1 = _fused(cfg, pd, dout)
    assert _same(out0, out1) and all(_same(g0[k], g1[k]) for k in g0)
    cfg.seed = SEED + 1
    assert not _same(_fused(cfg, pd, dout)[0], out0)


def test_empty_batch_and_refusals():
    F = _F()
    cfg, pd, _, dout = _setup(dict(lengths=[0, 0], hidden=64, H=2, d=32), torch.bfloat16)
    out, grads = _fused(cfg, pd, dout)
    assert out.shape == (0, 64) and out.dtype == torch.bfloat16
    for name, g in grads.items():
        assert g.shape == pd[name].shape and bool((g == 0).all()), name
    cfg, pd, _, dout = _setup(SHAPE_B, torch.bfloat16)
    off = torch.tensor(cfg.offsets, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="linear_dim_per_head"):
        F.fused_hstu_op(pd["x"], off, 70, 70, pd["w_uvqk"], pd["b_uvqk"], pd["w_proj"], 1, 32, 64, 1e-5, 0.0, False, pd["w_in"],
                        pd["b_in"], pd["w_out"], pd["b_out"])
    p32 = {k: t.float() for k, t in pd.items()}
    with pytest.raises(RuntimeError, match="fp16 and bf16"):
        F.fused_hstu_op(p32["x"], off, 70, 70, p32["w_uvqk"], p32["b_uvqk"], p32["w_proj"], 1, 64, 64, 1e-5, 0.0, False, p32["w_in"],
                        p32["b_in"], p32["w_out"], p32["b_out"])


def test_gradients_meet_in_one_duvqk_buffer(monkeypatch):
    """du, dq, dk, dv are written straight into one [T, 4 H d] buffer, and the SiLU backward runs over it in place"""
    F = _F()
    import hstu  # noqa: F401
    from hstu import hstu_attn_interface as A

    seen = {}
    norm_bwd, attn_bwd, addmm_bwd = F.triton_layer_norm_mul_dropout_bwd, A.hstu_varlen_bwd, F.triton_addmm_silu_bwd

    def spy_norm(*a, **kw):
        seen["du"] = kw["du"]
        return norm_bwd(*a, **kw)

    class SpyGradOut(A._GradOut):   # where the attention kernels are pointed: `to` holds the tensors they write
        def __init__(self, *a):
            super().__init__(*a)
            seen["kernel_targets"] = list(self.to)

    def spy_attn(*a, **kw):
        seen.update(dq=kw["dq"], dk=kw["dk"], dv=kw["dv"])
        out = attn_bwd(*a, **kw)
        assert out[0] is kw["dq"] and out[1] is kw["dk"] and out[2] is kw["dv"]
        return out

    def spy_addmm(*a, **kw):
        if kw.get("silu"):
            seen["duvqk"], seen["dz_out"] = kw["grad_output"], kw["dz_out"]
        return addmm_bwd(*a, **kw)

    monkeypatch.setattr(F, "triton_layer_norm_mul_dropout_bwd", spy_norm)
    monkeypatch.setattr(A, "hstu_varlen_bwd", spy_attn)
    monkeypatch.setattr(A, "_GradOut", SpyGradOut)
    monkeypatch.setattr(F, "triton_addmm_silu_bwd", spy_addmm)
    cfg, pd, _, dout = _training_a()
    _fused(cfg, pd, dout)
    duvqk = seen["duvqk"]
    n = cfg.H * cfg.d
    # the kernels wrote the views themselves: no contiguous stand-in copied back afterwards
    assert all(w is seen[name] for w, name in zip(seen["kernel_targets"], ("dq", "dk", "dv")))
    assert seen["dz_out"] is duvqk and duvqk.shape == (cfg.T, 4 * n) and duvqk.is_contiguous()
    base = duvqk.untyped_storage().data_ptr()
    assert duvqk.untyped_storage().nbytes() == cfg.T * 4 * n * duvqk.element_size()
    for i, name in enumerate(("du", "dv", "dq", "dk")):
        t = seen[name]
        assert t.untyped_storage().data_ptr() == base, name
        assert t.storage_offset() == i * n and t.stride(0) == 4 * n and t.stride(-1) == 1, name
