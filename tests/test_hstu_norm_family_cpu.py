"""CPU checks of the HSTU norm family (group norm mul dropout, swish layer norm, RMS norm) that need no GPU:

1. the float64 twin of tests/norm_family_twin.py against the reference's PyTorch statement (tests/golden/norm_family_golden.npz,
   an fp32 computation): every golden array lies within the twin's own fp32 bounds;
2. the bounds can be met: an fp32 emulation of the arithmetic of include/recsys_amd.h, written here without the twin, with
   the row sums taken in two different chunk orders, passes every bound for bf16 / fp16 / fp32 outputs at
   (N, H, L) = (67, 4, 64) and (5, 3, 344), and at D = 1032 for swish and RMS;
3. the bounds bite: six wrong variants of that emulation each fail at least one bound on the same inputs;
4. the surface: signatures, exported symbols, error codes of the C ABI, workspace sizes, launch parameters, refusals."""
import inspect
import os

import numpy as np
import pytest
import torch

import norm_family_twin as F

EPS = 1e-5
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
GN_SHAPES = [(67, 4, 64), (5, 3, 344)]
ROW_SHAPES = [(67, 1032), (5, 1032)]
SEED = 77
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_family_golden.npz")


def _ratios(pairs):
    """{name: worst |err| / bound}"""
    return {name: F.worst(got, ref, bound) for name, (got, ref, bound) in pairs.items()}


def _assert_all_within(pairs, tag):
    r = _ratios(pairs)
    print(f"{tag}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{tag}: {bad}"


# ---- 1. twin against golden ----
def test_twin_lies_within_its_fp32_bounds_of_the_golden():
    z = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(z[k])   # noqa: E731
    f32 = torch.float32
    keys = sorted({k.rsplit("_", 1)[0] for k in z.files if k.startswith("gn") and k.endswith("_shape")})
    assert len(keys) >= 6
    for key in keys:
        n, H, L = (int(v) for v in z[key + "_shape"])
        concat = key.endswith("_1")
        st = F.gn_mul_dropout_bwd(t(key + "_dy"), t(key + "_x"), t(key + "_u"), t(key + "_w"), t(key + "_b"), EPS, 0.3, False,
                                  concat, H, L)
        _assert_all_within({"y": (t(key + "_y"), st.out, F.gn_bound_out(st, f32, concat)),
                            "dx": (t(key + "_dx"), st.dx, F.gn_bound_dx(st, f32)),
                            "du": (t(key + "_du"), st.du, F.gn_bound_du(st, f32)),
                            "dw": (t(key + "_dw"), st.dw, F.gn_bound_dw(st, f32)),
                            "db": (t(key + "_db"), st.db, F.gn_bound_db(st, f32))}, key)
    for key in ("swish0", "swish1"):
        st = F.swish_bwd(t(key + "_dy"), t(key + "_x"), t(key + "_w"), t(key + "_b"), EPS)
        _assert_all_within({"y": (t(key + "_y"), st.y, F.swish_bound_y(st, f32)),
                            "dx": (t(key + "_dx"), st.dx, F.swish_bound_dx(st, f32)),
                            "dw": (t(key + "_dw"), st.dw, F.swish_bound_dw(st, f32)),
                            "db": (t(key + "_db"), st.db, F.swish_bound_db(st, f32))}, key)


# ---- 2. / 3. the fp32 emulation ----
def _sum(t, order):
    """fp32 sum over the last dimension: order 0 adds chunks of 8 from the left, order 1 chunks of 64 from the right"""
    c = (8, 64)[order]
    parts = [p.sum(-1) for p in t.split(c, dim=-1)]
    if order:
        parts = parts[::-1]
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc.unsqueeze(-1)


def _col_sum(t):
    """fp32 sum over the rows, one row at a time"""
    acc = torch.zeros_like(t[0])
    for r in range(t.size(0)):
        acc = acc + t[r]
    return acc


def _gn_inputs(n, H, L, dtype, concat):
    g = torch.Generator().manual_seed(100 * H + L)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    D = H * L
    return ((r(n, D) + 1.5).to(dtype), r(n, D).to(dtype), (1 + 0.1 * r(H)).to(dtype), (0.1 * r(H)).to(dtype),
            r(n, 3 * D if concat else D).to(dtype))


def _emulate_gn(x, u, w, b, dy, p, concat, H, L, order, wrong=None):
    X, U, G = x.float(), u.float(), dy.float()
    n, D = X.shape
    X3, U3 = X.reshape(n, H, L), U.reshape(n, H, L)
    W, B = w.float().reshape(1, H, 1), b.float().reshape(1, H, 1)
    fL = torch.tensor(float(L))
    mean = _sum(X3, order) / fL
    var = _sum((X3 - mean) ** 2, order) / (torch.tensor(float(L - 1)) if wrong == "var_l_minus_1" else fL)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(EPS))
    ms, rs = (mean.roll(-1, 1), rstd.roll(-1, 1)) if wrong == "next_head_stats" else (mean, rstd)
    xh = (X3 - ms) * rs
    gn = xh * W + B
    den = torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)
    if p > 0:
        k = [F.keep_mask(SEED, n, D, i, p) for i in ((0, 1, 2) if concat else (0, 0, 0))]
        drop = lambda v, i: torch.where(k[i], v / den, torch.zeros(()))   # noqa: E731
    else:
        drop = lambda v, i: v   # noqa: E731
    t = (gn * U3).reshape(n, D)
    if concat:
        out = torch.cat([drop(U, 0), drop(X, 1), drop(t, 2)], 1)
        dt, du_extra, extra = drop(G[:, 2 * D:], 2), drop(G[:, :D], 0), drop(G[:, D:2 * D], 1)
    else:
        out, dt, du_extra, extra = drop(t, 2), drop(G, 2), torch.zeros_like(X), torch.zeros_like(X)
    dt3 = dt.reshape(n, H, L)
    du = (dt3 * gn).reshape(n, D) + du_extra
    gp = dt3 * U3
    g = W * gp
    c1, c2 = _sum(xh * g, order) / fL, _sum(g, order) / fL
    if wrong == "no_c2":
        c2 = torch.zeros_like(c2)
    dx = ((g - (xh * c1 + c2)) * rs).reshape(n, D) + extra
    dw = _col_sum(_sum(gp * xh, order).reshape(n, H))
    db = _col_sum(_sum(gp, order).reshape(n, H))
    if wrong == "dw_whole_row":
        dw = dw.sum().expand(H).clone()
    return dict(mean=mean.reshape(-1), rstd=rstd.reshape(-1), out=out, du=du, dx=dx, dw=dw, db=db)


def _gn_pairs(e, st, dtype, concat):
    return {"mean": (e["mean"], st.mean, F.gn_bound_mean(st)), "rstd": (e["rstd"], st.rstd, F.gn_bound_rstd(st)),
            "out": (e["out"].to(dtype), st.out, F.gn_bound_out(st, dtype, concat)),
            "du": (e["du"].to(dtype), st.du, F.gn_bound_du(st, dtype)), "dx": (e["dx"].to(dtype), st.dx, F.gn_bound_dx(st, dtype)),
            "dw": (e["dw"].to(dtype), st.dw, F.gn_bound_dw(st, dtype)), "db": (e["db"].to(dtype), st.db, F.gn_bound_db(st, dtype))}


def _row_inputs(n, D, dtype):
    g = torch.Generator().manual_seed(D + n)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return (r(n, D) + 1.5).to(dtype), (1 + 0.1 * r(D)).to(dtype), (0.1 * r(D)).to(dtype), r(n, D).to(dtype)


def _emulate_swish(x, w, b, dy, order, wrong=None):
    X, W, B, G = x.float(), w.float(), b.float(), dy.float()
    fD = torch.tensor(float(X.size(1)))
    mean = _sum(X, order) / fD
    rstd = 1.0 / torch.sqrt(_sum((X - mean) ** 2, order) / fD + torch.tensor(EPS))
    xh = (X - mean) * rstd
    s = 1.0 / (1.0 + torch.exp(-(xh * W + B)))
    q = ((G * X) * s) * (1.0 - s)
    g = W * q
    c1, c2 = _sum(xh * g, order) / fD, _sum(g, order) / fD
    dx = (g - (xh * c1 + c2)) * rstd
    if wrong != "no_dy_s":
        dx = dx + G * s
    return dict(mean=mean.reshape(-1), rstd=rstd.reshape(-1), y=s * X, dx=dx, dw=_col_sum(q * xh), db=_col_sum(q))


def _swish_pairs(e, st, dtype):
    return {"mean": (e["mean"], st.mean, F.bound_mean(st)), "rstd": (e["rstd"], st.rstd, F.bound_rstd(st)),
            "y": (e["y"].to(dtype), st.y, F.swish_bound_y(st, dtype)), "dx": (e["dx"].to(dtype), st.dx, F.swish_bound_dx(st, dtype)),
            "dw": (e["dw"].to(dtype), st.dw, F.swish_bound_dw(st, dtype)), "db": (e["db"].to(dtype), st.db, F.swish_bound_db(st, dtype))}


def _emulate_rms(x, w, dy, order, wrong=None):
    X, W, G = x.float(), w.float(), dy.float()
    fD = torch.tensor(float(X.size(1)))
    rstd = 1.0 / torch.sqrt(_sum(X * X, order) / fD + torch.tensor(EPS))
    xh = X * rstd
    g = W * G
    c1 = _sum(xh * g, order) / fD
    inner = xh * c1 + (_sum(g, order) / fD if wrong == "rms_with_c2" else 0.0)
    return dict(rstd=rstd.reshape(-1), y=xh * W, dx=(g - inner) * rstd, dw=_col_sum(G * xh))


def _rms_pairs(e, st, dtype):
    return {"rstd": (e["rstd"], st.rstd, F.bound_rstd(st)), "y": (e["y"].to(dtype), st.y, F.rms_bound_y(st, dtype)),
            "dx": (e["dx"].to(dtype), st.dx, F.rms_bound_dx(st, dtype)), "dw": (e["dw"].to(dtype), st.dw, F.rms_bound_dw(st, dtype))}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,H,L", GN_SHAPES)
def test_fp32_emulation_of_the_group_norm_meets_every_bound(n, H, L, dtype):
    for p, concat in ((0.0, False), (0.3, True)):
        x, u, w, b, dy = _gn_inputs(n, H, L, dtype, concat)
        st = F.gn_mul_dropout_bwd(dy, x, u, w, b, EPS, p, True, concat, H, L, SEED)
        for order in (0, 1):
            e = _emulate_gn(x, u, w, b, dy, p, concat, H, L, order)
            assert bool((e["out"][~st.kept] == 0).all())
            _assert_all_within(_gn_pairs(e, st, dtype, concat), f"gn {n}x{H}x{L} {dtype} p={p} order={order}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,D", ROW_SHAPES)
def test_fp32_emulation_of_swish_and_rms_meets_every_bound(n, D, dtype):
    x, w, b, dy = _row_inputs(n, D, dtype)
    sw, rm = F.swish_bwd(dy, x, w, b, EPS), F.rms_bwd(dy, x, w, EPS)
    for order in (0, 1):
        _assert_all_within(_swish_pairs(_emulate_swish(x, w, b, dy, order), sw, dtype), f"swish {n}x{D} {dtype} order={order}")
        _assert_all_within(_rms_pairs(_emulate_rms(x, w, dy, order), rm, dtype), f"rms {n}x{D} {dtype} order={order}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,H,L", GN_SHAPES)
@pytest.mark.parametrize("wrong", ["var_l_minus_1", "next_head_stats", "no_c2", "dw_whole_row"])
def test_wrong_group_norms_fail_a_bound(wrong, n, H, L, dtype):
    x, u, w, b, dy = _gn_inputs(n, H, L, dtype, False)
    st = F.gn_mul_dropout_bwd(dy, x, u, w, b, EPS, 0.0, True, False, H, L, SEED)
    r = _ratios(_gn_pairs(_emulate_gn(x, u, w, b, dy, 0.0, False, H, L, 0, wrong), st, dtype, False))
    assert max(r.values()) > 1.0, (wrong, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,D", ROW_SHAPES)
def test_wrong_swish_and_rms_fail_a_bound(n, D, dtype):
    x, w, b, dy = _row_inputs(n, D, dtype)
    r = _ratios(_swish_pairs(_emulate_swish(x, w, b, dy, 0, "no_dy_s"), F.swish_bwd(dy, x, w, b, EPS), dtype))
    assert r["dx"] > 1.0, r
    r = _ratios(_rms_pairs(_emulate_rms(x, w, dy, 0, "rms_with_c2"), F.rms_bwd(dy, x, w, EPS), dtype))
    assert r["dx"] > 1.0, r


def test_twin_gradients_agree_with_autograd():
    n, H, L, p = 9, 3, 8, 0.3
    D = H * L
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True)   # noqa: E731
    x, u, w, b = r(n, D), r(n, D), r(H), r(H)
    dy = torch.randn(n, 3 * D, generator=g, dtype=torch.float64)
    f = [F.keep_mask(SEED, n, D, i, p).double() / (1 - p) for i in range(3)]
    e = float(torch.tensor(EPS, dtype=torch.float32))
    t = (torch.nn.functional.group_norm(x.view(n, H, L), H, w, b, e) * u.view(n, H, L)).view(n, D)
    want = torch.autograd.grad(torch.cat([u * f[0], x * f[1], t * f[2]], 1), (x, u, w, b), dy)
    st = F.gn_mul_dropout_bwd(dy, x, u, w, b, EPS, p, True, True, H, L, SEED)
    for got, ref in zip((st.dx, st.du, st.dw, st.db), want):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # RMS norm: no PyTorch statement in the reference; the formula under autograd
    wd = r(D)
    y = x * torch.rsqrt((x * x).mean(1, keepdim=True) + e) * wd
    want = torch.autograd.grad(y, (x, wd), dy[:, :D])
    rm = F.rms_bwd(dy[:, :D], x, wd, EPS)
    assert float((rm.y - y.detach()).abs().max()) <= 1e-12
    for got, ref in zip((rm.dx, rm.dw), want):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# ---- 4. the surface ----
SIGNATURES = {
    "triton_group_norm_mul_dropout_fwd": [("x",), ("u",), ("weight",), ("bias",), ("eps",), ("dropout_ratio",), ("training",),
                                          ("concat_ux", False), ("num_heads", 1), ("linear_dim", -1), ("seed", None)],
    "triton_group_norm_mul_dropout_bwd": [("dy",), ("x",), ("u",), ("weight",), ("bias",), ("mean",), ("rstd",), ("BLOCK_D",),
                                          ("BLOCK_H",), ("num_warps",), ("eps",), ("training",), ("dropout_ratio",), ("seed", None),
                                          ("concat_ux", False), ("num_heads", 1), ("linear_dim", -1), ("compute_y", False),
                                          ("du", None)],
    "triton_swish_layer_norm": [("x",), ("weight",), ("bias",), ("eps",)],
    "triton_rms_norm": [("x",), ("weight",), ("eps",)],
}
SYMBOLS = ("mi355_hstu_gn_mul_dropout_fwd", "mi355_hstu_gn_mul_dropout_bwd", "mi355_hstu_gn_mul_dropout_bwd_workspace_bytes",
           "mi355_hstu_swish_layer_norm_fwd", "mi355_hstu_swish_layer_norm_bwd", "mi355_hstu_swish_layer_norm_bwd_workspace_bytes",
           "mi355_hstu_rms_norm_fwd", "mi355_hstu_rms_norm_bwd", "mi355_hstu_rms_norm_bwd_workspace_bytes")


def test_signatures_and_exports():
    import hstu_norm as H

    for name, want in SIGNATURES.items():
        params = inspect.signature(getattr(H, name)).parameters.values()
        got = [(q.name,) if q.default is inspect.Parameter.empty else (q.name, q.default) for q in params]
        assert got == want, name
    for name in H.__all__:
        if name.startswith("triton_"):
            assert getattr(H, name[len("triton_"):]) is getattr(H, name) and name[len("triton_"):] in H.__all__, name
    for name in list(SIGNATURES) + ["GroupNormMulDropoutFunction", "SwishLayerNormFunction", "RMSNormFunction"]:
        assert name in H.__all__, name
    for cls in (H.GroupNormMulDropoutFunction, H.SwishLayerNormFunction, H.RMSNormFunction):
        assert issubclass(cls, torch.autograd.Function)
    assert "group_norm is not implemented" not in H.__doc__


def test_symbols_are_exported_and_bound():
    import mi355_native as N

    lib = N.lib()
    for name in SYMBOLS:
        assert name in N.exported_symbols(), name
        assert getattr(lib, name).argtypes == N.signature_of(name), name
    # at least the [2][H] (or [2][D], [1][D]) partials of one block; nothing negative for no rows
    assert lib.mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(1031, 4, 64) >= 2 * 4 * 4
    assert lib.mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(67, 257, 8) >= 2 * 257 * 4
    assert lib.mi355_hstu_swish_layer_norm_bwd_workspace_bytes(1031, 1024) >= 2 * 1024 * 4
    assert lib.mi355_hstu_rms_norm_bwd_workspace_bytes(1031, 1024) >= 1024 * 4
    assert lib.mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(0, 4, 64) >= 0
    assert lib.mi355_hstu_swish_layer_norm_bwd_workspace_bytes(0, 8) >= 0 and lib.mi355_hstu_rms_norm_bwd_workspace_bytes(0, 8) >= 0


def test_bad_arguments_are_error_codes():
    import mi355_native as N

    lib = N.lib()
    BF16, F16, F32 = N.DT_BF16, N.DT_F16, N.DT_F32

    def gn_fwd(D=8, dtype=BF16, wdtype=F32, H=2, L=4, p=0.3):
        return lib.mi355_hstu_gn_mul_dropout_fwd(None, D, None, D, L, H, L, 4, D, dtype, None, None, wdtype, EPS, p, 1, 5, 0, None,
                                                 D, None, None, None)

    def gn_bwd(D=8, dtype=BF16, wdtype=F32, H=2, L=4, p=0.3):
        return lib.mi355_hstu_gn_mul_dropout_bwd(None, D, None, D, None, D, L, H, L, 4, D, dtype, None, None, wdtype, None, None,
                                                 p, 1, 5, 0, None, D, None, D, L, None, None, None, 0, None, 0, None)

    def sw_fwd(D=8, dtype=BF16, wdtype=F32):
        return lib.mi355_hstu_swish_layer_norm_fwd(None, D, 4, D, dtype, None, None, wdtype, EPS, None, D, None, None, None)

    def sw_bwd(D=8, dtype=BF16, wdtype=F32):
        return lib.mi355_hstu_swish_layer_norm_bwd(None, D, None, D, 4, D, dtype, None, None, wdtype, None, None, None, D, None,
                                                   None, None, 0, None)

    def rms_fwd(D=8, dtype=BF16, wdtype=F32):
        return lib.mi355_hstu_rms_norm_fwd(None, D, 4, D, dtype, None, wdtype, EPS, None, D, None, None)

    def rms_bwd(D=8, dtype=BF16, wdtype=F32):
        return lib.mi355_hstu_rms_norm_bwd(None, D, None, D, 4, D, dtype, None, wdtype, None, None, D, None, None, 0, None)

    for call in (gn_fwd, gn_bwd, sw_fwd, sw_bwd, rms_fwd, rms_bwd):
        for kw, text in (({"D": 8193}, b"D must be in 1 .. 8192"), ({"D": 0}, b"D must be in 1 .. 8192"),
                         ({"dtype": 7}, b"unsupported dtype"), ({"dtype": BF16, "wdtype": F16}, b"fp32 or have the dtype of the rows")):
            assert call(**kw) == -1 and text in lib.mi355_last_error(), (call.__name__, kw)
        # with every argument in range the null buffers are the error
        assert call() == -1 and b"null buffer" in lib.mi355_last_error(), call.__name__
    for call in (gn_fwd, gn_bwd):
        assert call(H=2, L=3) == -1 and b"H * L == D" in lib.mi355_last_error()
        for p in (1.0, -0.1, 1.5):
            assert call(p=p) == -1 and b"dropout_ratio must be in [0, 1)" in lib.mi355_last_error()


def test_launch_parameters_and_refusals():
    import hstu_norm as H
    import mi355_native as N

    assert H._group_launch_params(64, 4, 2) == (64, 4, 1)
    assert H._group_launch_params(8, 257, 2) == (8, 512, 8)
    with pytest.raises(RuntimeError, match="This group norm doesn't support num_heads \\* linear_dim >= 64KB."):
        H._group_launch_params(4096, 16, 2)
    x, u, w, b = torch.randn(4, 8), torch.randn(4, 8), torch.ones(2), torch.zeros(2)
    m, r = torch.zeros(8), torch.ones(8)
    with pytest.raises(NotImplementedError, match="group norm has no CPU implementation"):
        H.triton_norm_mul_dropout(x, u, w, b, EPS, 0.0, False, group_norm=True, num_heads=2, linear_dim=4)
    with pytest.raises(N.NativeError):
        H.triton_group_norm_mul_dropout_fwd(x, u, w, b, EPS, 0.0, False, False, 2, 4)
    with pytest.raises(N.NativeError):
        H.triton_group_norm_mul_dropout_bwd(x, x, u, w, b, m, r, 4, 2, 1, EPS, False, 0.0, 0, False, 2, 4)
    with pytest.raises(N.NativeError):
        H.triton_swish_layer_norm(x, torch.ones(8), torch.zeros(8), EPS)
    with pytest.raises(N.NativeError):
        H.triton_rms_norm(x, torch.ones(8), EPS)
    # shape errors name the argument
    with pytest.raises(ValueError, match="x must have num_heads \\* linear_dim"):
        H.triton_group_norm_mul_dropout_fwd(x, u, w, b, EPS, 0.0, False, False, 2, 3)
    with pytest.raises(ValueError, match="weight"):
        H.triton_group_norm_mul_dropout_fwd(x, u, torch.ones(3), b, EPS, 0.0, False, False, 2, 4)
    with pytest.raises(ValueError, match="bias"):
        H.triton_group_norm_mul_dropout_fwd(x, u, w, torch.zeros(8), EPS, 0.0, False, False, 2, 4)
    with pytest.raises(ValueError, match="weight"):
        H.triton_group_norm_mul_dropout_fwd(x, u, None, b, EPS, 0.0, False, False, 2, 4)
    with pytest.raises(ValueError, match="bias"):
        H.triton_swish_layer_norm(x, torch.ones(8), None, EPS)
    with pytest.raises(ValueError, match="weight"):
        H.triton_rms_norm(x, torch.ones(7), EPS)
