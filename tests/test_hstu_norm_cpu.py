"""CPU checks of the HSTU layer norms (hstu_norm over csrc/norm_ops.hip) that need no GPU:

1. the bounds of tests/norm_twin.py can be met: an fp32 emulation of the specified arithmetic (strictly sequential sums; and
   torch's own fp32 layer_norm followed by one rounding) stays under every bound against the float64 twin, for N = 67,
   D in {8, 72, 256, 1024, 2048}, the three dtypes, inputs randn and randn + 3, with and without dropout;
2. the twin's gradients agree with torch.autograd on a float64 composition to 1e-12 relative;
3. the keep masks are functions of (seed, row, col, which, p) with the right kept fraction;
4. the Python surface: exported names, the reference's signatures, error codes of the C ABI, refusals."""
import inspect

import pytest
import torch
import torch.nn.functional as F

import norm_twin as T

N_ROWS = 67
DIMS = (8, 72, 256, 1024, 2048)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
EPS = 1e-5


def _inputs(D, dtype, shift, concat_ux):
    g = torch.Generator().manual_seed(1000 + D)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    x = (r(N_ROWS, D) + shift).to(dtype)
    u = (r(N_ROWS, D) + shift).to(dtype)
    w, b = (1 + 0.1 * r(D)).to(dtype), (0.1 * r(D)).to(dtype)
    dy = r(N_ROWS, 3 * D if concat_ux else D).to(dtype)
    acc = r(N_ROWS, D).to(dtype)
    return x, u, w, b, dy, acc


def _seq_sum(t, dim):
    """fp32 sum along `dim` in index order, one addition at a time"""
    acc = torch.zeros_like(t.select(dim, 0))
    for j in range(t.size(dim)):
        acc = acc + t.select(dim, j)
    return acc


def _emulate(x, u, w, b, dy, acc, p, seed, concat_ux, mul):
    """the arithmetic of include/recsys_amd.h in fp32 torch statements with sequential sums; values before the final rounding"""
    f = lambda t: t.float()   # noqa: E731
    X, W, B, G = f(x), f(w), f(b), f(dy)
    n, D = X.shape
    fD = torch.tensor(float(D))
    mean = _seq_sum(X, 1) / fD
    var = _seq_sum((X - mean[:, None]) ** 2, 1) / fD
    rstd = 1.0 / torch.sqrt(var + torch.tensor(EPS))
    xh = (X - mean[:, None]) * rstd[:, None]
    ln = xh * W + B
    out = SimpleOut(mean=mean, rstd=rstd, y=ln)
    if mul:
        U = f(u)
        den = torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)
        if p > 0:
            k = [T.keep_mask(seed, n, D, i, p) for i in ((0, 1, 2) if concat_ux else (0, 0, 0))]
            drop = lambda v, i: torch.where(k[i], v / den, torch.zeros(()))   # noqa: E731
        else:
            drop = lambda v, i: v   # noqa: E731
        t = ln * U
        if concat_ux:
            out.out = torch.cat([drop(U, 0), drop(X, 1), drop(t, 2)], 1)
            dt, du_extra, extra = drop(G[:, 2 * D:], 2), drop(G[:, :D], 0), drop(G[:, D:2 * D], 1)
        else:
            out.out = drop(t, 2)
            dt, du_extra, extra = drop(G, 2), torch.zeros_like(X), torch.zeros_like(X)
        out.du = dt * ln + du_extra
        gp = dt * U
    else:
        gp, extra = G, f(acc)
    g = W * gp
    c1, c2 = _seq_sum(xh * g, 1) / fD, _seq_sum(g, 1) / fD
    out.dx = (g - (xh * c1[:, None] + c2[:, None])) * rstd[:, None] + extra
    out.dw, out.db = _seq_sum(gp * xh, 0), _seq_sum(gp, 0)
    return out


class SimpleOut:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _check(name, got, ref, bound, log):
    ratio = T.worst(got, ref, bound)
    log.append(f"{name} {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: worst |err| / bound = {ratio}"


@pytest.mark.parametrize("shift", [0.0, 3.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", DIMS)
def test_fp32_emulation_with_sequential_sums_meets_every_bound(D, dtype, shift):
    log = []
    x, u, w, b, dy, acc = _inputs(D, dtype, shift, False)
    # layer norm, dx_accumulate given
    e = _emulate(x, u, w, b, dy, acc, 0.0, 0, False, False)
    fw, bw = T.layer_norm_fwd(x, w, b, EPS), T.layer_norm_bwd(dy, x, w, EPS, dx_accumulate=acc)
    _check("mean", e.mean, fw.mean, T.bound_mean(fw), log)
    _check("rstd", e.rstd, fw.rstd, T.bound_rstd(fw), log)
    _check("y", e.y.to(dtype), fw.y, T.bound_y(fw, dtype), log)
    _check("dx", e.dx.to(dtype), bw.dx, T.bound_dx(bw, dtype), log)
    _check("dw", e.dw.to(dtype), bw.dw, T.bound_dw(bw, dtype), log)
    _check("db", e.db.to(dtype), bw.db, T.bound_db(bw, dtype), log)
    # layer norm mul dropout: no dropout; dropout with the three parts
    for p, concat_ux in ((0.0, False), (0.3, True)):
        x, u, w, b, dy, acc = _inputs(D, dtype, shift, concat_ux)
        e = _emulate(x, u, w, b, dy, acc, p, 77, concat_ux, True)
        tw = T.ln_mul_dropout_bwd(dy, x, u, w, b, EPS, p, True, concat_ux, 77)
        got = e.out.to(dtype)
        assert bool((got[~tw.kept] == 0).all())
        _check(f"out p={p}", got, tw.out, T.bound_out(tw, dtype, concat_ux), log)
        _check(f"du p={p}", e.du.to(dtype), tw.du, T.bound_du(tw, dtype), log)
        _check(f"dx p={p}", e.dx.to(dtype), tw.dx, T.bound_dx(tw, dtype), log)
        _check(f"dw p={p}", e.dw.to(dtype), tw.dw, T.bound_dw(tw, dtype), log)
        _check(f"db p={p}", e.db.to(dtype), tw.db, T.bound_db(tw, dtype), log)
    print(f"D={D} {dtype} shift={shift}: worst |err| / bound: " + ", ".join(log))


@pytest.mark.parametrize("shift", [0.0, 3.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", DIMS)
def test_torch_fp32_layer_norm_and_one_rounding_meets_the_forward_bounds(D, dtype, shift):
    x, u, w, b, _, _ = _inputs(D, dtype, shift, False)
    ln = F.layer_norm(x.float(), (D,), w.float(), b.float(), EPS)
    fw = T.layer_norm_fwd(x, w, b, EPS)
    assert T.worst(ln.to(dtype), fw.y, T.bound_y(fw, dtype)) <= 1.0
    tw = T.ln_mul_dropout_fwd(x, u, w, b, EPS, 0.0, False)
    assert T.worst((ln * u.float()).to(dtype), tw.out, T.bound_out(tw, dtype)) <= 1.0


@pytest.mark.parametrize("concat_ux", [False, True])
def test_twin_gradients_agree_with_autograd(concat_ux):
    n, D, p, seed = 13, 24, 0.3, 5
    g = torch.Generator().manual_seed(3)
    x, u, w, b = (torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True) for s in ((n, D), (n, D), (D,), (D,)))
    dy = torch.randn(n, 3 * D if concat_ux else D, generator=g, dtype=torch.float64)
    f = [T.keep_mask(seed, n, D, i, p).double() / (1 - p) for i in range(3)]
    t = F.layer_norm(x, (D,), w, b, float(torch.tensor(EPS, dtype=torch.float32))) * u
    y = torch.cat([u * f[0], x * f[1], t * f[2]], 1) if concat_ux else t * f[0]
    want = torch.autograd.grad(y, (x, u, w, b), dy)
    tw = T.ln_mul_dropout_bwd(dy, x, u, w, b, EPS, p, True, concat_ux, seed)
    assert torch.allclose(tw.out, y.detach(), rtol=1e-12, atol=0)
    for got, ref in zip((tw.dx, tw.du, tw.dw, tw.db), want):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # the plain layer norm with dx_accumulate
    acc = torch.randn(n, D, generator=g, dtype=torch.float64)
    ln = F.layer_norm(x, (D,), w, b, float(torch.tensor(EPS, dtype=torch.float32)))
    want = torch.autograd.grad(ln, (x, w, b), dy[:, :D])
    bw = T.layer_norm_bwd(dy[:, :D], x, w, EPS, dx_accumulate=acc)
    for got, ref in zip((bw.dx - acc, bw.dw, bw.db), want):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_mask_is_a_function_of_seed_row_col_which_p():
    a = T.keep_mask(11, 40, 72, 0, 0.3)
    assert torch.equal(a, T.keep_mask(11, 40, 72, 0, 0.3))
    assert not torch.equal(a, T.keep_mask(12, 40, 72, 0, 0.3))
    assert not torch.equal(a, T.keep_mask(11 + (1 << 32), 40, 72, 0, 0.3))   # the high word of the seed counts
    assert not torch.equal(a, T.keep_mask(11, 40, 72, 1, 0.3))
    assert not torch.equal(T.keep_mask(11, 40, 72, 1, 0.3), T.keep_mask(11, 40, 72, 2, 0.3))
    # a row keeps its mask when N grows, a column when D grows
    assert torch.equal(a, T.keep_mask(11, 90, 72, 0, 0.3)[:40])
    assert torch.equal(a[:, :30], T.keep_mask(11, 40, 30, 0, 0.3))
    assert torch.equal(a[7:], T.keep_mask(11, 33, 72, 0, 0.3, row0=7))
    # a larger p drops a superset; p = 0 keeps everything
    assert bool((T.keep_mask(11, 40, 72, 0, 0.5) <= a).all())
    assert bool(T.keep_mask(11, 40, 72, 0, 0.0).all())


def test_philox_known_answers():
    """the known-answer vectors of Random123 for Philox4x32-10: counter and key all zeros, and all ones"""
    import numpy as np

    z, f = np.zeros(1, dtype=np.uint64), np.full(1, 0xFFFFFFFF, dtype=np.uint64)
    assert [int(v[0]) for v in T.philox4x32(z, z, z, z, z[0], z[0])] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v[0]) for v in T.philox4x32(f, f, f, f, f[0], f[0])] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert [int(v) for v in T.philox_draws(0, 1, 4, 0)[0]] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


@pytest.mark.parametrize("seed", [1, 2 ** 40 + 17, 2 ** 62 - 1])
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_kept_fraction(p, seed):
    n = 261 * 256
    kept = float(T.keep_mask(seed, 261, 256, 0, p).double().mean())
    assert abs(kept - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, kept


# ---- the Python surface ----
SIGNATURES = {
    "triton_weighted_layer_norm_fwd": [("x",), ("weight",), ("bias",), ("eps",), ("mean", None), ("rstd", None)],
    "triton_weighted_layer_norm_bwd": [("dy",), ("x",), ("weight",), ("bias",), ("mean",), ("rstd",), ("learnable",), ("eps",),
                                       ("BLOCK_D",), ("num_warps",), ("dx_accumulate", None), ("wait_event", None)],
    "triton_layer_norm_mul_dropout_fwd": [("x",), ("u",), ("weight",), ("bias",), ("eps",), ("dropout_ratio",), ("training",),
                                          ("concat_ux", False), ("seed", None)],
    "triton_layer_norm_mul_dropout_bwd": [("dy",), ("x",), ("u",), ("weight",), ("bias",), ("mean",), ("rstd",), ("BLOCK_D",),
                                          ("num_warps",), ("eps",), ("training",), ("dropout_ratio",), ("seed", None),
                                          ("concat_ux", False), ("compute_y", False), ("wait_event", None), ("du", None)],
    "triton_layer_norm": [("x",), ("weight",), ("bias",), ("eps",)],
    "triton_norm_mul_dropout": [("x",), ("u",), ("weight",), ("bias",), ("eps",), ("dropout_ratio",), ("training",),
                                ("concat_ux", False), ("group_norm", False), ("num_heads", 1), ("linear_dim", -1), ("seed", None)],
}


def test_signatures_are_the_references():
    import hstu_norm as H

    for name, want in SIGNATURES.items():
        params = inspect.signature(getattr(H, name)).parameters.values()
        got = [(q.name,) if q.default is inspect.Parameter.empty else (q.name, q.default) for q in params]
        assert got == want, name
        assert getattr(H, name[len("triton_"):]) is getattr(H, name)
        assert name in H.__all__ and name[len("triton_"):] in H.__all__


def test_symbols_are_exported_and_bound():
    import mi355_native as N

    lib = N.lib()
    for name in ("mi355_hstu_layer_norm_fwd", "mi355_hstu_layer_norm_bwd", "mi355_hstu_ln_mul_dropout_fwd",
                 "mi355_hstu_ln_mul_dropout_bwd", "mi355_hstu_layer_norm_bwd_workspace_bytes",
                 "mi355_hstu_ln_mul_dropout_bwd_workspace_bytes"):
        assert name in N.exported_symbols()
        assert getattr(lib, name).argtypes == N.signature_of(name)
    assert lib.mi355_hstu_layer_norm_bwd_workspace_bytes(1031, 1024) >= 2 * 1024 * 4
    assert lib.mi355_hstu_ln_mul_dropout_bwd_workspace_bytes(0, 8) >= 0


def test_workspace_bytes_are_the_contract():
    """The sizes callers may allocate by: 2 * blocks * D * 4 with blocks = min(ceil(rows / 4), 512) for D <= 2048 and
    min(rows, 1024) above, at least 1; RMS half of that; the group norm max(fast, general) partial rows plus (c1, c2)."""
    import mi355_native as N

    lib = N.lib()
    want = {(1031, 1024): 2113536, (5, 2056): 82240, (100000, 8): 32768, (100000, 4104): 33619968, (0, 8): 64}
    for (rows, D), nbytes in want.items():
        assert lib.mi355_hstu_layer_norm_bwd_workspace_bytes(rows, D) == nbytes, (rows, D)
        assert lib.mi355_hstu_ln_mul_dropout_bwd_workspace_bytes(rows, D) == nbytes, (rows, D)
        assert lib.mi355_hstu_swish_layer_norm_bwd_workspace_bytes(rows, D) == nbytes, (rows, D)
    assert lib.mi355_hstu_rms_norm_bwd_workspace_bytes(1031, 1024) == 1056768
    # (1031, 4, 64): fast 258 blocks, general 1031 slots: (1031 * 4 * 2 + 1031 * 4 * 2) * 4
    assert lib.mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(1031, 4, 64) == 65984
    # (67, 257, 8), D = 2056: fast 67 blocks, general 67 slots: (67 * 257 * 2 + 67 * 257 * 2) * 4
    assert lib.mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(67, 257, 8) == 275504
    # (100000, 16, 512), D = 8192: the fast layout's rows decide, 1024 blocks against 512 slots: (1024 * 16 * 2 + 100000 * 16 * 2) * 4
    assert lib.mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(100000, 16, 512) == 12931072


def test_bad_arguments_are_error_codes():
    import mi355_native as N

    lib = N.lib()
    BF16, F16, F32 = N.DT_BF16, N.DT_F16, N.DT_F32

    def ln_fwd(D=8, dtype=BF16, wdtype=F32):
        return lib.mi355_hstu_layer_norm_fwd(None, D, 4, D, dtype, None, None, wdtype, EPS, None, D, None, None, 0, None)

    def ln_bwd(D=8, dtype=BF16, wdtype=F32):
        return lib.mi355_hstu_layer_norm_bwd(None, D, None, D, 4, D, dtype, None, wdtype, None, None, None, 0, None, D, None,
                                             None, None, 0, None)

    def mul_fwd(D=8, dtype=BF16, wdtype=F32, H=1, UD=8, p=0.3):
        return lib.mi355_hstu_ln_mul_dropout_fwd(None, D, None, D, UD, H, UD, 4, D, dtype, None, None, wdtype, EPS, p, 1, 5, 0,
                                                 None, D, None, None, None)

    def mul_bwd(D=8, dtype=BF16, wdtype=F32, H=1, UD=8, p=0.3):
        return lib.mi355_hstu_ln_mul_dropout_bwd(None, D, None, D, None, D, UD, H, UD, 4, D, dtype, None, None, wdtype, None,
                                                 None, p, 1, 5, 0, None, D, None, D, UD, None, None, None, 0, None, 0, None)

    for call in (ln_fwd, ln_bwd, mul_fwd, mul_bwd):
        for kw, text in (({"D": 8193}, b"D must be in 1 .. 8192"), ({"D": 0}, b"D must be in 1 .. 8192"),
                         ({"dtype": 7}, b"unsupported dtype"), ({"dtype": BF16, "wdtype": F16}, b"fp32 or have the dtype of the rows")):
            assert call(**kw) == -1 and text in lib.mi355_last_error(), (call.__name__, kw)
    for call in (mul_fwd, mul_bwd):
        assert call(H=2, UD=3) == -1 and b"H * UD == D" in lib.mi355_last_error()
        for p in (1.0, -0.1, 1.5):
            assert call(p=p) == -1 and b"dropout_ratio must be in [0, 1)" in lib.mi355_last_error()
    # and with every argument in range the null buffers are the error
    assert ln_fwd() == -1 and b"null buffer" in lib.mi355_last_error()


def test_cpu_tensors_and_group_norm_are_refused():
    import hstu_norm as H
    import mi355_native as N

    x, u, w, b = torch.randn(4, 8), torch.randn(4, 8), torch.ones(8), torch.zeros(8)
    with pytest.raises(N.NativeError):
        H.triton_weighted_layer_norm_fwd(x, w, b, EPS)
    with pytest.raises(N.NativeError):
        H.triton_layer_norm_mul_dropout_fwd(x, u, w, b, EPS, 0.0, False)
    with pytest.raises(N.NativeError):
        H.triton_layer_norm(x, w, b, EPS)
    with pytest.raises(N.NativeError):
        H.triton_weighted_layer_norm_bwd(x, x, w, b, torch.zeros(4), torch.ones(4), True, EPS, 8, 1)
    with pytest.raises(N.NativeError):
        H.triton_layer_norm_mul_dropout_bwd(x, x, u, w, b, torch.zeros(4), torch.ones(4), 8, 1, EPS, False, 0.0)
    with pytest.raises(NotImplementedError):
        H.triton_norm_mul_dropout(x, u, w, b, EPS, 0.0, False, group_norm=True)
    # the launch parameters the reference returns
    assert H._launch_params(1024, 2) == (1024, 4) and H._launch_params(72, 4) == (128, 1) and H._launch_params(8192, 2) == (8192, 8)
