"""CPU checks of the HSTU activation kernels (hstu_addmm over csrc/act_ops.hip) that need no GPU:

1. the bounds of tests/act_twin.py can be met: an fp32 numpy emulation of the stated arithmetic stays under every bound against
   the float64 twin, for random data and for the edge list 0, +-2^-126, +-1, -1.2785, +-20, +-89, +-1e4, +-max-finite of each
   dtype (every edge z against every edge g);
2. they are not loose: one extra bf16 rounding of sig breaks the dz bound, a column sum that drops one row the dbias bound;
3. the Python shims refuse CPU tensors;
4. the C ABI answers -1 with a message for an unknown dtype, a bad stride and a short workspace."""
import pytest
import torch

import act_twin as T

DTYPES = (torch.bfloat16, torch.float16, torch.float32)
ROWS, WIDTH = 67, 72


def _random(dtype, scale=1.0):
    g = torch.Generator().manual_seed(4242)
    z = (scale * torch.randn(ROWS, WIDTH, generator=g)).to(dtype)
    go = torch.randn(ROWS, WIDTH, generator=g).to(dtype)
    return go, z


def _edges(dtype):
    """[n, n]: row i holds g = edge i against every edge z"""
    e = T.edge_values(dtype)
    return e[:, None].expand(len(e), len(e)).contiguous(), e[None, :].expand(len(e), len(e)).contiguous()


def _check(name, got, ref, bound):
    ratio = T.worst(got, ref, bound)
    print(f"{name}: worst |err| / bound = {ratio:.3f}")
    return ratio


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("data", ["random", "random x 8", "edges", "edge z, random g"])
def test_emulation_meets_every_bound(dtype, data):
    go, z = _edges(dtype) if data == "edges" else _random(dtype, 8.0 if data == "random x 8" else 1.0)
    if data == "edge z, random g":
        e = T.edge_values(dtype)
        go, z = go[:, :len(e)].contiguous(), e[None, :].expand(ROWS, len(e)).contiguous()
    fw = T.silu_fwd(z)
    s = T.emulate_silu_fwd(z, dtype)
    assert bool(torch.isfinite(s.float()).all())
    assert _check(f"s {dtype} {data}", s, fw.s, T.bound_s(fw, dtype)) <= 1.0
    bw = T.silu_bwd(go, z)
    for bdtype in (torch.float32, dtype):
        dz, dbias = T.emulate_silu_bwd(go, z, dtype, bdtype)
        assert bool(torch.isfinite(dz.float()).all())
        assert _check(f"dz {dtype} {data}", dz, bw.dz, T.bound_dz(bw, dtype)) <= 1.0
        if data != "edges":   # (a column of the edge table sums +-max-finite: its float64 sum is not the dtype's to hold)
            assert _check(f"dbias {dtype}->{bdtype} {data}", dbias, bw.dbias, T.bound_dbias(bw, bdtype)) <= 1.0


def test_edge_values_are_what_the_dtype_holds():
    for dtype in DTYPES:
        e = T.edge_values(dtype)
        assert bool(torch.isfinite(e.float()).all()) and float(e[-2]) == T.max_finite(dtype) and float(e[-1]) == -T.max_finite(dtype)
        assert float(e[0]) == 0.0 and float(e[3]) == 1.0
    assert float(T.edge_values(torch.float32)[1]) == 2.0 ** -126 and float(T.edge_values(torch.bfloat16)[1]) == 2.0 ** -126


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_bounds_are_not_loose(dtype):
    go, z = _random(dtype)
    bw = T.silu_bwd(go, z)
    dz, dbias = T.emulate_silu_bwd(go, z, dtype, torch.float32, sig_rounding=torch.bfloat16)
    assert _check(f"dz with sig rounded to bf16, {dtype}", dz, bw.dz, T.bound_dz(bw, dtype)) > 1.0
    dz, dbias = T.emulate_silu_bwd(go, z, dtype, torch.float32, drop_row=ROWS // 2)
    assert _check(f"dz, {dtype}", dz, bw.dz, T.bound_dz(bw, dtype)) <= 1.0
    assert _check(f"dbias without one row, {dtype}", dbias, bw.dbias, T.bound_dbias(bw, torch.float32)) > 1.0


def test_shims_refuse_cpu_tensors():
    import hstu_addmm as A
    import mi355_native as N

    x, w, b = torch.randn(5, 8), torch.randn(8, 16), torch.randn(16)
    z, go = torch.randn(5, 16), torch.randn(5, 16)
    for call in (lambda: A.triton_addmm_silu_fwd(x, w, b, True), lambda: A.torch_addmm_silu_fwd(x, w, b),
                 lambda: A.triton_addmm_silu_bwd(x, w, z, go, True, True), lambda: A.triton_addmm(b, x, w, True),
                 lambda: A.triton_silu_fwd(z), lambda: A.triton_silu_bwd(go, z), lambda: A.triton_silu(z)):
        with pytest.raises(N.NativeError):
            call()
    assert A.torch_addmm_silu_fwd is A.triton_addmm_silu_fwd


def test_entry_points_answer_bad_arguments_with_error_codes():
    import mi355_native as N

    lib = N.lib()
    assert lib.mi355_hstu_silu_fwd(None, 8, 4, 8, 7, None, 8, None) == -1 and b"dtype" in lib.mi355_last_error()
    assert lib.mi355_hstu_silu_bwd(None, 8, None, 8, 4, 8, 7, None, 8, None, 0, None, 0, None) == -1
    assert b"dtype" in lib.mi355_last_error()
    assert lib.mi355_hstu_silu_fwd(None, 0, 4, 8, N.DT_BF16, None, 8, None) == -1 and b"stride" in lib.mi355_last_error()
    assert lib.mi355_hstu_silu_bwd(None, 8, None, -8, 4, 8, N.DT_BF16, None, 8, None, 0, None, 0, None) == -1
    assert b"stride" in lib.mi355_last_error()
    # a dbias without enough workspace (the pointers are never followed: the checks come first)
    need = lib.mi355_hstu_silu_bwd_workspace_bytes(67, 72)
    fake = 1 << 20
    assert lib.mi355_hstu_silu_bwd(fake, 72, fake, 72, 67, 72, N.DT_BF16, fake, 72, fake, N.DT_F32, fake, need - 1, None) == -1
    assert b"workspace" in lib.mi355_last_error()
    assert lib.mi355_hstu_silu_bwd(fake, 72, fake, 72, 67, 72, N.DT_BF16, fake, 72, fake, N.DT_F16, fake, need, None) == -1
    assert b"dbias" in lib.mi355_last_error()
    # rows == 0 without a dbias and N == 0 are no-ops that touch no device
    assert lib.mi355_hstu_silu_fwd(None, 8, 0, 8, N.DT_F32, None, 8, None) == 0
    assert lib.mi355_hstu_silu_fwd(None, 0, 5, 0, N.DT_F32, None, 0, None) == 0
    assert lib.mi355_hstu_silu_bwd(None, 8, None, 8, 0, 8, N.DT_F16, None, 8, None, 0, None, 0, None) == 0


def test_workspace_bytes_positive_and_monotone_in_rows():
    import mi355_native as N

    lib = N.lib()
    for n in (8, 72, 1024, 2050, 4096):
        sizes = [lib.mi355_hstu_silu_bwd_workspace_bytes(r, n) for r in (0, 1, 5, 67, 1031, 8197, 1 << 20)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (n, sizes)
        assert sizes[-1] >= 64 * n * 4
