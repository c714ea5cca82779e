"""GPU checks of the HSTU activation kernels (csrc/act_ops.hip behind hstu_addmm) against the float64 twin of
tests/act_twin.py, element by element under the bounds stated there; every comparison prints its worst |err| / bound.

Rows: {0, 1, 5, 67, 1031}: the empty call, fewer rows than a block's four waves, no multiple of a wave or block count.
Widths: {8, 72, 256, 1024} at every row count; 2050 (no multiple of 8 or 4: the element-wise path, 33 column chunks) with rows
{5, 67}.  The grid is resident: a capped number of row groups of four rows each strides over the rows, a thread holding
ROWS_IN_FLIGHT rows of its column piece per trip of its row loop.  The cap is read from the workspace size (one fp32 row per row
group), and two row counts are derived from it at N = 8, bf16 only: five rows more than the groups hold (a thread's second row,
still inside its first trip) and five more than one trip of every thread holds (a second trip).  Both have the workspace at its
maximum of rows.
Dtypes bf16 / fp16 / fp32, dbias in fp32 and in the row dtype, contiguous and as a column slice of a sentinel-filled buffer:
from column 8 with row stride N + 8 (16-byte pieces stay possible), and at N = 72 from column 1 with row stride N + 1, where
the base pointers and the strides, not N, force the element-wise path."""
import itertools

import pytest
import torch

import act_twin as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
SHAPES = [(r, n) for n in (8, 72, 256, 1024) for r in (0, 1, 5, 67, 1031)] + [(5, 2050), (67, 2050)]
CASES = [(r, n, t) for (r, n) in SHAPES for t in DTYPES]
ROWS_IN_FLIGHT = 4   # kActRowsInFlight of csrc/act_ops.hip
SENTINEL = 7.0


def _A():
    import hstu_addmm as A

    return A


def _cmp(name, got, ref, bound):
    ratio = T.worst(got, ref, bound)
    print(f"{name}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: worst |err| / bound = {ratio}"


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _slice_of(t, lead):
    """(buffer, view): t's values as the column slice from `lead` on, row stride N + lead, of a buffer filled with the sentinel"""
    buf = torch.full((t.size(0), t.size(1) + lead), SENTINEL, dtype=t.dtype, device=DEV)
    view = buf[:, lead:]
    view.copy_(t)
    return buf, view


def _untouched(buf, lead):
    return bool((buf[:, :lead] == SENTINEL).all())


def _silu_fwd(z, s):
    import mi355_native as N

    stride = lambda t: t.stride(0) if t.size(0) > 1 else t.size(1)   # noqa: E731
    N.check(N.lib().mi355_hstu_silu_fwd(N.ptr(z), stride(z), z.size(0), z.size(1), N.dt(z), N.ptr(s), stride(s), N.stream()))
    return s


def _row_groups(rows, n):
    """row groups of the resident grid for (rows, n): the workspace holds one fp32 row of n columns for each"""
    import mi355_native as N

    nbytes = int(N.lib().mi355_hstu_silu_bwd_workspace_bytes(rows, n))
    assert nbytes % (4 * n) == 0
    return nbytes // (4 * n)


@pytest.mark.parametrize("rows,n,dtype", CASES)
def test_silu_forward_and_backward(rows, n, dtype):
    _check_shape(rows, n, dtype, lead=8)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_slice_takes_the_elementwise_path(dtype):
    """N = 72 allows 16-byte pieces; a slice from column 1 with row stride 73 does not: neither its base nor its stride is a
    multiple of 16 bytes.  The contiguous calls of the same check run the vector kernel; the strided ones are held to the same bounds."""
    _check_shape(67, 72, dtype, lead=1, other_kernel=True)


@pytest.mark.parametrize("trips", [1, 2])
def test_more_rows_than_the_resident_grid_holds(trips):
    """trips 1: five rows more than the capped grid has row groups of four, so five threads per column piece take a second row
    inside the first trip of their row loop.  trips 2: five rows more than one trip of every thread covers, so the loop makes a
    second trip.  The cap is the kernel's own, read from the workspace size."""
    n = 8
    cap = _row_groups(1 << 30, n)
    rows = cap * 4 * (ROWS_IN_FLIGHT if trips == 2 else 1) + 5
    assert _row_groups(rows, n) == cap and _row_groups(rows - 5, n) == cap and _row_groups(4 * cap - 4, n) == cap - 1
    print(f"row groups capped at {cap}: {rows} rows")
    _check_shape(rows, n, torch.bfloat16, lead=8)


def _check_shape(rows, n, dtype, lead, other_kernel=False):
    """other_kernel: the strided calls run another instantiation (V = 1) than the contiguous ones (V = 16 bytes' worth).  The
    compiler is free to contract a multiply and an add into one fma differently in the two, so their fp32 values may differ in
    the last bit: the strided results are then held to the twin's bounds, and the in-place results to the strided ones' bits."""
    A = _A()
    z = (2.0 * torch.randn(rows, n)).to(dtype).to(DEV)
    g = torch.randn(rows, n).to(dtype).to(DEV)
    fw, bw = T.silu_fwd(z), T.silu_bwd(g, z)
    tag = f"rows={rows} n={n} {dtype}"
    # forward: contiguous, strided, in place
    s = A.triton_silu_fwd(z)
    assert s.shape == z.shape and s.dtype == dtype
    _cmp(tag + " s", s, fw.s, T.bound_s(fw, dtype))
    zbuf, zs = _slice_of(z, lead)
    sbuf, ss = _slice_of(torch.zeros_like(z), lead)
    _silu_fwd(zs, ss)
    if other_kernel:   # under the twin's bound, and from here on the reference for the in-place call
        _cmp(tag + " s, strided", ss.contiguous(), fw.s, T.bound_s(fw, dtype))
        s = ss.contiguous()
    assert _same(ss.contiguous(), s) and _untouched(sbuf, lead) and _untouched(zbuf, lead), tag + ": strided forward"
    _silu_fwd(zs, zs)
    assert _same(zs.contiguous(), s) and _untouched(zbuf, lead), tag + ": in-place forward"
    # backward: dbias in fp32 and in the row dtype; twice; strided; in place; without dbias
    for bdtype in (torch.float32, dtype):
        runs = [A.silu_bwd_dbias(g, z, dbias_dtype=bdtype) for _ in range(2)]
        dz, dbias = runs[0]
        assert _same(dz, runs[1][0]) and _same(dbias, runs[1][1]), tag + ": the backward is not reproducible"
        assert dz.shape == z.shape and dz.dtype == dtype and dbias.shape == (n,) and dbias.dtype == bdtype
        _cmp(tag + " dz", dz, bw.dz, T.bound_dz(bw, dtype))
        _cmp(tag + f" dbias {bdtype}", dbias, bw.dbias, T.bound_dbias(bw, bdtype))
        if rows == 0:
            assert bool((dbias == 0).all())
    dz_none, none = A.silu_bwd_dbias(g, z, with_dbias=False)
    assert none is None and _same(dz_none, dz), tag + ": dz depends on dbias"
    assert _same(A.triton_silu_bwd(g, z), dz)
    gbuf, gs = _slice_of(g, lead)
    zbuf, zs = _slice_of(z, lead)
    obuf, os_ = _slice_of(torch.zeros_like(z), lead)
    dz_s, dbias_s = A.silu_bwd_dbias(gs, zs, dz_out=os_, dbias_dtype=dtype)
    if other_kernel:
        _cmp(tag + " dz, strided", os_.contiguous(), bw.dz, T.bound_dz(bw, dtype))
        _cmp(tag + " dbias, strided", dbias_s, bw.dbias, T.bound_dbias(bw, dtype))
        dz, dbias = os_.contiguous(), dbias_s.clone()
    assert dz_s is os_ and _same(os_.contiguous(), dz) and _same(dbias_s, dbias), tag + ": strided backward"
    assert _untouched(obuf, lead) and _untouched(gbuf, lead) and _untouched(zbuf, lead)
    dz_i, dbias_i = A.silu_bwd_dbias(gs, zs, dz_out=gs, dbias_dtype=dtype)
    assert dz_i is gs and _same(gs.contiguous(), dz) and _same(dbias_i, dbias) and _untouched(gbuf, lead), tag + ": in-place backward"


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_values_give_finite_outputs_within_bounds(dtype):
    A = _A()
    e = T.edge_values(dtype)
    n = len(e)
    g = e[:, None].expand(n, n).contiguous().to(DEV)
    z = e[None, :].expand(n, n).contiguous().to(DEV)
    fw, bw = T.silu_fwd(z), T.silu_bwd(g, z)
    s = A.triton_silu_fwd(z)
    dz = A.triton_silu_bwd(g, z)
    assert bool(torch.isfinite(s.float()).all()) and bool(torch.isfinite(dz.float()).all())
    _cmp(f"edges {dtype} s", s, fw.s, T.bound_s(fw, dtype))
    _cmp(f"edges {dtype} dz", dz, bw.dz, T.bound_dz(bw, dtype))
    # NaN goes through
    z[0, 0] = float("nan")
    assert bool(torch.isnan(A.triton_silu_fwd(z)[0, 0])) and bool(torch.isnan(A.triton_silu_bwd(g, z)[0, 0]))
    # random gradients over the edge columns: the column sums as well
    g = torch.randn(67, n).to(dtype).to(DEV)
    z = e[None, :].expand(67, n).contiguous().to(DEV)
    bw = T.silu_bwd(g, z)
    dz, dbias = A.silu_bwd_dbias(g, z, dbias_dtype=torch.float32)
    _cmp(f"edge columns {dtype} dz", dz, bw.dz, T.bound_dz(bw, dtype))
    _cmp(f"edge columns {dtype} dbias", dbias, bw.dbias, T.bound_dbias(bw, torch.float32))


# ---- hstu_addmm against float64 ----
M, K, NN = 67, 40, 72


def _gemm_inputs(dtype, y_2d):
    x = torch.randn(M, K).to(dtype).to(DEV)
    w = (torch.randn(K, NN) / K ** 0.5).to(dtype).to(DEV)
    y = torch.randn(M, NN).to(dtype).to(DEV) if y_2d else torch.randn(NN).to(dtype).to(DEV)
    return x, w, y


def _z64(x, w, y):
    return y.cpu().double() + x.cpu().double() @ w.cpu().double()


def _gemm_bound(x, w, y, dtype):
    """u |z| for the rounding of the result and u |x w| for one of the product before the addend joins it (torch.addmm does not
    promise a single rounding), plus the fp32 accumulation of K products in any order"""
    xw = x.cpu().double() @ w.cpu().double()
    mag = y.cpu().double().abs() + x.cpu().double().abs() @ w.cpu().double().abs()
    return T.unit_roundoff(dtype) * (_z64(x, w, y).abs() + xw.abs()) + (K + 2) * T.H32 * mag + T.sub(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_addmm_silu_fwd_tuples_and_aliasing(dtype):
    A = _A()
    for y_2d in (False, True):
        x, w, y = _gemm_inputs(dtype, y_2d)
        z_ref, _ = A.triton_addmm_silu_fwd(x, w, y)
        _cmp(f"addmm z {dtype} y_2d={y_2d}", z_ref, _z64(x, w, y), _gemm_bound(x, w, y, dtype))
        fw = T.silu_fwd(z_ref)
        for silu, keep, give_out, give_silu_out in itertools.product((False, True), repeat=4):
            for fn in (A.triton_addmm_silu_fwd, A.torch_addmm_silu_fwd):
                out = torch.empty(M, NN, dtype=dtype, device=DEV) if give_out else None
                silu_out = torch.empty(M, NN, dtype=dtype, device=DEV) if give_silu_out else None
                z, sz = fn(x, w, y, silu, keep, out, silu_out)
                tag = f"silu={silu} keep={keep} out={give_out} silu_out={give_silu_out}"
                if give_out:
                    assert z is out, tag
                if silu and give_silu_out:
                    assert sz is silu_out, tag
                assert (sz is None) == (not silu), tag
                if not silu:
                    assert _same(z, z_ref), tag
                    continue
                _cmp(f"addmm silu {dtype} {tag}", sz, fw.s, T.bound_s(fw, dtype))
                separate = keep or (give_out and give_silu_out)
                if separate:
                    assert z.data_ptr() != sz.data_ptr() and _same(z, z_ref), tag
                else:
                    assert z.data_ptr() == sz.data_ptr(), tag   # (one buffer: the SiLU ran in place)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("y_2d", [False, True])
def test_addmm_silu_bwd(dtype, y_2d):
    A = _A()
    x, w, y = _gemm_inputs(dtype, y_2d)
    go = torch.randn(M, NN).to(dtype).to(DEV)
    z, _ = A.triton_addmm_silu_fwd(x, w, y, True)
    dx, dw, dy = A.triton_addmm_silu_bwd(x, w, z, go, not y_2d, True)
    bw = T.silu_bwd(go, z)
    dz, dbias = A.silu_bwd_dbias(go, z)
    if y_2d:
        assert _same(dy, dz)
    else:
        assert _same(dy, dbias)
        _cmp(f"addmm bwd dy {dtype}", dy, bw.dbias, T.bound_dbias(bw, dtype))
    _cmp(f"addmm bwd dz {dtype}", dz, bw.dz, T.bound_dz(bw, dtype))
    # the GEMMs against float64 at the dz the kernel produced
    d64, u = dz.cpu().double(), T.unit_roundoff(dtype)
    dx64, dw64 = d64 @ w.cpu().double().t(), x.cpu().double().t() @ d64
    _cmp(f"addmm bwd dx {dtype}", dx, dx64, u * dx64.abs() + (NN + 2) * T.H32 * (d64.abs() @ w.cpu().double().abs().t()) + T.sub(dtype))
    _cmp(f"addmm bwd dw {dtype}", dw, dw64, u * dw64.abs() + (M + 2) * T.H32 * (x.cpu().double().abs().t() @ d64.abs()) + T.sub(dtype))
    # silu=False: dz is grad_output; dz_out in place leaves the results as they are
    dx0, dw0, dy0 = A.triton_addmm_silu_bwd(x, w, None, go, not y_2d)
    assert _same(dx0, torch.mm(go, w.t())) and _same(dw0, torch.mm(x.t(), go))
    assert dy0 is go if y_2d else _same(dy0, go.sum(0))
    g2 = go.clone()
    dx2, dw2, dy2 = A.triton_addmm_silu_bwd(x, w, z, g2, not y_2d, True, dz_out=g2)
    assert _same(g2, dz) and _same(dx2, dx) and _same(dw2, dw) and _same(dy2, dy)
    # side stream: the same bits once the event has passed
    stream, event = torch.cuda.Stream(), torch.cuda.Event()
    dx3, dw3, dy3 = A.triton_addmm_silu_bwd(x, w, z, go, not y_2d, True, stream, event)
    event.synchronize()
    torch.cuda.synchronize()
    assert _same(dx3, dx) and _same(dw3, dw) and _same(dy3, dy)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_autograd_wrappers_equal_the_raw_calls(dtype):
    A = _A()
    x, w, y = (t.requires_grad_(True) for t in _gemm_inputs(dtype, False))
    go = torch.randn(M, NN).to(dtype).to(DEV)
    for silu in (False, True):
        out = A.triton_addmm(y, x, w, silu)
        got = torch.autograd.grad(out, (x, w, y), go)
        z, sz = A.triton_addmm_silu_fwd(x.detach(), w.detach(), y.detach(), silu)
        want = A.triton_addmm_silu_bwd(x.detach(), w.detach(), z, go, True, silu)
        assert _same(out.detach(), sz if silu else z) and all(_same(p, q) for p, q in zip(got, want))
    t = torch.randn(5, 3, 72).to(dtype).to(DEV).requires_grad_(True)
    g3 = torch.randn(5, 3, 72).to(dtype).to(DEV)
    s = A.triton_silu(t)
    (gt,) = torch.autograd.grad(s, (t,), g3)
    assert s.shape == t.shape and _same(s.detach(), A.triton_silu_fwd(t.detach())) and _same(gt, A.triton_silu_bwd(g3, t.detach()))
    bw = T.silu_bwd(g3.view(15, 72), t.view(15, 72))
    _cmp(f"triton_silu grad {dtype}", gt.view(15, 72), bw.dz, T.bound_dz(bw, dtype))
