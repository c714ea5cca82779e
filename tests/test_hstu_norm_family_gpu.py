"""GPU checks of the HSTU norm family (csrc/group_norm_ops.hip and csrc/norm_family_ops.hip behind hstu_norm) against the
float64 twin of tests/norm_family_twin.py, element by element under the bounds stated there; every comparison prints its worst
|err| / bound.  Exact checks: dropout zeros and masks, reproducibility, compute_y, the du sentinel, head isolation, autograd.

Swish and RMS take the shapes of test_hstu_norm_gpu.py (the kernels share its decomposition): D in {8, 72, 256, 1024} with
N in {0, 1, 5, 67, 1031}, one D past each boundary (520, 1032, 2050, 2056, 4104) with N in {5, 67}, and the two loop shapes
8197 x 8 and 2051 x 2056 in bf16 (a wave, a workgroup walks more than one row; 8 MB, the largest case).
Group norm, (H, L):
  (1, 8), (4, 2)       general layout, one element an access; (1, 8) has the masks of the layer norm
  (6, 12)              nothing a power of two
  (4, 64), (8, 128)    the fast layout: lane groups of 8 / 16 (bf16, fp16), 16 / 32 (fp32)
  (3, 344)             D = 1032: heads that straddle lanes unevenly
  (8, 257), (257, 8)   D = 2056: many heads, odd head length; (257, 8) is fast in bf16 / fp16 (one piece a head, workgroup rows)
  (2, 2052)            D = 4104: a head longer than a wave's reach
  8197 x (2, 4) and 2051 x (8, 257) in bf16: more (row, head) pairs than lane groups."""
import pytest
import torch

import norm_family_twin as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
SHAPES = [(n, d) for d in (8, 72, 256, 1024) for n in (0, 1, 5, 67, 1031)] + \
         [(n, d) for d in (520, 1032, 2050, 2056, 4104) for n in (5, 67)]
ROW_CASES = [(n, d, t) for (n, d) in SHAPES for t in DTYPES] + [(n, d, torch.bfloat16) for (n, d) in ((8197, 8), (2051, 2056))]
GN_SHAPES = [(n, h, l) for (h, l) in ((1, 8), (4, 2), (6, 12), (4, 64), (8, 128)) for n in (0, 1, 5, 67, 1031)] + \
            [(n, h, l) for (h, l) in ((3, 344), (8, 257), (257, 8), (2, 2052)) for n in (5, 67)]
GN_CASES = [(n, h, l, t) for (n, h, l) in GN_SHAPES for t in DTYPES] + \
           [(8197, 2, 4, torch.bfloat16), (2051, 8, 257, torch.bfloat16)]
SEED = 0x1234_5678_9ABC


def _H():
    import hstu_norm as H

    return H


def _rand(n, d, dtype, shift=0.0, strided=False):
    """O(1) values; strided: a column slice of a wider tensor (row stride d + 8)"""
    t = (torch.randn(n, d + 8 if strided else d) + shift).to(dtype).to(DEV)
    return t[:, 8:] if strided else t


def _params(d, wdtype):
    return (1 + 0.1 * torch.randn(d)).to(wdtype).to(DEV), (0.1 * torch.randn(d)).to(wdtype).to(DEV)


def _cmp(name, got, ref, bound):
    ratio = F.worst(got, ref, bound)
    print(f"{name}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: worst |err| / bound = {ratio}"


def _same(a, b):
    if a is None or b is None:
        return a is b
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _u_of(n, h, l, dtype, three_d):
    """u as the layer passes it: a column slice of a [n, 4 d] buffer, or [n, H, L] cut from a buffer with a longer head"""
    if not three_d:
        return torch.randn(n, 4 * h * l).to(dtype).to(DEV)[:, h * l:2 * h * l]
    return torch.randn(n, h, l + 8).to(dtype).to(DEV)[:, :, 8:]


def _du_with_sentinel(u):
    """a strided tensor of u's shape inside a buffer filled with 7"""
    if u.dim() == 2:
        buf = torch.full((u.size(0), u.size(1) + 16), 7.0, dtype=u.dtype, device=DEV)
        return buf, buf[:, 8:8 + u.size(1)]
    buf = torch.full((u.size(0), u.size(1), u.size(2) + 16), 7.0, dtype=u.dtype, device=DEV)
    return buf, buf[:, :, 8:8 + u.size(2)]


# ---- 1. swish layer norm and RMS norm ----
@pytest.mark.parametrize("n,d,dtype", ROW_CASES)
def test_swish_layer_norm_fwd_bwd(n, d, dtype):
    H = _H()
    for strided, shift, row_w in ((False, 0.0, False), (True, 1.5, True)):
        tag = f"swish n={n} d={d} {dtype} strided={strided}"
        x, dy = _rand(n, d, dtype, shift, strided), _rand(n, d, dtype, 0.0, strided)
        w, b = _params(d, dtype if row_w else torch.float32)
        y, mean, rstd = H.triton_swish_layer_norm_fwd(x, w, b, EPS)
        assert y.shape == x.shape and y.dtype == dtype and mean.shape == rstd.shape == (n,)
        tw = F.swish_bwd(dy, x, w, b, EPS)
        _cmp(tag + " mean", mean, tw.mean, F.bound_mean(tw))
        _cmp(tag + " rstd", rstd, tw.rstd, F.bound_rstd(tw))
        _cmp(tag + " y", y, tw.y, F.swish_bound_y(tw, dtype))
        runs = [H.triton_swish_layer_norm_bwd(dy, x, w, b, mean, rstd) for _ in range(2)]
        assert all(_same(p, q) for p, q in zip(*runs)), tag + ": the backward is not reproducible"
        dx, dw, db = runs[0]
        assert dx.shape == x.shape and dx.dtype == dtype and dw.dtype == db.dtype == w.dtype and dw.shape == db.shape == (d,)
        _cmp(tag + " dx", dx, tw.dx, F.swish_bound_dx(tw, dtype))
        _cmp(tag + " dw", dw, tw.dw, F.swish_bound_dw(tw, w.dtype))
        _cmp(tag + " db", db, tw.db, F.swish_bound_db(tw, w.dtype))
        if n == 0:
            assert bool((dw == 0).all()) and bool((db == 0).all())


@pytest.mark.parametrize("n,d,dtype", ROW_CASES)
def test_rms_norm_fwd_bwd(n, d, dtype):
    H = _H()
    for strided, shift, row_w in ((False, 0.0, False), (True, 1.5, True)):
        tag = f"rms n={n} d={d} {dtype} strided={strided}"
        x, dy = _rand(n, d, dtype, shift, strided), _rand(n, d, dtype, 0.0, strided)
        w = _params(d, dtype if row_w else torch.float32)[0]
        y, rstd = H.triton_rms_norm_fwd(x, w, EPS)
        assert y.shape == x.shape and y.dtype == dtype and rstd.shape == (n,) and rstd.dtype == torch.float32
        tw = F.rms_bwd(dy, x, w, EPS)
        _cmp(tag + " rstd", rstd, tw.rstd, F.bound_rstd(tw))
        _cmp(tag + " y", y, tw.y, F.rms_bound_y(tw, dtype))
        runs = [H.triton_rms_norm_bwd(dy, x, w, rstd) for _ in range(2)]
        assert all(_same(p, q) for p, q in zip(*runs)), tag + ": the backward is not reproducible"
        dx, dw = runs[0]
        assert dx.shape == x.shape and dx.dtype == dtype and dw.dtype == w.dtype and dw.shape == (d,)
        _cmp(tag + " dx", dx, tw.dx, F.rms_bound_dx(tw, dtype))
        _cmp(tag + " dw", dw, tw.dw, F.rms_bound_dw(tw, w.dtype))
        if n == 0:
            assert bool((dw == 0).all())


# ---- 2. group norm mul dropout ----
@pytest.mark.parametrize("n,h,l,dtype", GN_CASES)
def test_group_norm_mul_dropout(n, h, l, dtype):
    H = _H()
    d = h * l
    # (u 3-D with a head stride, concat_ux, du supplied, weights in the row dtype, x / dy strided, training, p)
    for three_d, concat_ux, own_du, row_w, strided, training, p in ((False, False, False, False, False, False, 0.3),
                                                                    (True, True, True, True, True, True, 0.3),
                                                                    (False, True, True, False, True, True, 0.0)):
        tag = f"gn n={n} h={h} l={l} {dtype} 3d={three_d} concat={concat_ux} training={training} p={p}"
        x, u = _rand(n, d, dtype, 1.5 if strided else 0.0, strided), _u_of(n, h, l, dtype, three_d)
        w, b = _params(h, dtype if row_w else torch.float32)
        dy = _rand(n, 3 * d if concat_ux else d, dtype, 0.0, strided)
        y, mean, rstd, block_d, block_h, num_warps, seed = H.triton_group_norm_mul_dropout_fwd(
            x, u, w, b, EPS, p, training, concat_ux, h, l, SEED)
        assert y.shape == (n, 3 * d if concat_ux else d) and y.dtype == dtype
        assert mean.shape == rstd.shape == (n * h,) and mean.dtype == rstd.dtype == torch.float32
        assert seed == (SEED if n else 0)
        tw = F.gn_mul_dropout_bwd(dy, x, u, w, b, EPS, p, training, concat_ux, h, l, SEED)
        _cmp(tag + " mean", mean, tw.mean, F.gn_bound_mean(tw))
        _cmp(tag + " rstd", rstd, tw.rstd, F.gn_bound_rstd(tw))
        # dropped elements are exactly +0 and the zero pattern is keep_mask over the full row width
        yc = y.cpu()
        assert bool((yc[~tw.kept] == 0).all()) and not bool(torch.signbit(yc[~tw.kept]).any()), tag + ": a dropped element is not +0"
        # (compared where the value before dropout is not zero, in the twin and as the kernel rounds it)
        y_eval = H.triton_group_norm_mul_dropout_fwd(x, u, w, b, EPS, p, False, concat_ux, h, l, SEED)[0]
        nonzero = (tw.undropped != 0) & (y_eval.cpu() != 0)
        assert torch.equal((yc != 0)[nonzero], tw.kept[nonzero]), tag + ": the mask differs from keep_mask"
        _cmp(tag + " y", y, tw.out, F.gn_bound_out(tw, dtype, concat_ux))
        runs = []
        for _ in range(2):
            buf, du_in = _du_with_sentinel(u) if own_du else (None, None)
            out = H.triton_group_norm_mul_dropout_bwd(dy, x, u, w, b, mean, rstd, block_d, block_h, num_warps, EPS, training, p,
                                                      seed, concat_ux, h, l, True, du=du_in)
            if own_du:
                assert out[1] is du_in
                got = out[1].clone()
                du_in.fill_(7.0)
                assert bool((buf == 7.0).all()), tag + ": something outside du was written"
                out = (out[0], got) + out[2:]
            runs.append(out)
        assert all(_same(q, r) for q, r in zip(*runs)), tag + ": the backward is not reproducible"
        dx, du, dw, db, y_again = runs[0]
        assert _same(y_again, y), tag + ": compute_y differs from the forward"
        assert du.shape == u.shape and dx.shape == x.shape and dw.shape == db.shape == (h,) and dw.dtype == db.dtype == w.dtype
        _cmp(tag + " dx", dx, tw.dx, F.gn_bound_dx(tw, dtype))
        _cmp(tag + " du", du.reshape(n, d), tw.du, F.gn_bound_du(tw, dtype))
        _cmp(tag + " dw", dw, tw.dw, F.gn_bound_dw(tw, w.dtype))
        _cmp(tag + " db", db, tw.db, F.gn_bound_db(tw, w.dtype))
        if n == 0:
            assert bool((dw == 0).all()) and bool((db == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,l", [(67, 8), (67, 256), (5, 2056)])
def test_one_head_has_the_masks_of_the_layer_norm(n, l, dtype):
    H = _H()
    x, u = _rand(n, l, dtype), _rand(n, l, dtype)
    w1, b1 = _params(1, torch.float32)
    wd, bd = _params(l, torch.float32)
    gn = H.triton_group_norm_mul_dropout_fwd(x, u, w1, b1, EPS, 0.3, True, True, 1, l, SEED)[0]
    ln = H.triton_layer_norm_mul_dropout_fwd(x, u, wd, bd, EPS, 0.3, True, True, SEED)[0]
    assert _same(gn[:, :2 * l].clone(), ln[:, :2 * l].clone())   # drop0(u) and drop1(x): the same values, the same masks
    assert torch.equal(gn[:, 2 * l:] == 0, ln[:, 2 * l:] == 0)
    kept = F.keep_mask(SEED, n, l, 2, 0.3)
    assert torch.equal((gn[:, 2 * l:] != 0).cpu(), kept)


# ---- 3. head isolation ----
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("h,l", [(4, 64), (6, 12), (8, 257)])
def test_heads_do_not_see_each_other(h, l, dtype):
    H = _H()
    n, d, hp = 5, h * l, 1   # hp: the perturbed head
    x, u, dy = _rand(n, d, dtype), _rand(n, d, dtype), _rand(n, d, dtype)
    w, b = _params(h, torch.float32)
    others = torch.ones(d, dtype=torch.bool)
    others[hp * l:(hp + 1) * l] = False
    oh = torch.ones(h, dtype=torch.bool)
    oh[hp] = False

    def run(x, u, dy):
        y, mean, rstd, bd, bh, nw, seed = H.triton_group_norm_mul_dropout_fwd(x, u, w, b, EPS, 0.3, True, False, h, l, SEED)
        dx, du, dw, db, _ = H.triton_group_norm_mul_dropout_bwd(dy, x, u, w, b, mean, rstd, bd, bh, nw, EPS, True, 0.3, seed,
                                                                False, h, l)
        return y, mean.view(n, h), rstd.view(n, h), dx, du, dw, db

    base = run(x, u, dy)
    x2, u2, dy2 = x.clone(), u.clone(), dy.clone()
    x2[:, hp * l:(hp + 1) * l] += 1.0
    u2[:, hp * l:(hp + 1) * l] *= 2.0
    fwd = run(x2, u2, dy)
    assert not _same(fwd[0], base[0])
    for i in (0, 3, 4):
        assert _same(fwd[i][:, others], base[i][:, others]), f"forward output {i} of another head changed"
    for i in (1, 2):
        assert _same(fwd[i][:, oh], base[i][:, oh]), f"statistics {i} of another head changed"
    dy2[:, hp * l:(hp + 1) * l] *= -3.0
    bwd = run(x, u, dy2)
    assert not _same(bwd[3], base[3])
    for i in (3, 4):
        assert _same(bwd[i][:, others], base[i][:, others]), f"gradient {i} of another head changed"
    for i in (5, 6):
        assert _same(bwd[i][oh], base[i][oh]), f"parameter gradient {i} of another head changed"


# ---- 4. autograd wrappers ----
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n,h,l", [(67, 6, 12), (67, 8, 128), (5, 8, 257)])
def test_autograd_wrappers_equal_the_raw_calls(n, h, l, dtype):
    H = _H()
    d = h * l
    x, u = _rand(n, d, dtype, 0.0, True).requires_grad_(True), _u_of(n, h, l, dtype, True).requires_grad_(True)
    w, b = (t.requires_grad_(True) for t in _params(h, torch.float32))
    xd, ud, wd, bd = x.detach(), u.detach(), w.detach(), b.detach()
    for concat_ux in (False, True):
        dy = _rand(n, 3 * d if concat_ux else d, dtype)
        y = H.triton_norm_mul_dropout(x, u, w, b, EPS, 0.3, True, concat_ux, True, h, l, SEED)
        y.backward(dy)
        got = (x.grad, u.grad, w.grad, b.grad)
        y0, mean, rstd, bD, bH, nw, seed = H.triton_group_norm_mul_dropout_fwd(xd, ud, wd, bd, EPS, 0.3, True, concat_ux, h, l, SEED)
        want = H.triton_group_norm_mul_dropout_bwd(dy, xd, ud, wd, bd, mean, rstd, bD, bH, nw, EPS, True, 0.3, seed, concat_ux, h, l)
        assert _same(y.detach(), y0) and all(_same(p, q) for p, q in zip(got, want[:4]))
        assert got[1].shape == u.shape
        for t in (x, u, w, b):
            t.grad = None
    wf, bf = (t.requires_grad_(True) for t in _params(d, torch.float32))
    dy = _rand(n, d, dtype)
    y = H.triton_swish_layer_norm(x, wf, bf, EPS)
    y.backward(dy)
    y0, mean, rstd = H.triton_swish_layer_norm_fwd(xd, wf.detach(), bf.detach(), EPS)
    want = H.triton_swish_layer_norm_bwd(dy, xd, wf.detach(), bf.detach(), mean, rstd)
    assert _same(y.detach(), y0) and all(_same(p, q) for p, q in zip((x.grad, wf.grad, bf.grad), want))
    x.grad = wf.grad = None
    y = H.rms_norm(x, wf, EPS)
    y.backward(dy)
    y0, rstd = H.triton_rms_norm_fwd(xd, wf.detach(), EPS)
    want = H.triton_rms_norm_bwd(dy, xd, wf.detach(), rstd)
    assert _same(y.detach(), y0) and all(_same(p, q) for p, q in zip((x.grad, wf.grad), want))


# ---- 5. graph capture ----
def test_forwards_are_capturable():
    H = _H()
    n, h, l = 67, 4, 64
    d = h * l
    x, u = _rand(n, d, torch.bfloat16, 0.0, True), _u_of(n, h, l, torch.bfloat16, False)
    w, b = _params(h, torch.float32)
    wd, bd = _params(d, torch.float32)

    def chain():
        y1 = H.triton_rms_norm_fwd(x, wd, EPS)[0]
        y2 = H.triton_swish_layer_norm_fwd(y1, wd, bd, EPS)[0]
        return y1, y2, H.triton_group_norm_mul_dropout_fwd(y2, u, w, b, EPS, 0.3, True, False, h, l, SEED)[0]

    expect = chain()   # (loads the library outside the capture)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            outs = chain()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same(p, q) for p, q in zip(outs, expect))
    assert bool((outs[2] != 0).any())
