"""GPU checks of the HSTU layer norms (csrc/norm_ops.hip behind hstu_norm) against the float64 twin of tests/norm_twin.py,
element by element under the bounds stated there; every comparison prints its worst |err| / bound.

Rows: N in {0, 1, 5, 67, 1031}: the empty call, fewer rows than a block's four waves, no multiple of a wave or block count.
The grids are resident (at most 2048 blocks forward, 512 / 1024 backward), so two more shapes, bf16 only, make a wave and a
workgroup walk more than one row: 8197 x 8 (more rows than the 8192 waves of the forward) and 2051 x 2056 (more than the 2048
workgroups; 8 MB, the largest case).
Widths: D in {8, 72, 256, 1024} at every N, and with N in {5, 67} one D past each boundary of the kernels:
  520   past 512: a lane holds 16 elements, not 8          1032  past 1024: a lane holds 32
  2056  past 2048: a workgroup per row, LDS sums (16 a thread)   4104  past 4096: 32 a thread
  2050  no multiple of 8 or 4: the element-wise path (one element an access) of the workgroup kernels; the 3-D u of D = 8
        (UD = 2) takes the element-wise path of the wave kernels.
Dtypes: bf16, fp16, fp32 rows; weights in fp32 and in the row dtype."""
import pytest
import torch

import norm_twin as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
SHAPES = [(n, d) for d in (8, 72, 256, 1024) for n in (0, 1, 5, 67, 1031)] + \
         [(n, d) for d in (520, 1032, 2050, 2056, 4104) for n in (5, 67)]
LOOP_SHAPES = [(8197, 8), (2051, 2056)]
CASES = [(n, d, t) for (n, d) in SHAPES for t in DTYPES] + [(n, d, torch.bfloat16) for (n, d) in LOOP_SHAPES]
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
    ratio = T.worst(got, ref, bound)
    print(f"{name}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: worst |err| / bound = {ratio}"


def _same(a, b):
    if a is None or b is None:
        return a is b
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _u_of(n, d, dtype, three_d, shift=0.0):
    """u as the layer passes it: a column slice of a [n, 4 d] buffer, or [n, H, d / H] cut from a wider buffer"""
    if not three_d:
        return (torch.randn(n, 4 * d) + shift).to(dtype).to(DEV)[:, d:2 * d]
    h = 4 if d % 4 == 0 else 2
    return (torch.randn(n, h, d // h + 8) + shift).to(dtype).to(DEV)[:, :, 8:]


def _du_with_sentinel(u):
    """a strided tensor of u's shape inside a buffer filled with 7"""
    if u.dim() == 2:
        buf = torch.full((u.size(0), u.size(1) + 16), 7.0, dtype=u.dtype, device=DEV)
        return buf, buf[:, 8:8 + u.size(1)]
    buf = torch.full((u.size(0), u.size(1), u.size(2) + 16), 7.0, dtype=u.dtype, device=DEV)
    return buf, buf[:, :, 8:8 + u.size(2)]


# ---- 1. layer norm ----
@pytest.mark.parametrize("n,d,dtype", CASES)
def test_layer_norm_fwd_bwd(n, d, dtype):
    H = _H()
    # (learnable, strided, shift, dx_accumulate, weights in the row dtype)
    for learnable, strided, shift, with_acc, row_w in ((True, False, 0.0, False, False), (True, True, 3.0, True, True),
                                                       (False, True, 0.0, False, False)):
        tag = f"ln n={n} d={d} {dtype} learnable={learnable} strided={strided}"
        x, dy = _rand(n, d, dtype, shift, strided), _rand(n, d, dtype, 0.0, strided)
        w, b = _params(d, dtype if row_w else torch.float32) if learnable else (None, None)
        acc = _rand(n, d, dtype, 0.0, strided) if with_acc else None
        y, mean, rstd, block_d, num_warps = H.triton_weighted_layer_norm_fwd(x, w, b, EPS)
        assert y.shape == x.shape and y.dtype == dtype and y.is_contiguous()
        assert mean.dtype == rstd.dtype == torch.float32 and mean.shape == rstd.shape == (n,)
        fw = T.layer_norm_fwd(x, w, b, EPS)
        _cmp(tag + " mean", mean, fw.mean, T.bound_mean(fw))
        _cmp(tag + " rstd", rstd, fw.rstd, T.bound_rstd(fw))
        _cmp(tag + " y", y, fw.y, T.bound_y(fw, dtype))
        runs = [H.triton_weighted_layer_norm_bwd(dy, x, w, b, mean, rstd, learnable, EPS, block_d, num_warps, acc)
                for _ in range(2)]
        dx, dw, db = runs[0]
        assert all(_same(p, q) for p, q in zip(*runs)), tag + ": the backward is not reproducible"
        bw = T.layer_norm_bwd(dy, x, w, EPS, dx_accumulate=acc)
        assert dx.shape == x.shape and dx.dtype == dtype
        _cmp(tag + " dx", dx, bw.dx, T.bound_dx(bw, dtype))
        if learnable:
            assert dw.dtype == db.dtype == w.dtype and dw.shape == db.shape == (d,)
            _cmp(tag + " dw", dw, bw.dw, T.bound_dw(bw, w.dtype))
            _cmp(tag + " db", db, bw.db, T.bound_db(bw, w.dtype))
        else:
            assert dw is None and db is None
        if learnable and not strided:
            # statistics passed in, deliberately 1 % off: the output follows them and they are left as they are
            m2, r2 = (mean * 1.01).contiguous(), (rstd * 1.01).contiguous()
            m2c, r2c = m2.clone(), r2.clone()
            y2 = H.triton_weighted_layer_norm_fwd(x, w, b, EPS, m2, r2)[0]
            assert torch.equal(m2, m2c) and torch.equal(r2, r2c)
            given = T.layer_norm_fwd(x, w, b, EPS, mean=m2, rstd=r2)
            _cmp(tag + " y of given statistics", y2, given.y, T.bound_y(given, dtype))
            if n >= 5:
                assert not torch.equal(y2, y)


# ---- 2. layer norm mul dropout, training=False ----
@pytest.mark.parametrize("n,d,dtype", CASES)
def test_ln_mul_dropout_eval(n, d, dtype):
    H = _H()
    # (u 3-D, concat_ux, du supplied, weights in the row dtype, shift)
    for three_d, concat_ux, own_du, row_w, shift in ((False, False, False, False, 0.0), (True, True, True, True, 3.0),
                                                     (False, True, True, False, 0.0)):
        tag = f"lmd n={n} d={d} {dtype} 3d={three_d} concat={concat_ux}"
        x, u = _rand(n, d, dtype, shift, True), _u_of(n, d, dtype, three_d, shift)
        w, b = _params(d, dtype if row_w else torch.float32)
        dy = _rand(n, 3 * d if concat_ux else d, dtype, 0.0, True)
        y, mean, rstd, block_d, num_warps, seed = H.triton_layer_norm_mul_dropout_fwd(x, u, w, b, EPS, 0.3, False, concat_ux)
        assert y.shape == (n, 3 * d if concat_ux else d) and y.dtype == dtype
        tw = T.ln_mul_dropout_bwd(dy, x, u, w, b, EPS, 0.3, False, concat_ux)
        _cmp(tag + " mean", mean, tw.mean, T.bound_mean(tw))
        _cmp(tag + " rstd", rstd, tw.rstd, T.bound_rstd(tw))
        _cmp(tag + " y", y, tw.out, T.bound_out(tw, dtype, concat_ux))
        runs = []
        for _ in range(2):
            buf, du_in = _du_with_sentinel(u) if own_du else (None, None)
            out = H.triton_layer_norm_mul_dropout_bwd(dy, x, u, w, b, mean, rstd, block_d, num_warps, EPS, False, 0.3, seed,
                                                      concat_ux, True, None, du_in)
            if own_du:
                assert out[1] is du_in
                got = out[1].clone()
                du_in.fill_(7.0)
                assert bool((buf == 7.0).all()), tag + ": something outside du was written"
                out = (out[0], got) + out[2:]
            runs.append(out)
        assert all(_same(p, q) for p, q in zip(*runs)), tag + ": the backward is not reproducible"
        dx, du, dw, db, y_again = runs[0]
        assert _same(y_again, y), tag + ": compute_y differs from the forward"
        assert du.shape == u.shape
        _cmp(tag + " dx", dx, tw.dx, T.bound_dx(tw, dtype))
        _cmp(tag + " du", du.reshape(n, d), tw.du, T.bound_du(tw, dtype))
        _cmp(tag + " dw", dw, tw.dw, T.bound_dw(tw, w.dtype))
        _cmp(tag + " db", db, tw.db, T.bound_db(tw, w.dtype))
        if n == 0:
            assert bool((dw == 0).all()) and bool((db == 0).all())


# ---- 3. training=True ----
@pytest.mark.parametrize("concat_ux", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", [s for s in SHAPES if s[0] >= 5])
def test_ln_mul_dropout_training(n, d, dtype, concat_ux):
    H = _H()
    x, u = _rand(n, d, dtype), _u_of(n, d, dtype, d % 16 == 8)
    w, b = _params(d, torch.float32)
    dy = _rand(n, 3 * d if concat_ux else d, dtype)
    y_eval = H.triton_layer_norm_mul_dropout_fwd(x, u, w, b, EPS, 0.3, False, concat_ux)[0]
    for p in (0.0, 0.3):
        tag = f"lmd training n={n} d={d} {dtype} concat={concat_ux} p={p}"
        y, mean, rstd, block_d, num_warps, seed = H.triton_layer_norm_mul_dropout_fwd(x, u, w, b, EPS, p, True, concat_ux, SEED)
        assert seed == SEED
        if p == 0.0:
            assert _same(y, y_eval), tag + ": p = 0 differs from training=False"
        tw = T.ln_mul_dropout_bwd(dy, x, u, w, b, EPS, p, True, concat_ux, SEED)
        # the zero pattern is the twin's mask wherever the value before dropout is not zero
        nonzero = (tw.undropped != 0) & (y_eval.cpu().double() != 0)
        assert torch.equal((y.cpu() != 0)[nonzero], tw.kept[nonzero]), tag + ": the mask differs from the twin's"
        assert bool((y.cpu()[~tw.kept] == 0).all())
        _cmp(tag + " y", y, tw.out, T.bound_out(tw, dtype, concat_ux))
        runs = [H.triton_layer_norm_mul_dropout_bwd(dy, x, u, w, b, mean, rstd, block_d, num_warps, EPS, True, p, seed,
                                                    concat_ux, True) for _ in range(2)]
        assert all(_same(q, r) for q, r in zip(*runs)), tag + ": the backward is not reproducible"
        dx, du, dw, db, y_again = runs[0]
        assert _same(y_again, y), tag + ": compute_y differs from the forward"
        _cmp(tag + " dx", dx, tw.dx, T.bound_dx(tw, dtype))
        _cmp(tag + " du", du.reshape(n, d), tw.du, T.bound_du(tw, dtype))
        _cmp(tag + " dw", dw, tw.dw, T.bound_dw(tw, w.dtype))
        _cmp(tag + " db", db, tw.db, T.bound_db(tw, w.dtype))
        if p > 0 and not concat_ux:
            # the backward used the forward's mask: du is zero exactly where the output was dropped
            assert bool((du.reshape(n, d).cpu()[~tw.kept] == 0).all())


def test_seed_none_follows_torch_manual_seed():
    H = _H()
    x, u = _rand(67, 72, torch.bfloat16), _rand(67, 72, torch.bfloat16)
    w, b = _params(72, torch.float32)
    outs = []
    for _ in range(2):
        torch.manual_seed(99)
        outs.append(H.triton_layer_norm_mul_dropout_fwd(x, u, w, b, EPS, 0.3, True))
    assert outs[0][5] == outs[1][5] and 0 <= outs[0][5] < 2 ** 62
    assert _same(outs[0][0], outs[1][0])
    other = H.triton_layer_norm_mul_dropout_fwd(x, u, w, b, EPS, 0.3, True)
    assert other[5] != outs[0][5] and not _same(other[0], outs[0][0])
    # the mask does not depend on how many rows the call has: the first rows of a longer call
    longer = H.triton_layer_norm_mul_dropout_fwd(torch.cat([x, x]), torch.cat([u, u]), w, b, EPS, 0.3, True, False, outs[0][5])
    assert _same(longer[0][:67].clone(), outs[0][0])


# ---- 5. autograd wrappers ----
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n,d", [(67, 72), (67, 1024), (5, 2056)])
def test_autograd_wrappers_equal_the_raw_calls(n, d, dtype):
    H = _H()
    x, u = _rand(n, d, dtype, 0.0, True).requires_grad_(True), _u_of(n, d, dtype, True).requires_grad_(True)
    w, b = (t.requires_grad_(True) for t in _params(d, torch.float32))
    dy = _rand(n, d, dtype)
    y = H.triton_layer_norm(x, w, b, EPS)
    got = torch.autograd.grad(y, (x, w, b), dy)
    y0, mean, rstd, bd, nw = H.triton_weighted_layer_norm_fwd(x.detach(), w.detach(), b.detach(), EPS)
    want = H.triton_weighted_layer_norm_bwd(dy, x.detach(), w.detach(), b.detach(), mean, rstd, True, EPS, bd, nw)
    assert _same(y.detach(), y0) and all(_same(p, q) for p, q in zip(got, want))
    y = H.layer_norm(x, None, None, EPS)
    (gx,) = torch.autograd.grad(y, (x,), dy)
    y0, mean, rstd, bd, nw = H.triton_weighted_layer_norm_fwd(x.detach(), None, None, EPS)
    assert _same(y.detach(), y0)
    assert _same(gx, H.triton_weighted_layer_norm_bwd(dy, x.detach(), None, None, mean, rstd, False, EPS, bd, nw)[0])
    for concat_ux in (False, True):
        dy = _rand(n, 3 * d if concat_ux else d, dtype)
        y = H.triton_norm_mul_dropout(x, u, w, b, EPS, 0.3, True, concat_ux, seed=SEED)
        got = torch.autograd.grad(y, (x, u, w, b), dy)
        y0, mean, rstd, bd, nw, seed = H.triton_layer_norm_mul_dropout_fwd(x.detach(), u.detach(), w.detach(), b.detach(), EPS,
                                                                           0.3, True, concat_ux, SEED)
        want = H.triton_layer_norm_mul_dropout_bwd(dy, x.detach(), u.detach(), w.detach(), b.detach(), mean, rstd, bd, nw, EPS,
                                                   True, 0.3, seed, concat_ux)
        assert _same(y.detach(), y0) and all(_same(p, q) for p, q in zip(got, want[:4]))
        assert got[1].shape == u.shape


# ---- 6. graph capture ----
def test_forwards_are_capturable():
    H = _H()
    n, d = 67, 256
    x, u = _rand(n, d, torch.bfloat16, 0.0, True), _u_of(n, d, torch.bfloat16, False)
    w, b = _params(d, torch.float32)
    H.triton_weighted_layer_norm_fwd(x, w, b, EPS)   # (loads the library outside the capture)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            y1 = H.triton_weighted_layer_norm_fwd(x, w, b, EPS)[0]
            y2 = H.triton_layer_norm_mul_dropout_fwd(y1, u, w, b, EPS, 0.3, False)[0]
    y1.zero_()
    y2.zero_()
    graph.replay()
    torch.cuda.synchronize()
    e1 = H.triton_weighted_layer_norm_fwd(x, w, b, EPS)[0]
    e2 = H.triton_layer_norm_mul_dropout_fwd(e1, u, w, b, EPS, 0.3, False)[0]
    assert _same(y1, e1) and _same(y2, e2)
    assert bool((y2 != 0).any())
