"""Delta-q backward (mi355_hstu_attn_bwd_kv: fewer queries than keys, the queries of a sequence being the last Lq of its Lk keys)
against the CPU oracle.  The reference values are `ho.hstu_attn_bwd` on q / dout padded with zero rows up to Lk per sequence
(tests/test_hstu_delta_q_bwd_cpu.py pins that identity); the per-element floors are `ho.hstu_attn_magnitudes` on the same padded
inputs.  One jagged batch around the kernels' tile sizes (128 query rows per workgroup, 64 keys per tile, 32-row groups):
offsets 70, 37, 299, 50, 0, 224 -- a query block that crosses 128, a single query, a sequence without queries, one with Lq == Lk.
drab is held to the same element-wise rule (k = 4) with its magnitude = |dS| summed as the oracle sums drab, over the heads when the
bias has one shared head (_drab_magnitude: a second magnitude pass, not the max-norm rule)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import hstu_oracle as ho

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 6, 2
LQ = [130, 9, 1, 0, 64, 33]
LK = [200, 46, 300, 50, 64, 257]
MAXQ, MAXK, SCALE = 130, 300, 200
OFFQ = np.concatenate([[0], np.cumsum(LQ)]).astype(np.int64)
OFFK = np.concatenate([[0], np.cumsum(LK)]).astype(np.int64)
MODES = ["causal", "full", "window_20_0", "window_7_5", "targets", "ctx_targets", "rab", "rab_shared_drab"]


def _bf16_ulp(x):
    """spacing of bfloat16 at |x| (8 significand bits)"""
    ax = np.maximum(np.abs(x), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 7)


def _close_elementwise(actual, ref, mag, k, bits=7, what=""):
    """the rule of tests/test_hstu_gpu.py (copied): |x - ref| <= 1e-3 |ref| + 1 ulp(ref) + k * 2^-(bits + 2) * mag, element by
    element, mag = the accumulated magnitude of the element's summands; bits = 7 bf16, 10 fp16"""
    a = actual.detach().float().cpu().numpy().astype(np.float64)
    ref = np.asarray(ref, np.float64)
    ulp = _bf16_ulp(ref) * 2.0 ** (7 - bits)
    if bits == 10:
        ulp = np.maximum(ulp, 2.0 ** -24)
    tol = 1e-3 * np.abs(ref) + ulp + k * 2.0 ** -(bits + 2) * np.asarray(mag, np.float64) + 1e-30
    ratio = float((np.abs(a - ref) / tol).max()) if a.size else 0.0
    print(f"{what}: worst use of the tolerance {ratio:.3f}")
    try:   # the worst use of the tolerance goes to the terminal summary (conftest.py)
        from conftest import record_tolerance_use

        record_tolerance_use(f"{'fp16' if bits == 10 else 'bf16'} k={k}", os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], ratio)
    except ImportError:
        pass
    bad = np.abs(a - ref) > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements off: worst excess {ratio:.2f} x its tolerance"


def pad_rows(x, offq=OFFQ, offk=OFFK):
    """rows of x (Lq per sequence) moved to the END of that sequence's Lk rows, zeros in front"""
    out = np.zeros((int(offk[-1]),) + x.shape[1:], x.dtype)
    for b in range(len(offq) - 1):
        lq = int(offq[b + 1] - offq[b])
        out[int(offk[b + 1]) - lq:int(offk[b + 1])] = x[int(offq[b]):int(offq[b + 1])]
    return out


def unpad_rows(x, offq=OFFQ, offk=OFFK):
    return np.concatenate([x[int(offk[b + 1]) - int(offq[b + 1] - offq[b]):int(offk[b + 1])] for b in range(len(offq) - 1)])


def _mode_kwargs(mode):
    """(oracle kwargs, window_size, num_contexts, num_targets, group, rab kind) of a mode"""
    if mode == "causal":
        return {"causal": True}, (-1, 0), None, None, 1
    if mode == "full":
        return {"causal": False}, (-1, -1), None, None, 1
    if mode.startswith("window"):
        wl, wr = (int(x) for x in mode.split("_")[1:])
        return {"local_window": (wl, wr)}, (wl, wr), None, None, 1
    if mode == "targets":
        nt = np.minimum(np.array([8, 5, 1, 0, 7, 8]), np.array(LQ))
        return {"causal": True, "num_targets": nt, "target_group_size": 2}, (-1, 0), None, nt, 2
    if mode == "ctx_targets":
        # contextual rows in front of the first query (sequences 0, 1, 2, 5), among the queries (4: Lq == Lk) and none (3)
        nt = np.minimum(np.array([8, 5, 1, 0, 7, 8]), np.array(LQ))
        nc = np.array([3, 2, 4, 0, 5, 1])
        return {"causal": True, "num_targets": nt, "num_contextuals": nc, "target_group_size": 2}, (-1, 0), nc, nt, 2
    return {"causal": True}, (-1, 0), None, None, 1   # rab, rab_shared_drab


@functools.lru_cache(maxsize=None)
def _inputs(d, dtype):
    g = torch.Generator(device="cpu").manual_seed(1000 + d)
    mk = lambda n, lo, hi: torch.empty(n, H, d).uniform_(lo, hi, generator=g).to(dtype)
    q, dout = mk(int(OFFQ[-1]), -1, 1), mk(int(OFFQ[-1]), 0, 1)
    k, v = mk(int(OFFK[-1]), -1, 1), mk(int(OFFK[-1]), -1, 1)
    rab = torch.empty(B, H, MAXK, MAXK).uniform_(-1, 1, generator=g).to(dtype)
    return q, k, v, dout, rab


def _drab_magnitude(dn, qn, kn, vn, rab, alpha, shared):
    """|dS| behind every drab element, summed as the oracle sums drab (over the heads when the bias is shared): the causal mask of
    the rab modes, restated from the oracle's own pieces on the padded inputs"""
    qp, dp_ = pad_rows(qn), pad_rows(dn)
    mag = np.zeros(rab.shape)
    for b in range(B):
        lo, hi = int(OFFK[b]), int(OFFK[b + 1])
        L = hi - lo
        m = ho.valid_mask(L, True, None, None, 1)
        for hd in range(H):
            s = alpha * (qp[lo:hi, hd] @ kn[lo:hi, hd].T + ho._rab_of(rab, b, hd, L))
            ds = (np.abs(dp_[lo:hi, hd]) @ np.abs(vn[lo:hi, hd]).T) * m * np.abs(ho._dsilu(s)) / SCALE * alpha
            mag[b, 0 if shared else hd, :L, :L] += ds
    return mag


@functools.lru_cache(maxsize=None)
def _reference(d, mode, dtype):
    """oracle values of (out, dq, dk, dv, drab or None) and their magnitudes, computed once per (d, mode, dtype)"""
    q, k, v, dout, rab = _inputs(d, dtype)
    okw = dict(_mode_kwargs(mode)[0])
    qn, kn, vn, dn = (t.float().numpy().astype(np.float64) for t in (q, k, v, dout))
    rn = None
    if mode.startswith("rab"):
        rn = (rab[:, :1] if mode == "rab_shared_drab" else rab).float().numpy().astype(np.float64)
        okw["rab"] = rn
    alpha = 1.0 / d ** 0.5
    qp, dp_ = pad_rows(qn), pad_rows(dn)
    out = unpad_rows(ho.hstu_attn_fwd(qp, kn, vn, OFFK, alpha, SCALE, **okw))
    res = ho.hstu_attn_bwd(dp_, qp, kn, vn, OFFK, alpha, SCALE, **okw)
    mo, mq, mk, mv = ho.hstu_attn_magnitudes(dp_, qp, kn, vn, OFFK, alpha, SCALE, **okw)
    drab = res[3] if rn is not None else None
    mdrab = _drab_magnitude(dn, qn, kn, vn, rn, alpha, mode == "rab_shared_drab") if mode == "rab_shared_drab" else None
    return (out, unpad_rows(res[0]), res[1], res[2], drab), (unpad_rows(mo), unpad_rows(mq), mk, mv, mdrab)


def _dev_i32(x):
    return None if x is None else torch.from_numpy(np.asarray(x, np.int32)).to(DEV)


def _call(d, mode, dtype, grad=True, **extra):
    from hstu import hstu_attn_varlen_func

    q, k, v, dout, rab = _inputs(d, dtype)
    _, win, nc, nt, grp = _mode_kwargs(mode)
    qq, kk, vv = (t.to(DEV).requires_grad_(grad) for t in (q, k, v))
    rr = None
    if mode.startswith("rab"):
        rr = (rab[:, :1] if mode == "rab_shared_drab" else rab).contiguous().to(DEV).requires_grad_(mode == "rab_shared_drab")
    kw = dict(target_group_size=grp, window_size=win, alpha=1.0 / d ** 0.5, rab=rr, has_drab=mode == "rab_shared_drab")
    kw.update(extra)
    out = hstu_attn_varlen_func(qq, kk, vv, _dev_i32(OFFQ), _dev_i32(OFFK), None, None, MAXQ, MAXK, SCALE, _dev_i32(nc), _dev_i32(nt), **kw)
    if grad:
        out.backward(dout.to(DEV))
    return out, qq, kk, vv, rr


def _check_parity(d, mode, dtype, bits):
    out, qq, kk, vv, rr = _call(d, mode, dtype)
    (r_out, r_dq, r_dk, r_dv, r_drab), (mo, mq, mk, mv, mdrab) = _reference(d, mode, dtype)
    _close_elementwise(out, r_out, mo, 2, bits, "out")
    _close_elementwise(qq.grad, r_dq, mq, 4, bits, "dq")
    _close_elementwise(kk.grad, r_dk, mk, 4, bits, "dk")
    _close_elementwise(vv.grad, r_dv, mv, 4, bits, "dv")
    if mode == "rab_shared_drab":
        assert rr.grad.shape == rr.shape
        _close_elementwise(rr.grad, r_drab, mdrab, 4, bits, "drab")   # magnitude: |dS| summed over the heads, as the oracle sums drab


@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("mode", MODES)
def test_parity_with_the_padded_oracle(d, mode):
    _check_parity(d, mode, torch.bfloat16, 7)


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("mode", ["causal", "window_7_5"])
def test_parity_fp16(d, mode):
    _check_parity(d, mode, torch.float16, 10)


def _raw(d, mode, dtype=torch.bfloat16):
    from hstu import hstu_varlen_bwd_kv

    q, k, v, dout, rab = _inputs(d, dtype)
    _, win, nc, nt, grp = _mode_kwargs(mode)
    args = [t.to(DEV) for t in (dout, q, k, v)] + [_dev_i32(OFFQ), _dev_i32(OFFK)]
    nc, nt = _dev_i32(nc), _dev_i32(nt)   # (everything but the outputs is allocated here, not inside the call)
    return lambda: hstu_varlen_bwd_kv(*args, MAXQ, MAXK, SCALE, nc, nt, grp, win[0], win[1], 1.0 / d ** 0.5)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("mode", ["causal", "window_7_5"])
def test_every_gradient_row_is_written(d, mode):
    """dq / dk / dv come from torch.empty: between two calls the caching allocator's free blocks of their sizes are filled with
    NaN bit patterns, so the second call's outputs land in poisoned storage.  The (0, 50) sequence has no queries -- its dk / dv
    rows are exactly zero --, and under the window the keys left of every query's reach are zero as well."""
    run = _raw(d, mode)
    first = run()
    sizes = [t.numel() for t in first[:3]]
    del first
    poison = [torch.full((n,), float("nan"), dtype=torch.bfloat16, device=DEV) for n in sizes]
    reused = {p.data_ptr() for p in poison}
    del poison
    dq, dk, dv, _ = run()
    assert {dq.data_ptr(), dk.data_ptr(), dv.data_ptr()} & reused, "the allocator did not hand the poisoned blocks back"
    for t in (dq, dk, dv):
        assert not torch.isnan(t.float()).any()
    lo, hi = int(OFFK[3]), int(OFFK[4])
    assert not dk[lo:hi].float().abs().max().item() and not dv[lo:hi].float().abs().max().item()
    if mode == "window_7_5":   # sequence 2: one query at position 299 reaches keys 292 .. 299 only
        lo = int(OFFK[2])
        assert not dk[lo:lo + 292].float().abs().max().item() and not dv[lo:lo + 292].float().abs().max().item()


@pytest.mark.parametrize("d", [32, 256])
def test_deterministic(d):
    run = _raw(d, "ctx_targets")
    a, b = run(), run()
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("mode", ["causal", "window_7_5", "ctx_targets"])
def test_agrees_with_the_padding_workaround(d, mode):
    """today's public path to these gradients: the self-attention backward on q / dout padded with zero rows up to Lk.  Same
    bf16 operands, possibly another summation order: both sides within the element-wise rule of each other's reference, i.e. the
    new path is held to the oracle's magnitudes around the padded path's values."""
    from hstu import hstu_attn_varlen_func

    q, k, v, dout, _ = _inputs(d, torch.bfloat16)
    _, win, nc, nt, grp = _mode_kwargs(mode)
    dq, dk, dv, _ = _raw(d, mode)()
    qp = torch.from_numpy(pad_rows(q.float().numpy())).to(torch.bfloat16).to(DEV).requires_grad_(True)
    dp_ = torch.from_numpy(pad_rows(dout.float().numpy())).to(torch.bfloat16).to(DEV)
    kk, vv = k.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    cu = _dev_i32(OFFK)
    out = hstu_attn_varlen_func(qp, kk, vv, cu, cu, None, None, MAXK, MAXK, SCALE, _dev_i32(nc), _dev_i32(nt), target_group_size=grp,
                                window_size=win, alpha=1.0 / d ** 0.5)
    out.backward(dp_)
    _, (_, mq, mk, mv, _) = _reference(d, mode, torch.bfloat16)
    pdq = torch.from_numpy(unpad_rows(qp.grad.float().cpu().numpy()))
    _close_elementwise(dq, pdq.numpy(), mq, 4, what="dq vs padded")
    _close_elementwise(dk, kk.grad.float().cpu().numpy(), mk, 4, what="dk vs padded")
    _close_elementwise(dv, vv.grad.float().cpu().numpy(), mv, 4, what="dv vs padded")


def test_still_refused():
    from hstu import hstu_attn_varlen_func

    d = 64
    q, k, v, _, _ = _inputs(d, torch.bfloat16)
    qq, kk, vv = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    cq, ck = _dev_i32(OFFQ), _dev_i32(OFFK)
    base = (None, None, MAXQ, MAXK, SCALE, None, None)
    # a paged cache with a gradient (the argument check comes before anything touches the cache)
    cache = torch.zeros(4, 2, 32, H, d, dtype=torch.bfloat16, device=DEV)
    pages = dict(kv_cache=cache, page_offsets=_dev_i32(np.arange(B + 1)), page_ids=_dev_i32(np.zeros(B)), last_page_lens=_dev_i32(np.ones(B)))
    with pytest.raises(NotImplementedError, match="paged KV cache"):
        hstu_attn_varlen_func(qq, kk, vv, cq, ck, *base, window_size=(-1, 0), alpha=0.125, **pages)
    with pytest.raises(NotImplementedError, match="paged KV cache"):
        hstu_attn_varlen_func(qq, kk, vv, cq, ck, *base, window_size=(7, 5), alpha=0.125, **pages)
    # func over delta-q keys with a gradient
    func = torch.full((1, 1, int(OFFQ[-1])), MAXK, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError, match="func"):
        hstu_attn_varlen_func(qq, kk, vv, cq, ck, *base, window_size=(-1, 0), alpha=0.125, func=func)
    # FP8 over delta-q keys
    with pytest.raises(NotImplementedError, match="delta-q"):
        hstu_attn_varlen_func(qq, kk, vv, cq, ck, *base, window_size=(-1, 0), alpha=0.125, quant_mode=0)
    # without a gradient the forward-only paths still answer
    with torch.no_grad():
        out = hstu_attn_varlen_func(qq, kk, vv, cq, ck, *base, window_size=(-1, 0), alpha=0.125, func=func)
    assert out.shape == q.shape


def test_bad_arguments_are_error_codes():
    from hstu import hstu_varlen_bwd_kv

    q, k, v, dout, _ = _inputs(32, torch.bfloat16)
    args = [t.to(DEV) for t in (dout, q, k, v)]
    with pytest.raises(Exception, match="max_seqlen_q <= max_seqlen_k"):
        hstu_varlen_bwd_kv(*args, _dev_i32(OFFQ), _dev_i32(OFFK), MAXK + 1, MAXK, SCALE, None, None, 1, -1, 0, 0.2)
    with pytest.raises(Exception, match="causal"):   # target rows under a window
        hstu_varlen_bwd_kv(*args, _dev_i32(OFFQ), _dev_i32(OFFK), MAXQ, MAXK, SCALE, None, _dev_i32(np.zeros(B)), 1, 7, 5, 0.2)
