"""Mask functions (`func`) beside a relative attention bias (`rab`), both read inside the kernels
(mi355_hstu_attn_{fwd_kv,bwd}_rab_func): forward, dq / dk / dv and drab against the float64 oracle under the full mask, the causal mask
and the causal mask with contextual + target rows; bit equality with the dense statement of the same call (the functions as a
0 / -1e9 bias added to rab, through the rab kernels); delta-q keys and the paged cache; the packed entry point and the raw fbgemm ops;
a shared bias head under per-head functions; the memory bound; the MI355_HSTU_FUNC_DENSE switch.

Shapes: one jagged batch with an empty sequence, a single row, a partial last tile and lengths on both sides of the 32 / 64 / 128 tile
edges, H = 2.  The functions have a prefix of at most 20 keys on most rows and their first band from key 130 on, so the key tile
64 .. 127 is skipped by every wave of such rows; the rows 32 .. 63 of every 128 have a prefix of 64 keys and more (the tile below it
takes the bias and no per-element test); a fifth of the rows see nothing at all.

Tolerance: the project's element-wise rule (_close_elementwise of tests/test_hstu_gpu.py) with the accumulated magnitudes of
oracle.hstu_attn_magnitudes.  That function takes no `func`; it is given the bias with -1e9 added wherever the functions mask, which
makes exactly those summands zero in float64 -- the magnitudes of the masked call, not the larger ones of the unmasked call.  drab is
one dS per element: its magnitude is |dP| alpha / N sigmoid(x) (1 + |x| (1 - sigmoid(x))), the absolute summands of
dS = dP alpha / N SiLU'(x), with the k = 4 of the gradients that are built from dS."""
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import hstu_oracle as ho
from test_hstu_gpu import _assert_drab, _close_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 2
LENGTHS = np.array([0, 1, 33, 127, 130, 200])
CTX = np.array([0, 1, 3, 5, 4, 6])
TGT = np.array([0, 0, 4, 10, 7, 9])
MiB = 1 << 20

# (mask, head dim, n_func, rab heads, func heads, dtype)
ORACLE_CASES = [
    ("full", 32, 1, H, H, "bf16"), ("full", 64, 5, 1, H, "bf16"), ("full", 256, 3, H, 1, "bf16"),
    ("causal", 32, 7, H, 1, "bf16"), ("causal", 64, 3, H, H, "bf16"), ("causal", 256, 5, 1, 1, "bf16"), ("causal", 64, 5, H, H, "fp16"),
    ("ctx_g1", 32, 5, H, H, "bf16"), ("ctx_g1", 64, 7, 1, H, "bf16"), ("ctx_g1", 256, 3, H, H, "bf16"),
    ("ctx_g2", 32, 3, 1, 1, "bf16"), ("ctx_g2", 64, 1, H, H, "bf16"), ("ctx_g2", 256, 7, H, H, "bf16"),
]
_ids = lambda case: "-".join(str(x) for x in case)


def _rng(*name):
    return np.random.default_rng(zlib.crc32("-".join(str(x) for x in name).encode()))


def _ti(a):
    return torch.from_numpy(np.asarray(a, np.int32)).to(DEV)


def make_func(rng, pos, HF, n_func, slack=16, far=130):
    """int32 [HF, n_func, T + slack]: a short prefix (rows 32 .. 63 of every 128: a prefix of 64 keys and more), bands from key
    `far` on (more than one 64-key tile behind the short prefixes), a fifth of the rows blind"""
    T = pos.size
    r = lambda lo, hi: rng.integers(lo, hi, size=(HF, T))
    f = np.zeros((HF, n_func, T + slack), np.int64)
    wide = ((pos // 32) % 4 == 1)[None, :]
    blind = r(0, 5) == 0
    f[:, 0, :T] = np.where(blind, 0, np.where(wide, 64 + r(0, 80), r(0, 21)))
    starts = [(far, far + 20, 40), (far + 45, far + 55, 20), (far + 56, far + 62, 40)]   # the last band runs past the longest sequence
    for p in range(n_func // 2):
        lo = r(starts[p][0], starts[p][1])
        up = np.minimum(lo + r(0, starts[p][2]), starts[p + 1][0] if p + 1 < n_func // 2 else 1 << 20)
        f[:, 2 * p + 1, :T] = np.where(blind, 0, lo)
        f[:, 2 * p + 2, :T] = np.where(blind, 0, up)
    return f.astype(np.int32)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs, the oracle's outputs and gradients, the magnitudes: computed once per case and shared"""
    mask, d, n_func, rab_heads, func_heads, dt = case
    c = Case()
    rng = _rng("case", *case)
    c.tdt, c.bits = (torch.float16, 10) if dt == "fp16" else (torch.bfloat16, 7)
    c.d, c.alpha = d, 1.0 / d ** 0.5
    B, N = LENGTHS.size, int(LENGTHS.max())
    c.B, c.N = B, N
    c.off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    T = int(c.off[-1])
    pos = np.concatenate([np.arange(n) for n in LENGTHS])
    mk = lambda lo, hi, *shape: torch.from_numpy(rng.uniform(lo, hi, shape).astype(np.float32)).to(DEV).to(c.tdt)
    c.q, c.k, c.v, c.dout = mk(-1, 1, T, H, d), mk(-1, 1, T, H, d), mk(-1, 1, T, H, d), mk(0, 1, T, H, d)
    c.rab = mk(-2, 2, B, rab_heads, N, N)
    c.f = make_func(rng, pos, func_heads, n_func)
    c.func = torch.from_numpy(c.f).to(DEV)
    c.cu = _ti(c.off)
    c.causal = mask != "full"
    c.window = (-1, 0) if c.causal else (-1, -1)
    c.ctx = c.tgt = None
    c.grp = 1
    if mask.startswith("ctx"):
        c.ctx = np.minimum(CTX, LENGTHS)
        c.tgt = np.minimum(TGT, LENGTHS - c.ctx)
        c.grp = 2 if mask == "ctx_g2" else 1
    c.nc = None if c.ctx is None else _ti(c.ctx)
    c.nt = None if c.tgt is None else _ti(c.tgt)
    # ---- the oracle (float64), the visible pairs, the magnitudes
    qn, kn, vn, dn = (t.float().cpu().numpy() for t in (c.q, c.k, c.v, c.dout))
    rn = c.rab.float().cpu().numpy().astype(np.float64)
    okw = dict(causal=c.causal, num_targets=c.tgt, num_contextuals=c.ctx, target_group_size=c.grp)
    c.ref = ho.hstu_attn_fwd(qn, kn, vn, c.off, c.alpha, N, rab=rn, func=c.f, **okw)
    c.dq, c.dk, c.dv, c.drab = ho.hstu_attn_bwd(dn, qn, kn, vn, c.off, c.alpha, N, rab=rn, func=c.f, **okw)
    c.visible = np.zeros((B, H, N, N), bool)
    for b in range(B):
        lo, L = int(c.off[b]), int(LENGTHS[b])
        if L == 0:
            continue
        m = ho.valid_mask(L, c.causal, None if c.tgt is None else c.tgt[b], None if c.ctx is None else c.ctx[b], c.grp)
        free = np.zeros((L, L), bool)
        if c.ctx is not None:   # contextual rows x history columns: the functions do not apply (hstu_fwd.h:519-524)
            free = (np.arange(L)[:, None] < c.ctx[b]) & (np.arange(L)[None, :] < L - c.tgt[b])
        for h in range(H):
            c.visible[b, h, :L, :L] = m & (ho.func_mask(c.f, h, lo, L, L) | free)
    rab_masked = np.where(c.visible, np.broadcast_to(rn, (B, H, N, N)), -1e9)
    with np.errstate(over="ignore"):
        c.mags = ho.hstu_attn_magnitudes(dn, qn, kn, vn, c.off, c.alpha, N, rab=rab_masked, **okw)
    mag_drab = np.zeros((B, H, N, N))
    for b in range(B):
        lo, hi = int(c.off[b]), int(c.off[b + 1])
        L = hi - lo
        for h in range(H):
            x = c.alpha * (qn[lo:hi, h].astype(np.float64) @ kn[lo:hi, h].astype(np.float64).T + rn[b, h if rab_heads > 1 else 0, :L, :L])
            sg = 1.0 / (1.0 + np.exp(-x))
            dp = dn[lo:hi, h].astype(np.float64) @ vn[lo:hi, h].astype(np.float64).T
            mag_drab[b, h, :L, :L] = np.abs(dp) * c.alpha / N * sg * (1.0 + np.abs(x) * (1.0 - sg)) * c.visible[b, h, :L, :L]
    c.mag_drab = mag_drab if rab_heads > 1 else mag_drab.sum(1, keepdims=True)
    c.seen_by_any_head = c.visible if rab_heads > 1 else c.visible.any(1, keepdims=True)
    return c


def _grad_inputs(c):
    return [t.clone().requires_grad_(True) for t in (c.q, c.k, c.v, c.rab)]


@functools.lru_cache(maxsize=None)
def _varlen(case):
    """the call through hstu_attn_varlen_func, once per case: (out, dq, dk, dv, drab)"""
    from hstu import hstu_attn_varlen_func

    c = _case(case)
    qq, kk, vv, rr = _grad_inputs(c)
    out = hstu_attn_varlen_func(qq, kk, vv, c.cu, c.cu, None, None, c.N, c.N, c.N, c.nc, c.nt, target_group_size=c.grp,
                                window_size=c.window, alpha=c.alpha, rab=rr, has_drab=True, func=c.func)
    out.backward(c.dout)
    return out.detach(), qq.grad, kk.grad, vv.grad, rr.grad


def _dense_rab(c, rab=None, cu_q=None, cu_k=None, N=None):
    from hstu.hstu_attn_interface import func_mask_bias

    fb = func_mask_bias(c.func, c.cu if cu_q is None else cu_q, c.cu if cu_k is None else cu_k, c.N if N is None else N, c.tdt)
    return ((c.rab if rab is None else rab) + fb).clamp_(min=torch.finfo(c.tdt).min)


def _dense(c):
    """the dense statement of the same call: func=None, the functions as a 0 / -1e9 bias added to rab"""
    from hstu import hstu_attn_varlen_func

    qq, kk, vv, _ = _grad_inputs(c)
    rd = _dense_rab(c).detach().requires_grad_(True)
    out = hstu_attn_varlen_func(qq, kk, vv, c.cu, c.cu, None, None, c.N, c.N, c.N, c.nc, c.nt, target_group_size=c.grp,
                                window_size=c.window, alpha=c.alpha, rab=rd, has_drab=True, func=None)
    out.backward(c.dout)
    return out.detach(), qq.grad, kk.grad, vv.grad, rd.grad


@pytest.mark.parametrize("case", ORACLE_CASES, ids=_ids)
def test_func_beside_rab_forward_backward_and_drab_vs_oracle(case):
    """GPU case 1.  The contextual cases raise NotImplementedError without the in-kernel path (a dense bias cannot exempt the history
    columns of contextual rows)."""
    c = _case(case)
    out, dq, dk, dv, drab = _varlen(case)
    for name, got, want, mag, kk in (("out", out, c.ref, c.mags[0], 2), ("dq", dq, c.dq, c.mags[1], 4), ("dk", dk, c.dk, c.mags[2], 4),
                                     ("dv", dv, c.dv, c.mags[3], 4)):
        assert bool(torch.isfinite(got.float()).all()), name
        _close_elementwise(got, want, mag, kk, bits=c.bits)
    assert tuple(drab.shape) == tuple(c.rab.shape)
    _assert_drab(drab, c.drab)
    _close_elementwise(drab, c.drab, c.mag_drab, 4, bits=c.bits)
    dn = drab.float().cpu().numpy()
    assert not dn[~c.seen_by_any_head].any(), "drab is not zero where the functions / the mask hide the key or outside the sequences"
    assert np.abs(dn[c.seen_by_any_head]).max() > 0 and c.visible.sum() < 0.6 * sum(int(n) ** 2 for n in LENGTHS) * H


@pytest.mark.parametrize("case", [("full", 64, 5, H, H, "bf16"), ("causal", 256, 7, H, 1, "bf16"), ("causal", 32, 3, H, H, "bf16"),
                                  ("full", 64, 3, H, 1, "fp16")], ids=_ids)
def test_func_beside_rab_equals_its_dense_statement_bit_for_bit(case):
    """GPU case 2: masked elements are exactly zero after SiLU and SiLU' on both sides, visible ones see the same rab value"""
    c = _case(case)
    for name, a_, b_ in zip(("out", "dq", "dk", "dv", "drab"), _varlen(case), _dense(c)):
        assert a_.shape == b_.shape
        assert torch.equal(a_, b_), f"{name} differs from the dense statement in {int((a_ != b_).sum())} elements"


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("mask", ["causal_targets", "full"])
def test_func_beside_rab_over_delta_q_and_paged_keys(d, mask):
    """GPU case 3: rab by absolute positions, func by query token.  (a) contiguous delta-q keys: equal to the dense statement through
    hstu_varlen_fwd_kv(rab=...); (b) the same keys from a paged cache (page size 16, permuted page ids): equal to (a)."""
    from hstu import append_kvcache, hstu_attn_varlen_func, hstu_varlen_fwd_kv

    rng = _rng("delta_q", d, mask)
    B, P = 4, 16
    new_hist = rng.integers(1, 60, B)
    num_cand = rng.integers(1, 7, B)
    old = rng.integers(0, 100, B)
    old[1] = 0
    qlen, cachelen = new_hist + num_cand, old + new_hist
    klen = cachelen + num_cand
    q_off = np.concatenate([[0], np.cumsum(qlen)]).astype(np.int32)
    k_off = np.concatenate([[0], np.cumsum(klen)]).astype(np.int32)
    T, Nk = int(q_off[-1]), int(klen.max())
    mk = lambda *shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(DEV).bfloat16()
    q, k_new, v_new = mk(T, H, d), mk(T, H, d), mk(T, H, d)
    k_old, v_old = mk(int(old.sum()), H, d), mk(int(old.sum()), H, d)
    o_off = np.concatenate([[0], np.cumsum(old)])
    kf, vf = [], []
    for b in range(B):
        kf += [k_old[o_off[b]:o_off[b + 1]], k_new[q_off[b]:q_off[b + 1]]]
        vf += [v_old[o_off[b]:o_off[b + 1]], v_new[q_off[b]:q_off[b + 1]]]
    k_full, v_full = torch.cat(kf), torch.cat(vf)
    rab = (mk(B, H if d == 64 else 1, Nk, Nk) * 2)
    qpos = np.concatenate([klen[b] - qlen[b] + np.arange(qlen[b]) for b in range(B)])     # absolute positions of the query tokens
    func = torch.from_numpy(make_func(rng, qpos, 1 if d == 64 else H, 5, slack=8, far=75)).to(DEV)
    alpha, scaling = 1.0 / d ** 0.5, 100.0
    cuq, cuk = torch.from_numpy(q_off).to(DEV), torch.from_numpy(k_off).to(DEV)
    window, tgt, causal = ((-1, 0), _ti(num_cand), True) if mask == "causal_targets" else ((-1, -1), None, False)
    with torch.no_grad():
        out_a = hstu_attn_varlen_func(q, k_full, v_full, cuq, cuk, None, None, int(qlen.max()), Nk, scaling, None, tgt,
                                      window_size=window, alpha=alpha, rab=rab, func=func)
        c = Case()
        c.func, c.tdt = func, torch.bfloat16
        dense = hstu_varlen_fwd_kv(q, k_full, v_full, cuq, cuk, int(qlen.max()), scaling, None, tgt, 1, causal, alpha,
                                   rab=_dense_rab(c, rab, cuq, cuk, Nk), max_seqlen_k=Nk)
        plain = hstu_varlen_fwd_kv(q, k_full, v_full, cuq, cuk, int(qlen.max()), scaling, None, tgt, 1, causal, alpha, rab=rab, max_seqlen_k=Nk)
    assert torch.equal(out_a, dense), f"{int((out_a != dense).sum())} elements differ from the dense statement"
    assert not torch.equal(out_a, plain) and float(out_a.float().abs().sum()) > 0      # (the functions do mask something here)
    if mask == "full":
        return      # (the paged walk below serves candidates from k_new: as in the causal_targets case)
    npages = int(((cachelen + P - 1) // P).sum())
    cache = torch.zeros(npages + 1, 2, P, H, d, dtype=torch.bfloat16, device=DEV)
    perm = rng.permutation(npages + 1)[:npages]
    page_ids, page_off, last, cursor = [], [0], [], 0
    for b in range(B):
        n = int((cachelen[b] + P - 1) // P)
        pages = perm[cursor:cursor + n]
        cursor += n
        page_ids += pages.tolist()
        page_off.append(len(page_ids))
        last.append(int(cachelen[b] - (n - 1) * P))
        for j in range(int(old[b])):
            cache[pages[j // P], 0, j % P] = k_old[o_off[b] + j]
            cache[pages[j // P], 1, j % P] = v_old[o_off[b] + j]
    append_kvcache(k_new, v_new, _ti(np.repeat(np.arange(B), new_hist)), _ti(np.concatenate([old[b] + np.arange(new_hist[b]) for b in range(B)])),
                   _ti(np.concatenate([[0], np.cumsum(num_cand)])), _ti([int(new_hist.sum())]), 0, cache, _ti(page_ids), _ti(page_off), _ti(last), 0)
    with torch.no_grad():
        out_b = hstu_attn_varlen_func(q, k_new, v_new, cuq, cuk, None, None, int(qlen.max()), Nk, scaling, None, tgt,
                                      window_size=window, alpha=alpha, rab=rab, func=func, kv_cache=cache, page_offsets=_ti(page_off),
                                      page_ids=_ti(page_ids), last_page_lens=_ti(last))
    assert torch.equal(out_a, out_b)


def test_func_beside_rab_over_delta_q_keys_stays_forward_only():
    from hstu import hstu_attn_varlen_func

    rng = _rng("delta_q_forward_only")
    mk = lambda *shape: torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(DEV).bfloat16()
    q, k, v, rab = mk(8, H, 32).requires_grad_(True), mk(20, H, 32), mk(20, H, 32), mk(1, H, 20, 20)
    func = torch.full((1, 1, 8), 20, dtype=torch.int32, device=DEV)
    with pytest.raises(NotImplementedError, match="forward only"):
        hstu_attn_varlen_func(q, k, v, _ti([0, 8]), _ti([0, 20]), None, None, 8, 20, 20, None, None, window_size=(-1, 0), alpha=0.1,
                              rab=rab, func=func)


PACKED_CASES = [("causal", 64, 3, H, H, "bf16"), ("ctx_g2", 256, 7, H, H, "bf16"), ("ctx_g1", 64, 7, 1, H, "bf16")]


@pytest.mark.parametrize("case", PACKED_CASES, ids=_ids)
def test_func_beside_rab_through_the_packed_entry_point(case):
    """GPU case 4a: one packed gradient, written strided in place; results equal to hstu_attn_varlen_func's"""
    from hstu import hstu_attn_qkvpacked_func

    c = _case(case)
    qkv = torch.stack([c.q, c.k, c.v], 1).requires_grad_(True)
    rr = c.rab.clone().requires_grad_(True)
    out = hstu_attn_qkvpacked_func(qkv, c.cu, c.cu, c.N, c.N, c.nc, c.nt, c.grp, c.window, c.alpha, rr, True, c.func)
    out.backward(c.dout)
    want = _varlen(case)
    assert tuple(qkv.grad.shape) == tuple(qkv.shape)
    for name, a_, b_ in zip(("out", "dq", "dk", "dv", "drab"), (out.detach(), *qkv.grad.unbind(1), rr.grad), want):
        assert torch.equal(a_, b_), name


@pytest.mark.parametrize("case", PACKED_CASES, ids=_ids)
def test_func_beside_rab_through_the_raw_fbgemm_ops(case):
    """GPU cases 4b and 5: hstu_varlen_fwd_80 / bwd_80, the contexts case included; the forward hands rab back; with one shared
    bias head under per-head functions drab has one head, the sum over the heads"""
    import hstu.hstu_ops_gpu  # noqa: F401  (registers torch.ops.fbgemm.hstu_varlen_*)

    c = _case(case)
    wl, wr = c.window
    out, rab_back = torch.ops.fbgemm.hstu_varlen_fwd_80(c.q, c.k, c.v, c.cu, c.cu, None, None, c.N, c.N, float(c.N), c.nc, c.nt, c.grp,
                                                        wl, wr, c.alpha, c.rab, c.func)
    assert rab_back is not None and rab_back.data_ptr() == c.rab.data_ptr()
    got = torch.ops.fbgemm.hstu_varlen_bwd_80(c.dout, c.q, c.k, c.v, c.cu, c.cu, None, None, c.N, c.N, float(c.N), None, None, None,
                                              c.nc, c.nt, c.grp, wl, wr, c.alpha, c.rab, True, c.func, False)
    for name, a_, b_ in zip(("out", "dq", "dk", "dv", "drab"), (out, *got), _varlen(case)):
        assert torch.equal(a_, b_), name
    if c.rab.shape[1] == 1:
        assert tuple(got[3].shape) == (c.B, 1, c.N, c.N)
        _close_elementwise(got[3], c.drab, c.mag_drab, 4, bits=c.bits)     # (the oracle sums over the heads for a shared bias head)
    nodrab = torch.ops.fbgemm.hstu_varlen_bwd_80(c.dout, c.q, c.k, c.v, c.cu, c.cu, None, None, c.N, c.N, float(c.N), None, None, None,
                                                 c.nc, c.nt, c.grp, wl, wr, c.alpha, c.rab, False, c.func, False)
    assert nodrab[3] is None and all(torch.equal(a_, b_) for a_, b_ in zip(nodrab[:3], got[:3]))


def test_func_beside_rab_allocates_nothing_quadratic():
    """GPU case 6.  B = 2, N = 1024, H = 2, d = 64, bf16: the mask bias of the dense statement alone is B H N^2 2 B = 8 MiB (and its
    sum with rab another 8 MiB); the in-kernel path may rise by less than 4 MiB above the inputs, the outputs, the gradients and drab"""
    from hstu import hstu_attn_varlen_func

    rng = _rng("memory")
    B, N, d = 2, 1024, 64
    T = B * N
    mk = lambda lo, hi, *shape: torch.from_numpy(rng.uniform(lo, hi, shape).astype(np.float32)).to(DEV).bfloat16()
    q, k, v, dout, rab = mk(-1, 1, T, H, d), mk(-1, 1, T, H, d), mk(-1, 1, T, H, d), mk(0, 1, T, H, d), mk(-2, 2, B, H, N, N)
    pos = np.tile(np.arange(N), B)
    func = torch.from_numpy(make_func(rng, pos, H, 5, slack=0, far=600)).to(DEV)
    cu = _ti([0, N, 2 * N])

    def step():
        qq, kk, vv, rr = (t.detach().requires_grad_(True) for t in (q, k, v, rab))
        out = hstu_attn_varlen_func(qq, kk, vv, cu, cu, None, None, N, N, N, None, None, window_size=(-1, 0), alpha=0.125, rab=rr,
                                    has_drab=True, func=func)
        out.backward(dout)
        return out, qq.grad, kk.grad, vv.grad, rr.grad

    step()                                   # warm-up: module loads, the library's one-time allocations
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = step()
    torch.cuda.synchronize()
    results = sum(t.numel() * t.element_size() for t in res)
    rise = torch.cuda.max_memory_allocated() - base - results
    print(f"peak above inputs + results: {rise / MiB:.2f} MiB (results {results / MiB:.2f} MiB)")
    assert B * H * N * N * 2 == 8 * MiB and tuple(res[4].shape) == (B, H, N, N)
    assert rise < 4 * MiB, f"{rise / MiB:.2f} MiB above the inputs, outputs, gradients and drab"
    assert float(res[0].detach().float().abs().sum()) > 0 and float(res[4].float().abs().sum()) > 0


def test_the_dense_switch_takes_the_dense_path_and_gives_the_same_results(monkeypatch):
    """GPU case 7: MI355_HSTU_FUNC_DENSE (the module attribute it sets) keeps the dense-bias statement as the A/B switch"""
    import hstu.hstu_attn_interface as hi
    from hstu import hstu_attn_varlen_func

    case = ("full", 64, 5, H, H, "bf16")
    c = _case(case)
    want = _varlen(case)
    calls = []
    real = hi.func_mask_bias
    monkeypatch.setattr(hi, "func_mask_bias", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    qq, kk, vv, rr = _grad_inputs(c)
    kw = dict(target_group_size=1, window_size=c.window, alpha=c.alpha, rab=rr, has_drab=True, func=c.func)
    hstu_attn_varlen_func(qq, kk, vv, c.cu, c.cu, None, None, c.N, c.N, c.N, None, None, **kw)
    assert not calls, "the default path built a dense mask bias"
    monkeypatch.setattr(hi, "_FUNC_DENSE", True)
    out = hstu_attn_varlen_func(qq, kk, vv, c.cu, c.cu, None, None, c.N, c.N, c.N, None, None, **kw)
    out.backward(c.dout)
    assert calls, "the switch did not take the dense path"
    for name, a_, b_ in zip(("out", "dq", "dk", "dv", "drab"), (out.detach(), qq.grad, kk.grad, vv.grad, rr.grad), want):
        assert torch.equal(a_, b_), name
