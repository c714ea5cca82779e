"""Float64 twin of the softmax attention backward (softmax_attn.py / csrc/softmax_attn_bwd.hip): dq, dk, dv in the kernel's
layouts, each with the bound its elements are judged under, and the cases of the backward tests.

Statement.  The forward and its mask are those of tests/prefill_attn_twin.py.  With p_ij the float64 probabilities of row i of
query head h (kv head h // G), dO the gradient of out,
    dP_ij = dO_i . v_j,   delta_i = sum_j p_ij dP_ij (= dO_i . out_i),   dS_ij = p_ij (dP_ij - delta_i),
    dq_i = scale sum_j dS_ij k_j,   dk_j = scale sum_{h in group, i} dS_ij q_i,   dv_j = sum_{h in group, i} p_ij dO_i.
Dense: dq [B, Sq, Hq, D], dk / dv [B, Sk, Hkv, D].  Jagged: dq [total_q, Hq, D], dk / dv [total_k, Hkv, D].  A row that sees no
key has dq = 0, a key that no query sees has dk = dv = 0.

The bound (derived, not tuned).  u is the unit roundoff of the operand type (UNIT_ROUNDOFF), eps = 2^-24 the one of fp32, n_i
the number of visible keys of a row, T = ceil(Lk / 64), a_max = max over the visible j of scale sum_d |q_d| |k_jd|, N_j the
number of (head of the group, query) pairs that see key j, bound_out the bound of the forward twin.  The kernel recomputes
P~ = exp2(scale log2e s~ - lse~ log2e) from the STORED lse, takes delta~ in fp32 from the STORED out, forms dS~ = P~ (dP~ -
delta~), rounds P~ once to the operand type for the dV product and dS~ once for the dQ / dK products, accumulates in fp32 and
rounds each gradient once.

  * the score: as in the forward twin, an fp32 dot product over D of exact products, the scale, one subtraction, and exp2 good
    to 2 ulp:   e_s = (D + 2) eps a_max + 2^-22.
  * the recomputed probability, relative.  The stored lse is the forward kernel's: its own score error moves numerator and
    denominator of p alike (2 e_s in all, with the recomputed score's), the sum l behind it was accumulated in fp32 over n_i keys
    and rescaled at most T times ((n_i + T) eps), log, the conversion ln -> log2 and its product, and the fp32 rounding of the
    stored value (4 more eps relative to l), the two products by log2 e and the subtraction s - lse, roundings of numbers as
    large as a_max + |lse| that enter the exponent absolutely (4 eps (a_max + |lse|)), and the exp2 itself (2^-22):
        e_p = 2 e_s + (n_i + T + 4) eps + 4 eps (a_max + |lse_i|) + 2^-22.
  * delta is taken from the stored out, which lies within bound_out of the true one, in an fp32 sum over D:
        e_delta_i = sum_d |dO_id| bound_out_id + D eps sum_d |dO_id| |o_id|.
  * dS: the relative error of P~ and the two fp32 roundings of the subtraction and the product act on p |dP - delta|; dP~ is an
    fp32 sum over D of exact products (D eps sum_d |dO_id| |v_jd|) and delta~ is off by e_delta, both multiplied by p; then dS~ is
    rounded once to the operand type (a kernel that folds the scale in before this rounding is covered by the same term):
        e_dS_ij = p_ij [(e_p + 2 eps) |dP_ij - delta_i| + D eps sum_d |dO_id| |v_jd| + e_delta_i] + u |dS_ij|.
  * dq: the errors of its summands, the fp32 accumulation over the n_i visible keys plus the scale and one more rounding
    ((n_i + 2) eps of the sum of magnitudes), and the output rounding:
        bound_dq_id = scale sum_j e_dS_ij |k_jd| + (n_i + 2) eps scale sum_j |dS_ij| |k_jd| + u |dq_id|.
  * dk, the same over the N_j pairs that see the key:
        bound_dk_jd = scale sum_{h,i} e_dS_ij |q_id| + (N_j + 2) eps scale sum_{h,i} |dS_ij| |q_id| + u |dk_jd|.
  * dv: P~ is off by e_p relative and rounded once to the operand type (u), the products with dO are exact, N_j fp32 additions:
        bound_dv_jd = sum_{h,i} p_ij (u + e_p) |dO_id| + N_j eps sum_{h,i} p_ij |dO_id| + u |dv_jd|.

An element whose bound is 0 (a key nobody sees, a row that sees nothing) must be exactly 0 (compare_grads()).
"""
import math
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from prefill_attn_cases import CASES, Case, make_inputs  # noqa: E402,F401
from prefill_attn_twin import KEY_TILE, UNIT_ROUNDOFF, prefill_attn_twin, sequences, visible_mask  # noqa: E402

EPS = 2.0 ** -24

# the edges of the key-owning pass: few queries over three key workgroup tiles with a ragged last one; an MQA group of 4 over
# keys that cross two workgroup tiles; sequences with keys and no queries, and with more queries than keys
EXTRA_CASES = [
    Case("bwd_none_5x257", mask="none", Sq=5, Sk=257),
    Case("bwd_causal_130x259_mqa", Sq=130, Sk=259, Hq=4, Hkv=1),
    Case("bwd_jagged_causal_edges", form="jagged", lens_q=(0, 3, 130), lens_k=(70, 129, 1)),
]
BWD_CASES = list(CASES) + EXTRA_CASES
BWD_CASE_BY_NAME = {c.name: c for c in BWD_CASES}


def make_dout(case, inp):
    """the gradient of out: randn of the shape and dtype of q, seeded by crc32(name + "/do")"""
    g = torch.Generator().manual_seed(zlib.crc32((case.name + "/do").encode()) & 0x7fffffff)
    return torch.randn(*inp["q"].shape, generator=g).to(inp["q"].dtype)


def softmax_attn_bwd_twin(q, k, v, dout, causal=False, func=None, cu_seqlens_q=None, cu_seqlens_k=None, softmax_scale=None,
                          unit_roundoff=None):
    """-> dq, dk, dv, bound_dq, bound_dk, bound_dv: float64 on the CPU, in the layouts of the kernel"""
    assert func is None or (not causal and cu_seqlens_q is None)
    jagged = cu_seqlens_q is not None
    Hq, D, Hkv = q.shape[-2], q.shape[-1], k.shape[-2]
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D) if softmax_scale is None else softmax_scale
    u = UNIT_ROUNDOFF[q.dtype] if unit_roundoff is None else unit_roundoff
    f64 = lambda t: t.detach().to("cpu").double()   # noqa: E731
    q64, k64, v64, do64 = f64(q), f64(k), f64(v), f64(dout)
    o64, lse64, bo64, _ = prefill_attn_twin(q, k, v, causal=causal, func=func, cu_seqlens_q=cu_seqlens_q,
                                            cu_seqlens_k=cu_seqlens_k, softmax_scale=softmax_scale, unit_roundoff=unit_roundoff)
    hk_of = torch.arange(Hq) // G
    dq, dk, dv = torch.zeros_like(q64), torch.zeros_like(k64), torch.zeros_like(v64)
    b_dq, b_dk, b_dv = torch.zeros_like(q64), torch.zeros_like(k64), torch.zeros_like(v64)
    group = lambda t, Lk: t.reshape(Lk, Hkv, G, D).sum(2)   # noqa: E731  ([Lk, Hq, D] -> [Lk, Hkv, D])
    zero = torch.zeros((), dtype=torch.float64)
    for b, q0, Lq, k0, Lk in sequences(q, k, cu_seqlens_q, cu_seqlens_k):
        if Lq == 0 or Lk == 0:
            continue
        qs, ks = (slice(q0, q0 + Lq), slice(k0, k0 + Lk)) if jagged else (b, b)
        qb, dob, ob, bob = q64[qs], do64[qs], o64[qs], bo64[qs]                      # [Lq, Hq, D]
        kb, vb = k64[ks][:, hk_of], v64[ks][:, hk_of]                               # [Lk, Hq, D]
        ls = (lse64[:, q0:q0 + Lq] if jagged else lse64[b])                         # [Hq, Lq]
        if func is not None:
            fh = func.shape[1]
            vis = torch.stack([visible_mask(Lq, Lk, func_rows=func[b, h if fh > 1 else 0].cpu()) for h in range(Hq)])
        else:
            vis = visible_mask(Lq, Lk, causal=causal)[None].expand(Hq, Lq, Lk)
        has = torch.isfinite(ls)
        s = torch.einsum("ihd,jhd->hij", qb, kb) * scale
        a = torch.einsum("ihd,jhd->hij", qb.abs(), kb.abs()) * scale
        p = torch.where(vis & has[..., None], torch.exp(s - torch.where(has, ls, zero)[..., None]), zero)   # [Hq, Lq, Lk]
        dP = torch.einsum("ihd,jhd->hij", dob, vb)
        delta = (p * dP).sum(-1)                                                    # [Hq, Lq]
        dS = p * (dP - delta[..., None])
        dq_b = torch.einsum("hij,jhd->ihd", dS, kb) * scale
        dk_b = group(torch.einsum("hij,ihd->jhd", dS, qb) * scale, Lk)
        dv_b = group(torch.einsum("hij,ihd->jhd", p, dob), Lk)

        n = vis.sum(-1).double()                                                    # [Hq, Lq]
        Nj = vis.sum(1).double().t().reshape(Lk, Hkv, G).sum(2)[..., None]          # [Lk, Hkv, 1]
        T = -(-Lk // KEY_TILE)
        a_max = torch.where(vis, a, zero).max(-1).values
        e_s = (D + 2) * EPS * a_max + 2.0 ** -22
        e_p = torch.where(has, 2 * e_s + (n + T + 4) * EPS + 4 * EPS * (a_max + torch.where(has, ls, zero).abs()) + 2.0 ** -22, zero)
        e_delta = (dob.abs() * bob).sum(-1).t() + D * EPS * (dob.abs() * ob.abs()).sum(-1).t()   # [Hq, Lq]
        dov = torch.einsum("ihd,jhd->hij", dob.abs(), vb.abs())
        e_dS = p * ((e_p[..., None] + 2 * EPS) * (dP - delta[..., None]).abs() + D * EPS * dov + e_delta[..., None]) + u * dS.abs()
        bq = (scale * torch.einsum("hij,jhd->ihd", e_dS, kb.abs())
              + ((n + 2) * EPS).t()[..., None] * scale * torch.einsum("hij,jhd->ihd", dS.abs(), kb.abs()) + u * dq_b.abs())
        bk = (scale * group(torch.einsum("hij,ihd->jhd", e_dS, qb.abs()), Lk)
              + (Nj + 2) * EPS * scale * group(torch.einsum("hij,ihd->jhd", dS.abs(), qb.abs()), Lk) + u * dk_b.abs())
        bv = (group(torch.einsum("hij,ihd->jhd", p * (u + e_p[..., None]), dob.abs()), Lk)
              + Nj * EPS * group(torch.einsum("hij,ihd->jhd", p, dob.abs()), Lk) + u * dv_b.abs())
        dq[qs], b_dq[qs] = dq_b, bq
        dk[ks], b_dk[ks] = dk_b, bk
        dv[ks], b_dv[ks] = dv_b, bv
    return dq, dk, dv, b_dq, b_dk, b_dv


def twin_of(case, inp, dout):
    return softmax_attn_bwd_twin(inp["q"], inp["k"], inp["v"], dout, causal=inp["causal"], func=inp["func"],
                                 cu_seqlens_q=inp["cu_seqlens_q"], cu_seqlens_k=inp["cu_seqlens_k"])


def compare_grads(grads, twin):
    """worst |err| / bound of (dq, dk, dv) against a twin result; an element whose bound is 0 must be exactly 0 (else inf), a
    NaN is inf"""
    ratios = []
    for got, want, bound in zip(grads, twin[:3], twin[3:]):
        got = got.detach().to("cpu").double()
        assert got.shape == want.shape, (got.shape, want.shape)
        err = (got - want).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bound)               # 0 / 0 is a match, x / 0 is inf
        r = torch.nan_to_num(r, nan=math.inf)
        ratios.append(float(r.max()) if r.numel() else 0.0)
    return tuple(ratios)
