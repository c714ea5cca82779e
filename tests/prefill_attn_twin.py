"""Float64 twin of softmax prefill attention (prefill_attn.py / csrc/prefill_attn.hip), with the bound each output element is
judged under.

Statement.  For sequence b with Lq queries and Lk keys, query head h and kv head h // G (G = Hq / Hkv), query i sees key j iff
  none:    always;
  causal:  j <= i + Lk - Lq                    (bottom-right aligned; a row with i + Lk - Lq < 0 sees nothing);
  func:    j < F[0][i], or F[2p-1][i] <= j < F[2p][i] for some p >= 1, F = func[b, h or 0], interval ends clamped to [0, Lk]
           (oracle/hstu_oracle.py:func_mask; columns of func at or past Lq are not rows of anything and are never read).
scores = softmax_scale q.k over the visible keys, out = softmax(scores) V, lse = logsumexp(scores) in natural-log units; a row
with no visible key has out = 0 and lse = -inf.  Dense: q [B, Sq, Hq, D], k / v [B, Sk, Hkv, D] -> out [B, Sq, Hq, D], lse
[B, Hq, Sq].  Jagged: q [total_q, Hq, D], k / v [total_k, Hkv, D] with cu_seqlens -> out [total_q, Hq, D], lse [Hq, total_q].

The bound (derived, not tuned; the derivation of tests/beam_decode_twin.py with ns = 0, restated for this kernel).  Let p_j be
the float64 probabilities of a row, A_d = sum_j p_j |v_jd|, u the unit roundoff of the operand type as the kernel's contract
states it (2^-8 bf16, 2^-11 fp16; 2^-24 when the computation under test is fp32 throughout), n the number of visible keys of
the row and T = ceil(Lk / 64) the number of key tiles of its sequence.  Per visited tile the kernel computes
P~ = exp2(s~ - m) in fp32, adds the fp32 P~ into l, rounds P~ ONCE to the operand type for the MFMA, rescales O and l by
exp2(m_old - m_new) and accumulates P~ V in fp32; at the end it multiplies O by 1 / l and rounds out once.

  * rounding of P to the operand type: every p_j moves by at most u p_j, the denominator is taken from the unrounded values
    and does not move: |d out_d| <= u A_d.
  * the final rounding of out: u |out_d|.
  * fp32 accumulation over the n visible keys: each addition is one fp32 rounding of a partial sum bounded by A_d:
    n 2^-24 A_d.  (A masked key enters as an exact 0 and rounds nothing.)
  * the per-tile rescale, which the decode kernel's bound has as its ns + 1 merges and this kernel has once per visited tile:
    one fp32 rounding of a partial sum bounded by A_d, at most T times: T 2^-24 A_d.  The same rescale of l moves numerator
    and denominator alike and is covered by it to first order; the reciprocal and the final multiplication are two more fp32
    roundings of out itself, 2 2^-24 |out_d|, which the u |out_d| term (u >= 2^-11) is not asked to absorb: they are added.
  * the score error e_s.  A score is an fp32 dot product over D of exactly representable products, times the scale:
    |d s_j| <= (D + 2) 2^-24 softmax_scale sum_d |q_d| |k_jd| (D - 1 additions, the scale, the subtraction of the max), and
    exp2 on the result is good to 2 ulp: + 2^-22.  e_s is the largest of these over the visible keys of the row.  A score
    error d s_j multiplies p_j by exp(d s_j); numerator and denominator both move, so to first order |d out_d| <= 2 e_s A_d.
  * lse: the absolute 1e-3 that tests/beam_decode_twin.py takes from the decode kernel's documentation in the reference, plus
    the shift e_s of the scores: 1e-3 + e_s.

bound_out = u A + u |out| + (n + T) 2^-24 A + 2 2^-24 |out| + 2 e_s A;  bound_lse = 1e-3 + e_s.  A row without visible keys
has bound 0 on out: it must be exactly 0, and its lse exactly -inf (compare()).
"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from beam_decode_twin import UNIT_ROUNDOFF, compare  # noqa: E402,F401  (the same comparison rule)

KEY_TILE = 64


def visible_mask(Lq, Lk, causal=False, func_rows=None):
    """bool [Lq, Lk] (func_rows: int [n_func, >= Lq] of one batch entry and head, or None)"""
    j = torch.arange(Lk)[None, :]
    i = torch.arange(Lq)[:, None]
    if func_rows is not None:
        f = func_rows[:, :Lq].long().clamp(0, Lk)          # only the first Lq columns are rows
        m = j < f[0][:, None]
        for p in range(1, f.shape[0] // 2 + 1):
            m = m | ((f[2 * p - 1][:, None] <= j) & (j < f[2 * p][:, None]))
        return m
    if causal:
        return j <= i + (Lk - Lq)
    return torch.ones(Lq, Lk, dtype=torch.bool)


def sequences(q, k, cu_seqlens_q=None, cu_seqlens_k=None):
    """[(batch index or None, q row 0, Lq, k row 0, Lk)]"""
    if cu_seqlens_q is None:
        return [(b, 0, q.shape[1], 0, k.shape[1]) for b in range(q.shape[0])]
    cq, ck = [int(x) for x in cu_seqlens_q.tolist()], [int(x) for x in cu_seqlens_k.tolist()]
    return [(None, cq[b], cq[b + 1] - cq[b], ck[b], ck[b + 1] - ck[b]) for b in range(len(cq) - 1)]


def prefill_attn_twin(q, k, v, causal=False, func=None, cu_seqlens_q=None, cu_seqlens_k=None, softmax_scale=None,
                      unit_roundoff=None):
    """-> out, lse, bound_out, bound_lse: float64 on the CPU, in the layouts of the kernel"""
    assert func is None or (not causal and cu_seqlens_q is None)
    jagged = cu_seqlens_q is not None
    Hq, D, Hkv = q.shape[-2], q.shape[-1], k.shape[-2]
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D) if softmax_scale is None else softmax_scale
    u = UNIT_ROUNDOFF[q.dtype] if unit_roundoff is None else unit_roundoff
    f64 = lambda t: t.detach().to("cpu").double()   # noqa: E731
    q64, k64, v64 = f64(q), f64(k), f64(v)
    hk_of = torch.arange(Hq) // G
    out = torch.zeros(q.shape, dtype=torch.float64)
    if jagged:
        lse = torch.full((Hq, q.shape[0]), -math.inf, dtype=torch.float64)
    else:
        lse = torch.full((q.shape[0], Hq, q.shape[1]), -math.inf, dtype=torch.float64)
    b_out, b_lse = torch.zeros_like(out), torch.zeros_like(lse)
    for bi, (b, q0, Lq, k0, Lk) in enumerate(sequences(q, k, cu_seqlens_q, cu_seqlens_k)):
        if Lq == 0:
            continue
        qb = q64[q0:q0 + Lq] if jagged else q64[b]                                   # [Lq, Hq, D]
        kb = (k64[k0:k0 + Lk] if jagged else k64[b])[:, hk_of]                       # [Lk, Hq, D]
        vb = (v64[k0:k0 + Lk] if jagged else v64[b])[:, hk_of]
        if func is not None:
            fh = func.shape[1]
            vis = torch.stack([visible_mask(Lq, Lk, func_rows=func[b, h if fh > 1 else 0].cpu()) for h in range(Hq)])
        else:
            vis = visible_mask(Lq, Lk, causal=causal)[None].expand(Hq, Lq, Lk)
        s = torch.einsum("ihd,jhd->hij", qb, kb) * scale
        a = torch.einsum("ihd,jhd->hij", qb.abs(), kb.abs()) * scale
        n = vis.sum(-1)                                                             # [Hq, Lq]
        has = n > 0
        s = torch.where(vis, s, torch.full_like(s, -math.inf))
        m = torch.where(has, s.max(-1).values if Lk else torch.zeros(Hq, Lq, dtype=torch.float64), torch.zeros((), dtype=torch.float64))
        e = torch.exp(s - m[..., None])
        l = e.sum(-1)
        p = torch.where(has[..., None], e / l.clamp_min(1e-300)[..., None], torch.zeros_like(e))
        o = torch.einsum("hij,jhd->ihd", p, vb)                                      # [Lq, Hq, D]
        A = torch.einsum("hij,jhd->ihd", p, vb.abs())
        a_max = torch.where(vis, a, torch.zeros_like(a)).max(-1).values if Lk else torch.zeros(Hq, Lq, dtype=torch.float64)
        e_s = (D + 2) * 2.0 ** -24 * a_max + 2.0 ** -22                              # [Hq, Lq]
        T = -(-Lk // KEY_TILE)
        acc = ((n + T).double() * 2.0 ** -24).t()[..., None]                         # [Lq, Hq, 1]
        bo = u * A + u * o.abs() + acc * A + 2 * 2.0 ** -24 * o.abs() + 2 * e_s.t()[..., None] * A
        ls = torch.where(has, m + torch.log(l.clamp_min(1e-300)), torch.full_like(m, -math.inf))
        if jagged:
            out[q0:q0 + Lq], b_out[q0:q0 + Lq] = o, bo
            lse[:, q0:q0 + Lq], b_lse[:, q0:q0 + Lq] = ls, 1e-3 + e_s
        else:
            out[b], b_out[b] = o, bo
            lse[b], b_lse[b] = ls, 1e-3 + e_s
    return out, lse, b_out, b_lse
