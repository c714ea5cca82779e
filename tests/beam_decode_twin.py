"""Float64 twin of beam-search decode attention (beam_decode_attn.py / csrc/beam_decode.hip), with the bound each output
element is judged under.

Statement (single pass, the semantics of the reference's beam_attention_ref).  For batch b, beam w, query head h, kv head
h // G (G = Hq / Hkv) the key set is the Sk_b context rows of sample b followed by the beam rows
k_beam[b, topk[b, 0, (h // G) G, n, w], h // G] for n < decode_nums; an index outside [0, decode_nums W) is an absent key, a
repeated one counts twice.  scores = softmax_scale q.k, out = softmax(scores) V, lse = logsumexp(scores); a row with no key
has out = 0 and lse = -inf.  Sk_b is the allocated length, min(seqused_k[b], Sk), or cu_seqlens_k[b + 1] - cu_seqlens_k[b].

The bound (derived, not tuned).  Let p_j be the float64 probabilities of a row, A_d = sum_j p_j |v_jd|, u the unit roundoff
of the operand type as the kernel's contract states it (2^-8 bf16, 2^-11 fp16; 2^-24 when the computation under test is
fp32 throughout), n the number of keys of the row and ns the number of KV splits.  The kernel computes, per tile,
P~ = exp2(s~ - m) in fp32, sums the fp32 P~ into l, rounds P~ ONCE to the operand type for the MFMA, accumulates P~ V in
fp32, merges partials by log-sum-exp in fp32 and rounds out once.

  * rounding of P to the operand type: every p_j moves by at most u p_j, the denominator is taken from the unrounded
    values and does not move: |d out_d| <= u A_d.
  * the final rounding of out: u |out_d|.
  * fp32 accumulation over n keys and the ns + 1 rescale-and-add merges: each addition and each rescale is one fp32
    rounding of a partial sum that is bounded by A_d: (n + ns) 2^-24 A_d.
  * the score error e_s.  A score is an fp32 dot product over D of exactly representable products, times the scale:
    |d s_j| <= (D + 2) 2^-24 softmax_scale sum_d |q_d| |k_jd| (D - 1 additions, the scale, the subtraction of the max),
    and exp2 on the result is good to 2 ulp: + 2^-22.  e_s is the largest of these over the keys of the row.  A score
    error d s_j multiplies p_j by exp(d s_j); numerator and denominator both move, so to first order
    |d out_d| <= 2 e_s A_d.
  * lse: the reference's own rule (corelib/gr_decode_atten/README.md, "Tolerance") is an absolute 1e-3; the score error
    shifts lse by at most e_s: 1e-3 + e_s.

bound_out = u A + u |out| + (n + ns) 2^-24 A + 2 e_s A;  bound_lse = 1e-3 + e_s.  A row without keys has bound 0 on out:
it must be exactly 0, and its lse must be exactly -inf (compare()).
"""
import math

import torch

UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -24}


def context_lengths(B, k_context, seqused_k=None, cu_seqlens_k=None):
    """(first row, length) of every sample's context; for a dense context the first row is 0"""
    if cu_seqlens_k is not None:
        cu = [int(x) for x in cu_seqlens_k.tolist()]
        return [(cu[b], cu[b + 1] - cu[b]) for b in range(B)]
    Sk = k_context.shape[1]
    if seqused_k is not None:
        return [(0, max(0, min(int(x), Sk))) for x in seqused_k.tolist()]
    return [(0, Sk)] * B


def beam_decode_twin(q, k_context, v_context, k_beam, v_beam, topk_indices, decode_nums, softmax_scale=None,
                     seqused_k=None, cu_seqlens_k=None, unit_roundoff=None, num_splits=1):
    """-> out [B, 1, W, Hq, D] f64, lse [B, 1, W, Hq] f64, bound_out (as out), bound_lse (as lse); all on the CPU"""
    assert seqused_k is None or cu_seqlens_k is None
    B, Sq, W, Hq, D = q.shape
    assert Sq == 1
    jagged = cu_seqlens_k is not None
    Hkv = k_context.shape[1] if jagged else k_context.shape[2]
    G = Hq // Hkv
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    u = UNIT_ROUNDOFF[q.dtype] if unit_roundoff is None else unit_roundoff
    f = lambda t: t.detach().to("cpu").double()
    q64, kb64, vb64 = f(q)[:, 0], f(k_beam), f(v_beam)
    kc_all, vc_all = f(k_context), f(v_context)
    topk = topk_indices.detach().to("cpu").long()
    lens = context_lengths(B, k_context, None if seqused_k is None else seqused_k.cpu(),
                           None if cu_seqlens_k is None else cu_seqlens_k.cpu())
    out = torch.zeros(B, 1, W, Hq, D, dtype=torch.float64)
    lse = torch.full((B, 1, W, Hq), -math.inf, dtype=torch.float64)
    b_out = torch.zeros_like(out)
    b_lse = torch.zeros_like(lse)
    hk_of = torch.arange(Hq) // G
    for b in range(B):
        r0, n_ctx = lens[b]
        kc = (kc_all[r0:r0 + n_ctx] if jagged else kc_all[b, :n_ctx])[:, hk_of]   # [n_ctx, Hq, D]
        vc = (vc_all[r0:r0 + n_ctx] if jagged else vc_all[b, :n_ctx])[:, hk_of]
        qb = q64[b]                                                              # [W, Hq, D]
        s_ctx = torch.einsum("whd,shd->whs", qb, kc) * softmax_scale
        a_ctx = torch.einsum("whd,shd->whs", qb.abs(), kc.abs()) * softmax_scale
        if decode_nums > 0:
            idx = topk[b, 0, (hk_of * G), :decode_nums, :].permute(2, 0, 1)      # [W, Hq, dn]
            ok = (idx >= 0) & (idx < decode_nums * W)
            idc = idx.clamp(0, max(decode_nums * W - 1, 0))
            h_idx = hk_of[None, :, None].expand_as(idc)
            kg, vg = kb64[b][idc, h_idx], vb64[b][idc, h_idx]                    # [W, Hq, dn, D]
            s_beam = torch.einsum("whd,whnd->whn", qb, kg) * softmax_scale
            a_beam = torch.einsum("whd,whnd->whn", qb.abs(), kg.abs()) * softmax_scale
            s_beam = torch.where(ok, s_beam, torch.full_like(s_beam, -math.inf))
            a_beam = torch.where(ok, a_beam, torch.zeros_like(a_beam))
        else:
            ok = torch.zeros(W, Hq, 0, dtype=torch.bool)
            s_beam = a_beam = torch.zeros(W, Hq, 0, dtype=torch.float64)
            vg = torch.zeros(W, Hq, 0, D, dtype=torch.float64)
        s = torch.cat([s_ctx, s_beam], dim=-1)
        n_keys = n_ctx + ok.sum(-1)                                              # [W, Hq]
        has = n_keys > 0
        m = torch.where(has, s.max(-1).values if s.shape[-1] else torch.zeros(W, Hq, dtype=torch.float64), torch.zeros(()).double())
        e = torch.exp(s - m[..., None])
        l = e.sum(-1)
        p = torch.where(has[..., None], e / l.clamp_min(1e-300)[..., None], torch.zeros_like(e))
        p_ctx, p_beam = p[..., :n_ctx], p[..., n_ctx:]
        o = torch.einsum("whs,shd->whd", p_ctx, vc) + torch.einsum("whn,whnd->whd", p_beam, vg)
        A = torch.einsum("whs,shd->whd", p_ctx, vc.abs()) + torch.einsum("whn,whnd->whd", p_beam, vg.abs())
        a_max = torch.cat([a_ctx, a_beam], dim=-1)
        a_max = a_max.max(-1).values if a_max.shape[-1] else torch.zeros(W, Hq, dtype=torch.float64)
        e_s = (D + 2) * 2.0 ** -24 * a_max + 2.0 ** -22
        out[b, 0] = o
        lse[b, 0] = torch.where(has, m + torch.log(l.clamp_min(1e-300)), torch.full_like(m, -math.inf))
        b_out[b, 0] = u * A + u * o.abs() + ((n_keys + num_splits).double() * 2.0 ** -24)[..., None] * A \
            + 2 * e_s[..., None] * A
        b_lse[b, 0] = 1e-3 + e_s
    return out, lse, b_out, b_lse


def compare(out, lse, twin):
    """worst |err| / bound of out and of lse against a twin result; rows without keys must be exactly 0 / -inf (else inf)"""
    t_out, t_lse, b_out, b_lse = twin
    out, lse = out.detach().to("cpu").double(), lse.detach().to("cpu").double()
    assert out.shape == t_out.shape and lse.shape == t_lse.shape, (out.shape, t_out.shape, lse.shape, t_lse.shape)
    err = (out - t_out).abs()
    r_out = torch.where(err == 0, torch.zeros_like(err), err / b_out)            # 0 / 0 is a match, x / 0 is inf
    r_out = torch.nan_to_num(r_out, nan=math.inf)
    empty = torch.isinf(t_lse)
    lerr = torch.where(empty, torch.where(lse == t_lse, 0.0, math.inf), (lse - t_lse).abs() / b_lse)
    lerr = torch.nan_to_num(lerr, nan=math.inf)
    return (float(r_out.max()) if r_out.numel() else 0.0), (float(lerr.max()) if lerr.numel() else 0.0)
