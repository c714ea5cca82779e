"""The shapes of the beam-decode GPU test (tests/test_beam_decode_gpu.py), their inputs, and a torch-on-CPU emulation of the
kernel's arithmetic (tests/test_beam_decode_cpu.py checks on these same shapes that the twin's bound can be met by that
arithmetic and that it catches mistakes).  The shapes are the smallest at which the kernels can go wrong: the context kernel
packs W G query rows per kv head into wave tiles of 32 and workgroup tiles of 128 rows, and walks keys in tiles of 64."""
import math
import zlib
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

KEY_TILE = 64


@dataclass(frozen=True)
class Case:
    name: str
    B: int = 2
    W: int = 5
    Hq: int = 4
    Hkv: int = 2
    D: int = 64
    ctx: int = 70
    dn: int = 2
    dtype: str = "bf16"
    form: str = "dense"            # dense | seqused | jagged | strided
    lens: Tuple[int, ...] = ()     # seqused values / jagged lengths (B = len(lens))
    idx64: bool = False
    idx: str = ""                  # "" | repeat | oob
    q_scale: float = 1.0
    spike: str = ""                # "" | late (largest score in the last key tile) | beam (in the beam keys)
    splits: Tuple[int, ...] = (1,)

    @property
    def torch_dtype(self):
        return torch.bfloat16 if self.dtype == "bf16" else torch.float16

    @property
    def batch(self):
        return len(self.lens) if self.lens else self.B


def _cases():
    c = []
    for W in (1, 31, 32, 33, 129):                       # packed rows W G cross one wave tile (32) and one workgroup tile (128)
        for G in (1, 2, 4):
            c.append(Case(f"qtile_W{W}_G{G}", B=1, W=W, Hkv=4 // G, ctx=70, dn=2))
    for ctx in (0, 1, 63, 64, 65, 130):
        c.append(Case(f"ktile_ctx{ctx}", ctx=ctx, dn=1))
    c.append(Case("splits_ctx453", B=1, W=33, D=128, ctx=453, dn=3, splits=(1, 2, 3, 7)))
    for dn in (0, 1, 3, 16):
        c.append(Case(f"beam_dn{dn}_i32", ctx=37, dn=dn))
        c.append(Case(f"beam_dn{dn}_i64", ctx=37, dn=dn, idx64=True))
    c.append(Case("beam_repeat", ctx=37, dn=3, idx="repeat"))
    c.append(Case("beam_oob_i32", ctx=37, dn=3, idx="oob"))
    c.append(Case("beam_oob_i64", ctx=37, dn=3, idx="oob", idx64=True))
    c.append(Case("beam_only", ctx=0, dn=3))
    c.append(Case("ctx_only", ctx=37, dn=0))
    c.append(Case("no_keys", ctx=0, dn=0))
    c.append(Case("seqused", ctx=130, lens=(0, 37, 130), dn=2, form="seqused", splits=(1, 3)))
    c.append(Case("jagged", lens=(0, 1, 64, 130), dn=2, form="jagged", splits=(1, 3)))
    c.append(Case("strided", ctx=70, dn=2, form="strided", splits=(1, 2)))
    c.append(Case("numerics_q8", ctx=130, dn=3, q_scale=8.0, splits=(1, 2)))
    c.append(Case("numerics_late_max", ctx=130, dn=3, spike="late", splits=(1, 2)))
    c.append(Case("numerics_beam_max", ctx=130, dn=3, spike="beam", splits=(1, 2)))
    for D in (64, 128):
        for dt in ("bf16", "fp16"):
            c.append(Case(f"dtype_{dt}_D{D}", W=33, D=D, ctx=130, dn=3, dtype=dt, splits=(1, 3)))
    c.append(Case("dtype_fp16_G4_jagged", W=9, Hkv=1, D=128, lens=(65, 3), dn=1, dtype="fp16", form="jagged"))
    return c


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


def make_inputs(case: Case):
    """CPU tensors of a case, from a generator seeded by the case's name.  Returns a dict with the positional tensors and
    the seqused_k / cu_seqlens_k keywords."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) & 0x7fffffff)
    dt = case.torch_dtype
    B, W, Hq, Hkv, D, dn = case.batch, case.W, case.Hq, case.Hkv, case.D, case.dn
    G = Hq // Hkv
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    q = (r(B, 1, W, Hq, D) * case.q_scale).to(dt)
    seqused = cu = None
    if case.form == "jagged":
        total = sum(case.lens)
        kc, vc = r(total, Hkv, D).to(dt), r(total, Hkv, D).to(dt)
        cu = torch.tensor([0] + list(torch.tensor(case.lens).cumsum(0)), dtype=torch.int32)
    elif case.form == "strided":   # the layer-select view of a [B, Sk, layers, Hkv, D] cache
        kv = r(2, B, case.ctx, 3, Hkv, D).to(dt)
        kc, vc = kv[0][:, :, 1], kv[1][:, :, 1]
    else:
        kc, vc = r(B, case.ctx, Hkv, D).to(dt), r(B, case.ctx, Hkv, D).to(dt)
        if case.form == "seqused":
            seqused = torch.tensor(case.lens, dtype=torch.int32)
    kb, vb = r(B, dn * W, Hkv, D).to(dt), r(B, dn * W, Hkv, D).to(dt)
    max_dn = dn + 2
    tk = torch.randint(0, max(dn * W, 1), (B, 1, Hkv, max_dn, W), generator=g)
    if dn > 0 and case.idx == "repeat":
        tk[:, :, :, 1] = tk[:, :, :, 0]
    if dn > 0 and case.idx == "oob":
        tk[:, :, :, 0, ::2] = -1
        tk[:, :, :, 1, 1::2] = dn * W
    tk[:, :, :, dn:] = 2 ** 30          # the unused tail of the index list is never read
    topk = tk.repeat_interleave(G, dim=2).to(torch.int64 if case.idx64 else torch.int32)
    if case.spike:   # row (b = last, w = 0, h = 0): one key aligned with q, so that its score is the row's largest by far
        b = B - 1
        qv = q[b, 0, 0, 0].float()
        kv_ = (qv * (6.0 / max(float(qv.norm()), 1e-6) * math.sqrt(math.sqrt(D)))).to(dt)
        if case.spike == "late":
            kc[b, case.ctx - 1, 0] = kv_
        else:
            kb[b, int(topk[b, 0, 0, dn - 1, 0]), 0] = kv_
    return dict(q=q, k_context=kc, v_context=vc, k_beam=kb, v_beam=vb, topk_indices=topk, decode_nums=dn,
                seqused_k=seqused, cu_seqlens_k=cu)


def _ctx_rows(inp, b):
    kc, vc = inp["k_context"], inp["v_context"]
    if inp["cu_seqlens_k"] is not None:
        s, e = int(inp["cu_seqlens_k"][b]), int(inp["cu_seqlens_k"][b + 1])
        return kc[s:e], vc[s:e]
    n = kc.shape[1] if inp["seqused_k"] is None else max(0, min(int(inp["seqused_k"][b]), kc.shape[1]))
    return kc[b, :n], vc[b, :n]


def emulate(inp, num_splits=1, mistake: Optional[str] = None, key_tile: int = KEY_TILE):
    """The kernel's arithmetic in torch on the CPU: operands in their 16-bit type, fp32 scores, an online max over
    64-key tiles, P rounded to the operand type for the P V product while the row sum takes the fp32 P, fp32 accumulation,
    `num_splits` ranges of key tiles and the fp32 beam phase merged by log-sum-exp, the output rounded once.
    mistake: None | drop_top | shift_idx | wrong_head | max_merge.  -> out (operand dtype), lse (fp32)"""
    q, kb, vb, topk, dn = inp["q"], inp["k_beam"], inp["v_beam"], inp["topk_indices"].long(), inp["decode_nums"]
    dt = q.dtype
    B, _, W, Hq, D = q.shape
    Hkv = kb.shape[2]
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    hk_of = torch.arange(Hq) % Hkv if mistake == "wrong_head" else torch.arange(Hq) // G
    if mistake == "shift_idx":
        topk = topk + 1
    out = torch.zeros(B, 1, W, Hq, D, dtype=dt)
    lse = torch.full((B, 1, W, Hq), -math.inf, dtype=torch.float32)
    ninf = torch.tensor(-math.inf)
    for b in range(B):
        kc, vc = _ctx_rows(inp, b)
        n_ctx = kc.shape[0]
        kc32, vc32 = kc.float()[:, hk_of], vc.float()[:, hk_of]                  # [n, Hq, D]
        qb = q[b, 0].float()
        s_ctx = torch.einsum("whd,shd->whs", qb, kc32) * scale                   # fp32
        if dn > 0:
            idx = topk[b, 0, (torch.arange(Hq) // G) * G, :dn, :].permute(2, 0, 1)
            ok = (idx >= 0) & (idx < dn * W)
            idc = idx.clamp(0, dn * W - 1)
            h_idx = hk_of[None, :, None].expand_as(idc)
            kg, vg = kb[b].float()[idc, h_idx], vb[b].float()[idc, h_idx]
            s_beam = torch.where(ok, torch.einsum("whd,whnd->whn", qb, kg) * scale, ninf)
        else:
            s_beam = torch.zeros(W, Hq, 0)
            vg = torch.zeros(W, Hq, 0, D)
        if mistake == "drop_top":
            s_all = torch.cat([s_ctx, s_beam], -1)
            if s_all.shape[-1]:
                top = s_all.argmax(-1, keepdim=True)
                s_all = s_all.scatter(-1, top, -math.inf)
                s_ctx, s_beam = s_all[..., :n_ctx], s_all[..., n_ctx:]
        parts = []   # (lse [W, Hq], normalised O [W, Hq, D]) in fp32
        nt = -(-n_ctx // key_tile)
        for sp in range(num_splits):
            t0, t1 = sp * nt // num_splits, (sp + 1) * nt // num_splits
            if t0 >= t1:
                continue
            m = torch.full((W, Hq), -math.inf)
            l = torch.zeros(W, Hq)
            o = torch.zeros(W, Hq, D)
            for t in range(t0, t1):
                sl = slice(t * key_tile, min((t + 1) * key_tile, n_ctx))
                st = s_ctx[..., sl]
                m_new = torch.maximum(m, st.max(-1).values)
                ok_m = torch.isfinite(m_new)
                alpha = torch.where(ok_m, torch.exp(m - m_new), torch.zeros(()))
                p = torch.where(ok_m[..., None], torch.exp(st - m_new[..., None]), torch.zeros(()))
                l = l * alpha + p.sum(-1)
                o = o * alpha[..., None] + torch.einsum("whs,shd->whd", p.to(dt).float(), vc32[sl])
                m = m_new
            has = l > 0
            parts.append((torch.where(has, m + torch.log(l), ninf), torch.where(has[..., None], o / l[..., None], torch.zeros(()))))
        if dn > 0:   # the beam phase, fp32 throughout
            m = s_beam.max(-1).values
            ok_m = torch.isfinite(m)
            p = torch.where(ok_m[..., None], torch.exp(s_beam - m[..., None]), torch.zeros(()))
            l = p.sum(-1)
            o = torch.einsum("whn,whnd->whd", p, vg)
            has = l > 0
            parts.insert(0, (torch.where(has, m + torch.log(l), ninf), torch.where(has[..., None], o / l.clamp_min(1e-30)[..., None], torch.zeros(()))))
        if not parts:
            continue
        if mistake == "max_merge":
            ls = torch.stack([p_[0] for p_ in parts])                            # [P, W, Hq]
            os_ = torch.stack([p_[1] for p_ in parts])
            best = ls.argmax(0)
            lse[b, 0] = ls.gather(0, best[None])[0]
            out[b, 0] = os_.gather(0, best[None, ..., None].expand(1, W, Hq, D))[0].to(dt)
            continue
        m = torch.full((W, Hq), -math.inf)
        l = torch.zeros(W, Hq)
        acc = torch.zeros(W, Hq, D)
        for ls, o in parts:
            m_new = torch.maximum(m, ls)
            ok_m = torch.isfinite(m_new)
            alpha = torch.where(ok_m, torch.exp(m - m_new), torch.zeros(()))
            e = torch.where(ok_m, torch.exp(ls - m_new), torch.zeros(()))
            l = l * alpha + e
            acc = acc * alpha[..., None] + e[..., None] * o
            m = m_new
        has = l > 0
        out[b, 0] = torch.where(has[..., None], acc / l.clamp_min(1e-30)[..., None], torch.zeros(())).to(dt)
        lse[b, 0] = torch.where(has, m + torch.log(l.clamp_min(1e-30)), ninf)
    return out, lse
