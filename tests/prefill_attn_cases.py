"""The shapes of the prefill-attention GPU test (tests/test_prefill_attn_gpu.py), their inputs, and a torch-on-CPU emulation
of the kernel's arithmetic (tests/test_prefill_attn_cpu.py checks on these same shapes that the twin's bound can be met by that
arithmetic and that it catches mistakes).  The shapes are the smallest that cross every edge of the kernel: key tiles of 64,
workgroup tiles of 128 query rows, wave tiles of 32.  The arbitrary_func tensors are those the reference's own encoders wrote
(tests/golden/prefill_attn_golden.npz), with their 256 padding columns overwritten by a large value."""
import math
import os
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

KEY_TILE = 64
PAD_VALUE = 2 ** 30
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prefill_attn_golden.npz")


@dataclass(frozen=True)
class Case:
    name: str
    form: str = "dense"            # dense | strided (unbind(2) views of one [B, S, 3, H, D] buffer) | jagged
    mask: str = "causal"           # none | causal | func
    B: int = 2
    Sq: int = 64
    Sk: int = 0                    # 0: Sq
    Hq: int = 4
    Hkv: int = 2
    D: int = 64
    dtype: str = "bf16"
    lens_q: Tuple[int, ...] = ()   # jagged
    lens_k: Tuple[int, ...] = ()   # () : lens_q
    func: str = ""                 # jagged_causal | target_aware | random | batch2
    func_heads: int = 1
    q_scale: float = 1.0
    spike: bool = False            # the largest score of one row lies in its last key tile

    @property
    def torch_dtype(self):
        return torch.bfloat16 if self.dtype == "bf16" else torch.float16

    @property
    def sk(self):
        return self.Sk or self.Sq

    @property
    def klens(self):
        return self.lens_k or self.lens_q


def _cases():
    c = []
    combo = [(64, "bf16"), (128, "fp16"), (64, "fp16"), (128, "bf16")]
    for n, S in enumerate((1, 63, 64, 65, 129, 257)):
        D, dt = combo[n % 4]
        c.append(Case(f"causal_S{S}_D{D}_{dt}", Sq=S, D=D, dtype=dt))
    c.append(Case("causal_S257_D64_fp16", Sq=257, D=64, dtype="fp16"))
    c.append(Case("causal_mqa_S129", Sq=129, Hkv=1))
    c.append(Case("causal_mha_S65_D128", Sq=65, Hq=2, Hkv=2, D=128))
    c.append(Case("none_70x130_D64_bf16", mask="none", Sq=70, Sk=130))
    c.append(Case("none_70x130_D128_fp16", mask="none", Sq=70, Sk=130, D=128, dtype="fp16"))
    c.append(Case("causal_33x97", Sq=33, Sk=97))                                   # bottom-right aligned
    c.append(Case("causal_97x33", Sq=97, Sk=33))                                   # the first 64 rows see nothing
    c.append(Case("causal_97x33_D128_fp16", Sq=97, Sk=33, D=128, dtype="fp16"))
    c.append(Case("causal_q8_S129", Sq=129, q_scale=8.0))
    c.append(Case("causal_late_max_S257", Sq=257, spike=True))
    c.append(Case("jagged_causal_D64_bf16", form="jagged", lens_q=(0, 1, 64, 65, 200)))
    c.append(Case("jagged_causal_D128_fp16", form="jagged", lens_q=(0, 1, 64, 65, 200), D=128, dtype="fp16"))
    c.append(Case("jagged_causal_qk_differ", form="jagged", lens_q=(5, 0, 70, 130, 40, 90), lens_k=(9, 12, 0, 130, 100, 30)))
    c.append(Case("jagged_causal_first_empty", form="jagged", lens_q=(0, 70, 3), Hkv=1))
    c.append(Case("jagged_none", form="jagged", mask="none", lens_q=(3, 0, 130), lens_k=(70, 5, 1), D=128))
    c.append(Case("strided_causal_D64_bf16", form="strided", Sq=130, Hq=2, Hkv=2))
    c.append(Case("strided_none_D128_fp16", form="strided", mask="none", Sq=70, Hq=2, Hkv=2, D=128, dtype="fp16"))
    fcombo = {"jagged_causal": [(64, "bf16", 1), (128, "fp16", 4)], "target_aware": [(128, "bf16", 1), (64, "fp16", 4)],
              "random": [(64, "bf16", 1), (128, "fp16", 4), (128, "bf16", 4)]}
    for kind, lst in fcombo.items():
        for D, dt, fh in lst:
            c.append(Case(f"func_{kind}_D{D}_{dt}_fh{fh}", mask="func", B=1, Sq=300, D=D, dtype=dt, func=kind, func_heads=fh))
    c.append(Case("func_batch2_mqa", mask="func", B=2, Sq=300, Hkv=1, func="batch2", func_heads=1))
    return c


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def golden_mask(kind):
    S = int(golden()["offsets"][-1])
    return torch.from_numpy(np.unpackbits(golden()[f"{kind}_mask"], axis=-1)[:, :S].astype(bool))


def case_func(case: Case):
    """int32 [B, func_heads, n_func, Sq + 256]: the reference's tensor, padding columns filled with PAD_VALUE; with Hq heads,
    head h additionally sees the first h keys (F[0] = max(F[0], h)), so that the heads differ"""
    g = golden()
    if case.func == "batch2":
        a, b = torch.from_numpy(g["jagged_causal_func"]), torch.from_numpy(g["target_aware_func"])
        a = torch.cat([a, torch.zeros(1, 1, b.shape[2] - a.shape[2], a.shape[3], dtype=torch.int32)], dim=2)   # empty intervals
        f = torch.cat([a, b], dim=0)
    else:
        f = torch.from_numpy(g[f"{case.func}_func"])
    f = f.clone()
    assert f.shape[3] == case.Sq + 256
    if case.func_heads > 1:
        f = f.repeat(1, case.func_heads, 1, 1)
        for h in range(case.func_heads):
            f[:, h, 0] = f[:, h, 0].clamp_min(h)
    f[..., case.Sq:] = PAD_VALUE
    return f


def make_inputs(case: Case):
    """CPU tensors of a case, from a generator seeded by the case's name: dict(q, k, v, causal, func, cu_seqlens_q,
    cu_seqlens_k, max_seqlen_q, max_seqlen_k)"""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) & 0x7fffffff)
    dt = case.torch_dtype
    Hq, Hkv, D = case.Hq, case.Hkv, case.D
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    cu_q = cu_k = func = None
    max_q = max_k = 0
    if case.form == "jagged":
        cu_q = torch.tensor([0] + list(np.cumsum(case.lens_q)), dtype=torch.int32)
        cu_k = torch.tensor([0] + list(np.cumsum(case.klens)), dtype=torch.int32)
        max_q, max_k = max(case.lens_q), max(case.klens)
        q = (r(sum(case.lens_q), Hq, D) * case.q_scale).to(dt)
        k, v = r(sum(case.klens), Hkv, D).to(dt), r(sum(case.klens), Hkv, D).to(dt)
    elif case.form == "strided":
        assert Hq == Hkv and case.sk == case.Sq
        qkv = r(case.B, case.Sq, 3, Hq, D).to(dt)
        q, k, v = qkv.unbind(2)
    else:
        q = (r(case.B, case.Sq, Hq, D) * case.q_scale).to(dt)
        k, v = r(case.B, case.sk, Hkv, D).to(dt), r(case.B, case.sk, Hkv, D).to(dt)
        if case.spike:   # row (b = last, i = last, h = 0): its last key is aligned with q, so that its score is the largest by far
            qv = q[-1, -1, 0].float()
            k[-1, -1, 0] = (qv * (6.0 / max(float(qv.norm()), 1e-6) * math.sqrt(math.sqrt(D)))).to(dt)
    if case.mask == "func":
        func = case_func(case)
    return dict(q=q, k=k, v=v, causal=case.mask == "causal", func=func, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k,
                max_seqlen_q=int(max_q), max_seqlen_k=int(max_k))


MISTAKES = ("causal_off_by_one", "top_left", "inclusive_end", "wrong_head", "pad_column")


def _emu_mask(Lq, Lk, causal, frows, mistake):
    j = torch.arange(Lk)[None, :]
    i = torch.arange(Lq)[:, None]
    if frows is not None:
        cols = torch.arange(Lq)
        if mistake == "pad_column":          # the last row reads the first padding column
            cols[-1] = Lq
        f = frows[:, cols].long()
        inc = 1 if mistake == "inclusive_end" else 0
        m = j < (f[0] + inc).clamp(0, Lk)[:, None]
        for p in range(1, f.shape[0] // 2 + 1):
            lo, up = f[2 * p - 1].clamp(0, Lk), (f[2 * p] + inc).clamp(0, Lk)
            m = m | ((lo[:, None] <= j) & (j < up[:, None]) & (f[2 * p - 1] < f[2 * p])[:, None])
        return m
    if causal:
        if mistake == "top_left":
            return j <= i
        return (j < i + (Lk - Lq)) if mistake == "causal_off_by_one" else (j <= i + (Lk - Lq))
    return torch.ones(Lq, Lk, dtype=torch.bool)


def emulate(inp, mistake: Optional[str] = None, key_tile: int = KEY_TILE):
    """The kernel's arithmetic in torch on the CPU: operands in their 16-bit type, fp32 scores, an online max over 64-key
    tiles in key order (the exponent of a row that has seen no key yet is taken against 0), P rounded to the operand type for
    the P V product while the row sum takes the fp32 P, O and l rescaled per tile, fp32 accumulation, one multiplication by
    1 / l, the output rounded once.  A tile no row sees is a no-op in this arithmetic, so visiting it or not is the same.
    -> out (operand dtype), lse (fp32), in the kernel's layouts"""
    assert mistake is None or mistake in MISTAKES
    q, k, v, func = inp["q"], inp["k"], inp["v"], inp["func"]
    cu_q, cu_k = inp["cu_seqlens_q"], inp["cu_seqlens_k"]
    jagged = cu_q is not None
    dt = q.dtype
    Hq, D, Hkv = q.shape[-2], q.shape[-1], k.shape[-2]
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    hk_of = torch.arange(Hq) % Hkv if mistake == "wrong_head" else torch.arange(Hq) // G
    out = torch.zeros(q.shape, dtype=dt)
    lse = torch.full((Hq, q.shape[0]) if jagged else (q.shape[0], Hq, q.shape[1]), -math.inf, dtype=torch.float32)
    if jagged:
        cq, ck = cu_q.tolist(), cu_k.tolist()
        seqs = [(None, cq[b], cq[b + 1] - cq[b], ck[b], ck[b + 1] - ck[b]) for b in range(len(cq) - 1)]
    else:
        seqs = [(b, 0, q.shape[1], 0, k.shape[1]) for b in range(q.shape[0])]
    zero, ninf = torch.zeros(()), torch.tensor(-math.inf)
    for b, q0, Lq, k0, Lk in seqs:
        if Lq == 0:
            continue
        qb = (q[q0:q0 + Lq] if jagged else q[b]).float()
        kb = (k[k0:k0 + Lk] if jagged else k[b]).float()[:, hk_of]
        vb = (v[k0:k0 + Lk] if jagged else v[b]).float()[:, hk_of]
        if func is not None:
            fh = func.shape[1]
            vis = torch.stack([_emu_mask(Lq, Lk, False, func[b, h if fh > 1 else 0], mistake) for h in range(Hq)])
        else:
            vis = _emu_mask(Lq, Lk, inp["causal"], None, mistake)[None].expand(Hq, Lq, Lk)
        s = torch.where(vis, torch.einsum("ihd,jhd->hij", qb, kb) * scale, ninf)      # fp32 [Hq, Lq, Lk]
        m = torch.full((Hq, Lq), -math.inf)
        l = torch.zeros(Hq, Lq)
        o = torch.zeros(Hq, Lq, D)
        for t in range(-(-Lk // key_tile)):
            sl = slice(t * key_tile, min((t + 1) * key_tile, Lk))
            st = s[..., sl]
            m_new = torch.maximum(m, st.max(-1).values)
            m_use = torch.where(torch.isfinite(m_new), m_new, zero)
            alpha = torch.exp(m - m_use)
            p = torch.exp(st - m_use[..., None])
            l = l * alpha + p.sum(-1)
            o = o * alpha[..., None] + torch.einsum("hij,jhd->hid", p.to(dt).float(), vb[sl])
            m = m_new
        has = l > 0
        inv = torch.where(has, 1.0 / l.clamp_min(1e-37), zero)
        ob = (o * inv[..., None]).permute(1, 0, 2).to(dt)
        ls = torch.where(has, m + torch.log(l.clamp_min(1e-37)), ninf)
        if jagged:
            out[q0:q0 + Lq] = ob
            lse[:, q0:q0 + Lq] = ls
        else:
            out[b] = ob
            lse[b] = ls
    return out, lse
