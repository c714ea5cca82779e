"""Writes tests/golden/prefill_attn_golden.npz: the arbitrary_func tensors of the reference's own encoders
(examples/sid_gr/model/attention_mask.py: build_jagged_causal_arbitrary_func, build_jagged_target_aware_arbitrary_func,
dense_mask_to_arbitrary_func, run on the CPU) for the arbitrary-mask cases of tests/prefill_attn_cases.py, the dense boolean
masks they encode (stated here independently, bit-packed), seeded q / k / v, and the fp32 results of
torch.nn.functional.scaled_dot_product_attention under those masks.

    python tests/golden/gen_prefill_attn_golden.py <root of the reference checkout>

The reference module is imported by path; only arrays are stored.  q / k / v are drawn in bf16 (stored as their 16-bit
patterns) and upcast, so the fp32 result is that of exactly representable inputs.  tests/test_prefill_attn_cpu.py decodes the
functions with the float64 twin (tests/prefill_attn_twin.py) and compares with these arrays under the twin's own fp32 bound."""
import importlib.util
import math
import os
import sys

import numpy as np
import torch

OFFSETS = [0, 37, 37, 165, 300]      # the flattened batch: lengths 37, 0, 128, 135
W, CL = 3, 4                          # target regions per sample and tokens per region (target-aware case)
D = 32
SEED = 31


def block_causal(offsets):
    S = offsets[-1]
    m = torch.zeros(S, S, dtype=torch.bool)
    for s, e in zip(offsets[:-1], offsets[1:]):
        m[s:e, s:e] = torch.tril(torch.ones(e - s, e - s, dtype=torch.bool))
    return m


def target_aware(offsets, hist):
    """history rows causal over the history; a target row sees its sample's history and, causally, its own region"""
    S = offsets[-1]
    m = torch.zeros(S, S, dtype=torch.bool)
    for b, (s, e) in enumerate(zip(offsets[:-1], offsets[1:])):
        for i in range(s, e):
            loc = i - s
            if loc < hist[b]:
                m[i, s:i + 1] = True
            else:
                reg = min((loc - hist[b]) // CL, W - 1)
                m[i, s:s + hist[b]] = True
                m[i, s + hist[b] + reg * CL:i + 1] = True
    return m


def random_mask(S, g):
    """0 to 4 random intervals per row; row 5 sees keys 130 .. 139 only (nothing in the first key tile of 64), row 9 has four
    intervals none of which starts at key 0 (n_func = 9), rows 64 .. 70 and 299 see nothing"""
    m = torch.zeros(S, S, dtype=torch.bool)
    for i in range(S):
        for _ in range(int(torch.randint(0, 5, (1,), generator=g))):
            s = int(torch.randint(0, S, (1,), generator=g))
            e = min(S, s + 1 + int(torch.randint(0, 90, (1,), generator=g)))
            if int(torch.randint(0, 4, (1,), generator=g)) == 0:
                s = 0
            m[i, s:e] = True
    m[5] = False
    m[5, 130:140] = True
    m[9] = False
    for s in (3, 70, 140, 290):
        m[9, s:s + 6] = True
    m[64:71] = False
    m[299] = False
    return m


def main(ref_root: str):
    spec = importlib.util.spec_from_file_location(
        "sid_gr_attention_mask", os.path.join(ref_root, "examples/sid_gr/model/attention_mask.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(SEED)
    S = OFFSETS[-1]
    offsets = torch.tensor(OFFSETS, dtype=torch.int64)
    lens = [e - s for s, e in zip(OFFSETS[:-1], OFFSETS[1:])]
    hist = [max(n - W * CL, 0) for n in lens]
    masks = {
        "jagged_causal": block_causal(OFFSETS),
        "target_aware": target_aware(OFFSETS, hist),
        "random": random_mask(S, g),
    }
    funcs = {
        "jagged_causal": mod.build_jagged_causal_arbitrary_func(offsets, S),
        "target_aware": mod.build_jagged_target_aware_arbitrary_func(torch.tensor(hist, dtype=torch.int64), W, CL, offsets, S),
        "random": mod.dense_mask_to_arbitrary_func(masks["random"][None], S),
    }
    q, k, v = (torch.randn(1, S, 1, D, generator=g).to(torch.bfloat16) for _ in range(3))
    out = {"offsets": np.array(OFFSETS, dtype=np.int64), "hist": np.array(hist, dtype=np.int64),
           "wcl": np.array([W, CL], dtype=np.int64)}
    for name, t in (("q", q), ("k", k), ("v", v)):
        out[name] = t.view(torch.int16).numpy()
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))            # [1, 1, S, D]
    for name, m in masks.items():
        f = funcs[name]
        assert f.dtype == torch.int32 and f.shape[:2] == (1, 1) and f.shape[3] == S + 256, f.shape
        o = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, attn_mask=m[None, None])
        o = torch.nan_to_num(o, nan=0.0).permute(0, 2, 1, 3).contiguous()     # rows that see nothing: 0
        s = (qf @ kf.transpose(-1, -2)) / math.sqrt(D)
        lse = torch.logsumexp(s.masked_fill(~m[None, None], -math.inf), dim=-1)   # [1, 1, S]; -inf for such rows
        out[f"{name}_func"] = f.numpy()
        out[f"{name}_mask"] = np.packbits(m.numpy(), axis=-1)
        out[f"{name}_out"] = o.numpy()
        out[f"{name}_lse"] = lse.numpy()
        print(name, "n_func", f.shape[2], "visible", int(m.sum()), "empty rows", int((~m.any(-1)).sum()))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prefill_attn_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
