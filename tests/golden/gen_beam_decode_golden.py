"""Writes tests/golden/beam_decode_golden.npz: inputs and fp32 results of the reference's single-pass PyTorch statement of
beam-search decode attention (corelib/gr_decode_atten/tests/reference.py: generate_test_data on the CPU, then
beam_attention_ref(upcast=True)).

    python tests/golden/gen_beam_decode_golden.py <root of the reference checkout>

The reference module is imported by path and run on the CPU; only arrays are stored.  The inputs are drawn in bf16 (stored as
their 16-bit patterns) and upcast by the reference, so its fp32 result is that of exactly representable inputs.
tests/test_beam_decode_cpu.py compares the float64 twin (tests/beam_decode_twin.py) with these arrays under the twin's own
fp32 bound."""
import importlib.util
import os
import sys

import numpy as np
import torch

# (B, W, Hq, Hkv, D, ctx, decode_nums, max_decode_nums)
CASES = [
    (2, 5, 4, 2, 64, 37, 3, 5),
    (1, 3, 4, 4, 64, 0, 2, 4),     # no context: the beam keys alone
    (1, 3, 4, 1, 64, 9, 0, 2),     # no beam keys: the context alone
]


def main(ref_root: str):
    spec = importlib.util.spec_from_file_location(
        "gr_decode_reference", os.path.join(ref_root, "corelib/gr_decode_atten/tests/reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(24)
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for i, (B, W, Hq, Hkv, D, ctx, dn, max_dn) in enumerate(CASES):
        q, kc, vc, kb, vb, topk, _ = mod.generate_test_data(B, 1, W, Hq, Hkv, D, ctx, dn, max_decode_nums=max_dn,
                                                            dtype=torch.bfloat16, device="cpu")
        o, lse = mod.beam_attention_ref(q, kc, vc, kb, vb, topk, dn, upcast=True)
        for name, t in (("q", q), ("k_context", kc), ("v_context", vc), ("k_beam", kb), ("v_beam", vb)):
            out[f"c{i}_{name}"] = t.view(torch.int16).numpy()
        out[f"c{i}_topk"] = topk.numpy().astype(np.int32)
        out[f"c{i}_out"] = o.float().numpy()
        out[f"c{i}_lse"] = lse.float().numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "beam_decode_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
