"""Writes tests/golden/norm_family_golden.npz: inputs and fp32 results of the reference's PyTorch statement of the group norm
mul dropout (examples/hstu/ops/pt_ops/pt_norm_mul_dropout.py, group_norm=True, training=False, with and without concat_ux)
under torch.autograd, and of x * sigmoid(F.layer_norm(x)) for the swish layer norm.

    python tests/golden/gen_norm_family_golden.py <root of the reference checkout>

The reference module is imported and run on the CPU; only arrays are stored (a few cases of at most 8 x 72, fp32).  The RMS
norm has no PyTorch statement in the reference, so there is no golden for it.  tests/test_hstu_norm_family_cpu.py compares the
float64 twin (tests/norm_family_twin.py) with these arrays under the twin's own fp32 bounds."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
GN_CASES = [(4, 4, 16), (3, 3, 24), (3, 1, 40), (3, 6, 12)]   # (N, H, L)
SWISH_CASES = [(6, 72), (5, 8)]                              # (N, D)


def main(ref_root: str):
    spec = importlib.util.spec_from_file_location(
        "pt_norm_mul_dropout", os.path.join(ref_root, "examples/hstu/ops/pt_ops/pt_norm_mul_dropout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(20)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    out = {}
    for i, (n, H, L) in enumerate(GN_CASES):
        for concat_ux in (False, True):
            key = f"gn{i}_{int(concat_ux)}"
            x, u = (r(n, H * L) + 0.5).requires_grad_(True), r(n, H * L).requires_grad_(True)
            w, b = (1 + 0.1 * r(H)).requires_grad_(True), (0.1 * r(H)).requires_grad_(True)
            dy = r(n, 3 * H * L if concat_ux else H * L)
            y = mod.pytorch_norm_mul_dropout(x, u, w, b, EPS, 0.3, False, concat_ux=concat_ux, group_norm=True, num_heads=H,
                                             linear_dim=L)
            dx, du, dw, db = torch.autograd.grad(y, (x, u, w, b), dy)
            out[key + "_shape"] = np.array([n, H, L], dtype=np.int64)
            for name, t in (("x", x), ("u", u), ("w", w), ("b", b), ("dy", dy), ("y", y), ("dx", dx), ("du", du), ("dw", dw),
                            ("db", db)):
                out[f"{key}_{name}"] = t.detach().numpy().astype(np.float32)
    for i, (n, D) in enumerate(SWISH_CASES):
        key = f"swish{i}"
        x = (r(n, D) + 0.5).requires_grad_(True)
        w, b = (1 + 0.1 * r(D)).requires_grad_(True), (0.1 * r(D)).requires_grad_(True)
        dy = r(n, D)
        y = x * torch.sigmoid(F.layer_norm(x, (D,), w, b, EPS))
        dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
        for name, t in (("x", x), ("w", w), ("b", b), ("dy", dy), ("y", y), ("dx", dx), ("dw", dw), ("db", db)):
            out[f"{key}_{name}"] = t.detach().numpy().astype(np.float32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "norm_family_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
