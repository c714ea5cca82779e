"""Generates tests/golden/hstu_fp8_quant_golden.npz: the FP8 quantisers of the REFERENCE's hopper interface, run as the
reference states them.  `quantize_for_two_directions`, `quantize_for_block_scale`, `get_bm_and_bn_block_size_fwd` and
`quantize_for_head_batch_tensor` (/root/reference/corelib/hstu/hopper/hstu_attn_interface.py:32-292) are pulled out of
that file's AST (the file itself imports the CUDA extension), `device="cuda"` rewritten to the CPU, and run on jagged bf16
and fp16 inputs: lengths that are no multiple of 16, 64 or 128, a sequence shorter than one block, an all-zero head, and both
mode-2 block sizes (64, 128) on every case
(every descale of it sits on the 1e-6 floor).  Mode 0 is the plain `x.to(torch.float8_e4m3fn)` of
HSTUAttnVarlenFunc.forward (:474-478).  fp8 tensors are stored as their raw bytes (uint8), 16-bit inputs as raw bits.
Run in the build container only:

    python tests/golden/gen_hstu_fp8_golden.py
"""
import ast
import os
import zlib

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference/corelib/hstu/hopper/hstu_attn_interface.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hstu_fp8_quant_golden.npz")
WANT = {"quantize_for_two_directions", "quantize_for_block_scale", "get_bm_and_bn_block_size_fwd",
        "quantize_for_head_batch_tensor"}


class _ToCpu(ast.NodeTransformer):
    def visit_keyword(self, node):
        if node.arg == "device" and isinstance(node.value, ast.Constant) and node.value.value == "cuda":
            node.value = ast.Constant("cpu")
        return node


ns = {"torch": torch, "nn": nn}
for node in ast.parse(open(REF).read()).body:
    if isinstance(node, ast.FunctionDef) and node.name in WANT:
        node = ast.fix_missing_locations(_ToCpu().visit(node))
        exec(compile(ast.Module([node], []), REF, "exec"), ns)

CASES = [
    # name, dtype, lengths, H, d, zero head  (kept small: the fixture is committed; every block size is run on every case)
    ("bf16_d64", torch.bfloat16, [70, 17, 3], 2, 64, 1),
    ("f16_d128", torch.float16, [5, 30], 1, 128, None),
    ("bf16_d256", torch.bfloat16, [11, 2], 1, 256, None),
    ("f16_d32_zero", torch.float16, [129, 1], 2, 32, 1),
]


def raw(t):
    if t.dtype == torch.float8_e4m3fn:
        return t.view(torch.uint8).numpy()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def run(case, out):
    name, dt, lengths, H, d, zero = case
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) % (2**31))
    off = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32)
    T = int(off[-1])
    # per-head and per-token magnitudes that differ, a few outliers, values well inside e4m3's range for mode 0
    x = torch.empty(T, H, d).uniform_(-1.0, 1.0, generator=gen)
    x *= torch.empty(1, H, 1).uniform_(0.05, 4.0, generator=gen)
    x *= torch.empty(T, 1, 1).uniform_(0.1, 3.0, generator=gen)
    x[torch.randint(0, T, (4,), generator=gen), torch.randint(0, H, (4,), generator=gen)] *= 20.0
    if zero is not None:
        x[:, zero] = 0.0
    x = x.to(dt)
    p = name + "/"
    out[p + "x"] = raw(x)
    out[p + "offsets"] = off.numpy()
    out[p + "meta"] = np.array([1 if dt == torch.float16 else 0, T, H, d], np.int64)
    out[p + "m0_x"] = raw(x.to(torch.float8_e4m3fn))
    xq, xd, xtq, xtd, cu = ns["quantize_for_two_directions"](x, off)
    for k, v in (("x", xq), ("descale", xd), ("xt", xtq), ("descale_xt", xtd), ("cu", cu)):
        out[p + "m1_" + k] = raw(v)
    bm, bn = ns["get_bm_and_bn_block_size_fwd"](None, d)
    out[p + "m2_blocks"] = np.array([bm, bn], np.int64)
    for bs in (64, 128):
        xq, xd, cu = ns["quantize_for_block_scale"](x, off, block_size=bs)
        for k, v in (("x", xq), ("descale", xd), ("cu", cu)):
            out[p + f"m2_{bs}_" + k] = raw(v)
    for m in (3, 4, 5):
        xq, xd = ns["quantize_for_head_batch_tensor"](x, off, quant_mode=m)
        out[p + f"m{m}_x"], out[p + f"m{m}_descale"] = raw(xq), raw(xd)


if __name__ == "__main__":
    out = {}
    for c in CASES:
        run(c, out)
    out["cases"] = np.array([c[0] for c in CASES])
    np.savez_compressed(OUT, **out)
    print(OUT, len(out), "arrays,", os.path.getsize(OUT), "bytes")
