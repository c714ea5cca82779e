"""Writes tests/golden/fused_layer_signatures.json: parameter names, their order and their default literals of the reference's
fused HSTU layer function and of the addmm / SiLU functions it is built on.

    python tests/golden/gen_fused_layer_golden.py <root of the reference checkout>

The reference sources are parsed with `ast` only: nothing of them is imported, run or copied; what is recorded is a list of
names and the source text of each default literal (null: no default).  tests/test_hstu_fused_layer_cpu.py compares the
signatures of fused_hstu_op.py and hstu_addmm.py with it."""
import ast
import json
import os
import sys

FUNCTIONS = {
    "examples/hstu/ops/fused_hstu_op.py": ["fused_hstu_op"],
    "examples/hstu/ops/triton_ops/triton_addmm.py": ["triton_addmm_silu_fwd", "triton_addmm_silu_bwd", "triton_addmm"],
    "examples/hstu/ops/pt_ops/torch_addmm.py": ["torch_addmm_silu_fwd"],
    "examples/hstu/ops/triton_ops/triton_silu.py": ["triton_silu_fwd", "triton_silu_bwd", "triton_silu"],
}


def signature(fn: ast.FunctionDef):
    args = fn.args
    assert not args.posonlyargs and not args.kwonlyargs and args.vararg is None and args.kwarg is None
    defaults = [None] * (len(args.args) - len(args.defaults)) + [ast.unparse(d) for d in args.defaults]
    return [[a.arg, d] for a, d in zip(args.args, defaults)]


def main(ref_root: str):
    out = {}
    for rel, names in FUNCTIONS.items():
        tree = ast.parse(open(os.path.join(ref_root, rel)).read())
        found = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
        for name in names:
            out[name] = signature(found[name])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fused_layer_signatures.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
