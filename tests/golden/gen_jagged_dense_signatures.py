"""Writes tests/golden/jagged_dense_signatures.json: parameter names, their order and their default literals of the seven
public functions of the reference's examples/commons/ops/triton_ops/triton_jagged.py.

    python tests/golden/gen_jagged_dense_signatures.py <root of the reference checkout>

The reference source is parsed with `ast` only: nothing of it is imported, run or copied; what is recorded is a list of names
and the source text of each default literal (null: no default).  tests/test_hstu_jagged_dense_cpu.py compares the signatures
of hstu_jagged.py with it."""
import ast
import json
import os
import sys

SOURCE = "examples/commons/ops/triton_ops/triton_jagged.py"
FUNCTIONS = ["triton_jagged_dense_bmm", "triton_jagged_dense_bmm_broadcast_add", "triton_jagged_dense_broadcast_add",
             "triton_concat_2D_jagged", "triton_concat_2D_jagged_jagged", "triton_concat_2D_dense_jagged",
             "triton_split_2D_jagged"]


def signature(fn: ast.FunctionDef):
    args = fn.args
    assert not args.posonlyargs and not args.kwonlyargs and args.vararg is None and args.kwarg is None
    defaults = [None] * (len(args.args) - len(args.defaults)) + [ast.unparse(d) for d in args.defaults]
    return [[a.arg, d] for a, d in zip(args.args, defaults)]


def main(ref_root: str):
    tree = ast.parse(open(os.path.join(ref_root, SOURCE)).read())
    found = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    out = {name: signature(found[name]) for name in FUNCTIONS}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jagged_dense_signatures.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
