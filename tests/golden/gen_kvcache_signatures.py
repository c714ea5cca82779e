"""Writes tests/golden/kvcache_signatures.json: the names the KV cache GPU tier shares with the reference's
corelib/recsys_kvcache_manager --

* the methods of `DeviceKVCache` (gpu_kvcache_manager.py) with their parameter names, order and default literals,
* the field names of the dataclasses `KVCacheMetadata` (kvcache_metadata.py) and `KVLookupResult` (kvcache_utils.py), in order,
  and the parameters of `get_kvcache_metadata_buffer` / `copy_kvcache_metadata`,
* the parameter names of `gather_kvcache` (the C++ function bound under that name in
  examples/commons/ops/cuda_ops/csrc/paged_kvcache_ops_cuda.cpp).

    python tests/golden/gen_kvcache_signatures.py <root of the reference checkout>

The Python sources are parsed with `ast` and the C++ parameter list with a regular expression: nothing of the reference is
imported, run or copied; what is recorded is lists of names and the source text of each default literal (null: no default).
tests/test_kvcache_allocator_cpu.py compares recsys_kvcache_manager and paged_kvcache_ops with it."""
import ast
import json
import os
import re
import sys

PKG = "corelib/recsys_kvcache_manager/recsys_kvcache_manager/"
CPP = "examples/commons/ops/cuda_ops/csrc/paged_kvcache_ops_cuda.cpp"


def signature(fn: ast.FunctionDef):
    args = fn.args
    assert not args.posonlyargs and not args.kwonlyargs and args.vararg is None and args.kwarg is None
    defaults = [None] * (len(args.args) - len(args.defaults)) + [ast.unparse(d) for d in args.defaults]
    return [[a.arg, d] for a, d in zip(args.args, defaults)]


def _module(ref_root, name):
    return ast.parse(open(os.path.join(ref_root, PKG, name)).read())


def _class(tree, name):
    return next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)


def _fields(cls: ast.ClassDef):
    return [n.target.id for n in cls.body if isinstance(n, ast.AnnAssign)]


def _cpp_params(ref_root, bound_name):
    src = open(os.path.join(ref_root, CPP)).read()
    target = re.search(r'm\.def\("%s",\s*&(\w+)' % bound_name, src).group(1)
    params = re.search(r"\b%s\s*\(([^)]*)\)\s*\{" % target, src).group(1)
    return [re.split(r"[\s*&]+", p.strip())[-1] for p in params.split(",")]


def main(ref_root: str):
    gpu = _module(ref_root, "gpu_kvcache_manager.py")
    meta = _module(ref_root, "kvcache_metadata.py")
    utils = _module(ref_root, "kvcache_utils.py")
    dev = _class(gpu, "DeviceKVCache")
    out = {
        "DeviceKVCache": {n.name: signature(n) for n in dev.body if isinstance(n, ast.FunctionDef)},
        "DeviceKVCache_aliases": [n.targets[0].id for n in gpu.body if isinstance(n, ast.Assign)
                                  and isinstance(n.value, ast.Name) and n.value.id == "DeviceKVCache"],
        "KVCacheMetadata": _fields(_class(meta, "KVCacheMetadata")),
        "KVLookupResult": _fields(_class(utils, "KVLookupResult")),
        "KVIndexMeta": _fields(_class(utils, "KVIndexMeta")),
        "kvcache_metadata_functions": {n.name: signature(n) for n in meta.body if isinstance(n, ast.FunctionDef)},
        "gather_kvcache": _cpp_params(ref_root, "gather_kvcache"),
    }
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kvcache_signatures.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
