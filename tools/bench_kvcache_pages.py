"""KV cache page mover (csrc/kvcache_ops.hip, DeviceKVCache.offload_pages / onboard_pages) at the serving shape: 8 layers,
page_size 32, H = 4, D = 128, bf16 -- 64 KiB per page and layer.  Two moves of randomly chosen pages of a 4 GiB cache: 1024 pages
(512 MiB, bandwidth-bound) and 32 pages (16 MiB, launch-bound).  Timed in one process, HIP events around --reps calls per
window, every line warmed up, --passes passes over all lines in turn (the median pass is printed, the spread next to it):

  mover        the all-layers launch, gather and scatter, at its default grid cap and cache hint
  cap / nt     the same launch at every grid cap of the sweep (256-thread blocks), with plain and with nontemporal ("nt")
               loads and stores: the defaults in csrc/kvcache_ops.hip were picked from these lines
  torch        what a user would write without it: torch.index_select(cache, 1, ids, out=staging) and
               cache.index_copy_(1, ids, staging)
  copy         a device-to-device copy_ of the same number of contiguous bytes: the ceiling
  per layer    L single-layer calls (paged_kvcache_ops.gather_kvcache / scatter_kvcache on the unbind tables)

GB/s counts the moved bytes once (read once and written once).  "/ copy" is the copy's time over the line's (1.0 = the
ceiling), "/ torch" the torch expression's time over the line's (> 1: faster than torch).  Last, the append-metadata kernel
once: B = 8, 1024 new tokens.

    python tools/bench_kvcache_pages.py [--reps 50] [--passes 3] [--out profiles/kvcache_pages_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import torch  # noqa: E402

import paged_kvcache_ops  # noqa: E402
from recsys_kvcache_manager import DeviceKVCache, page_ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--pages", type=int, default=8192, help="pages of the cache")
ap.add_argument("--out", default="")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_kvcache_pages.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")
L, PS, H, D = 8, 32, 4, 128
CAPS = [512, 2048, 8192, 16384, 32768, 65536]

kv = DeviceKVCache(L, H, D, PS, 4 * PS, a.pages, a.pages, 8, 4096, torch.bfloat16, torch.cuda.current_device())
cache = kv.gpu_kvcache_tensor
cache.view(torch.int16).random_(-32768, 32768)
tables = kv.get_cache_tables()
page_bytes = cache[0, 0].numel() * 2
lines_out = []


def emit(s=""):
    print(s, flush=True)
    lines_out.append(s)


def time_us(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / a.reps


def run(items):
    """items: [(name, fn)] -> {name: (median us, min us, max us)} over the passes, the lines taken in turn in every pass"""
    for _, fn in items:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name, _ in items}
    for _ in range(a.passes):
        for name, fn in items:
            got[name].append(time_us(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


emit(f"device {torch.cuda.get_device_name()}  torch {torch.__version__}  reps {a.reps}  passes {a.passes}  "
     f"cache {L} x {a.pages} pages x {page_bytes // 1024} KiB = {cache.numel() * 2 / 2 ** 30:.1f} GiB")
for n in (1024, 32):
    g = torch.Generator().manual_seed(n)
    ids = torch.randperm(a.pages, generator=g)[:n].to(torch.int32).to(dev)
    ids64 = ids.long()
    staging = torch.empty((L, n) + tuple(cache.shape[2:]), dtype=cache.dtype, device=dev)
    staging.view(torch.int16).random_(-32768, 32768)
    twin = torch.empty_like(staging)
    nbytes = staging.numel() * 2
    # (the moves agree before they are timed)
    assert torch.equal(kv.offload_pages(ids).view(torch.int16), torch.index_select(cache, 1, ids64).view(torch.int16))

    def per_layer(op):
        def fn():
            for l in range(L):
                op(staging[l], tables[l], ids, n, 0, 0)
        return fn

    items = [("copy", lambda: twin.copy_(staging)),
             ("gather  mover", lambda: page_ops.move_pages(page_ops.GATHER, cache, staging, ids, n)),
             ("gather  torch index_select", lambda: torch.index_select(cache, 1, ids64, out=staging)),
             ("gather  per layer", per_layer(paged_kvcache_ops.gather_kvcache)),
             ("scatter mover", lambda: page_ops.move_pages(page_ops.SCATTER, cache, staging, ids, n)),
             ("scatter torch index_copy_", lambda: cache.index_copy_(1, ids64, staging)),
             ("scatter per layer", per_layer(paged_kvcache_ops.scatter_kvcache))]
    for d, dname in ((page_ops.GATHER, "gather "), (page_ops.SCATTER, "scatter")):
        for nt in (0, 1):
            for cap in CAPS:
                items.append((f"{dname} mover cap {cap}{' nt' if nt else ''}", lambda d=d, cap=cap, nt=nt: page_ops.move_pages(
                    d, cache, staging, ids, n, grid_cap=cap, nontemporal=nt)))
    res = run(items)
    emit()
    emit(f"{n} pages x {L} layers, {nbytes / 2 ** 20:.0f} MiB")
    emit(f"{'':32s} {'us':>9s} {'min':>9s} {'max':>9s} {'GB/s':>8s} {'/ copy':>7s} {'/ torch':>8s}")
    copy_us = res["copy"][0]
    for name, _ in items:
        med, lo, hi = res[name]
        torch_us = res["gather  torch index_select" if name.startswith("gather") else "scatter torch index_copy_"][0]
        vs_torch = "" if name == "copy" else f"{torch_us / med:8.2f}"
        emit(f"{name:32s} {med:9.1f} {lo:9.1f} {hi:9.1f} {nbytes / med / 1e3:8.0f} {copy_us / med:7.2f} {vs_torch}")

B, nnz = 8, 1024
new = torch.full((B,), nnz // B, dtype=torch.int32)
off = torch.cat([torch.zeros(1, dtype=torch.int32), new.cumsum(0).int()]).to(dev)
total = (new + 1000).to(dev)
bi, pos = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev)
res = run([("append metadata", lambda: page_ops.batch_positions(off, total, nnz, bi, pos))])
emit()
emit(f"append metadata kernel, B = {B}, {nnz} new tokens: {res['append metadata'][0]:.1f} us per call "
     f"(min {res['append metadata'][1]:.1f}, max {res['append metadata'][2]:.1f}; back-to-back calls, launch included)")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines_out) + "\n")
