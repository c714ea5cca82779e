"""The FBGEMM jagged ops of fbgemm_jagged_ops (torch.ops.fbgemm.*), each next to three yardsticks timed in the same process
(HIP events around --reps back-to-back calls, warmed up; a call that is host-bound is charged its host time, as a training
step would be):

  clone   torch.clone of a contiguous tensor of the bytes the op writes: the copy ceiling of the machine for these bytes
  tiny    fill_ of a one-element tensor: what one launch costs from Python at all
  comp    the torch composition of the same op -- the op's own "CPU" implementation (fbgemm_jagged_ops.COMPOSITIONS) run on
          the GPU tensors: what the example would pay without the kernels.  The sizes the ops would read on the host are
          passed in (total_L, selected_lengths_sum), so no sync is charged to either side.

"comp /" is the composition's time over ours (> 1: the kernel path is faster); "/ clone" ours over the clone's.

Shapes: 32 samples x 512 rows and 8 x 4096, lengths uniform in [L / 2, L], D in {1, 256, 1024}, bf16 and int64 (to dense, back,
and back from the slice dense[:, 1:] as jagged_tensors_shift_n passes it); the three cumsums at N in {32, 4096, 1 M}; the
batch select with F = 8 features of bags randint(0, 11) plus one sequence feature of 512 ids per bag, B = S = 4096.

A last table gives the scan's GPU time alone (calls captured into a graph and replayed) next to torch.cumsum's and a clone's.

    python tools/bench_fbgemm_jagged.py [--reps 50]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fbgemm_jagged_ops as J  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_fbgemm_jagged.py needs a GPU: a time taken anywhere else says nothing")
dev = torch.device("cuda")
ops, comp = torch.ops.fbgemm, J.COMPOSITIONS


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


worst = [None]


def report(op, shape, ours, composed, out_bytes):
    same = all(torch.equal(x, y) for x, y in zip(ours(), composed())) if isinstance(ours(), (list, tuple)) \
        else torch.equal(ours(), composed())
    assert same, (op, shape)
    buf = torch.empty(max(out_bytes, 1), dtype=torch.uint8, device=dev)
    one = torch.empty(1, device=dev)
    t_ours, t_comp = timeit(ours, a.reps), timeit(composed, a.reps)
    t_clone, t_tiny = timeit(lambda: buf.clone(), a.reps), timeit(lambda: one.fill_(0), a.reps)
    ratio = t_comp / t_ours
    if worst[0] is None or ratio < worst[0][0]:
        worst[0] = (ratio, op, shape)
    print(f"{op:34s} {shape:42s} {out_bytes / 1e6:8.2f} | {t_ours:8.1f} {t_clone:8.1f} {t_tiny:6.1f} {t_comp:8.1f} | "
          f"{ratio:7.2f} {t_ours / t_clone:7.2f}", flush=True)


print(f"{'op':34s} {'shape':42s} {'MB out':>8s} | {'ours':>8s} {'clone':>8s} {'tiny':>6s} {'comp':>8s} | {'comp /':>7s} "
      f"{'/ clone':>7s}   (times in us)", flush=True)

# ---- cumsum ----
for name in ("asynchronous_complete_cumsum", "asynchronous_inclusive_cumsum", "asynchronous_exclusive_cumsum"):
    for n in (32, 4096, 1 << 20):
        for dtype in (torch.int64, torch.int32):
            x = torch.randint(0, 100, (n,), device=dev, dtype=dtype)
            report(name, f"N = {n} {str(dtype)[6:]}", lambda: getattr(ops, name)(x), lambda: comp[name](x),
                   (n + (name == "asynchronous_complete_cumsum")) * x.element_size())

# ---- jagged <-> padded dense ----
rng = np.random.default_rng(1)
for B, L in ((32, 512), (8, 4096)):
    lengths = rng.integers(L // 2, L + 1, size=B)
    off = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    short = torch.tensor(np.concatenate([[0], np.cumsum(lengths - 1)]), dtype=torch.int64, device=dev)
    total = int(lengths.sum())
    for dtype in (torch.bfloat16, torch.int64):
        for D in (1, 256, 1024):
            values = torch.randint(-1000, 1000, (total, D), device=dev).to(dtype)
            shape = f"{B} x {L} D = {D} {str(dtype)[6:]}"
            eb = values.element_size()
            report("jagged_to_padded_dense", shape, lambda: ops.jagged_to_padded_dense(values, [off], [L], 0.0),
                   lambda: comp["jagged_to_padded_dense"](values, [off], [L], 0.0), B * L * D * eb)
            dense = ops.jagged_to_padded_dense(values, [off], [L], 0.0)
            report("dense_to_jagged", shape, lambda: ops.dense_to_jagged(dense, [off], total)[0],
                   lambda: comp["dense_to_jagged"](dense, [off], total)[0], total * D * eb)
            report("dense_to_jagged(dense[:, 1:])", shape, lambda: ops.dense_to_jagged(dense[:, 1:], [short], total - B)[0],
                   lambda: comp["dense_to_jagged"](dense[:, 1:], [short], total - B)[0], (total - B) * D * eb)
            del values, dense

# ---- KeyedJaggedTensor batch select ----
F, B = 8, 4096
g = torch.Generator().manual_seed(2)
name = "keyed_jagged_index_select_dim1"
for label, lengths in (("F = 8 bags 0..10", torch.randint(0, 11, (F * B,), generator=g)),
                       ("F = 8 + one feature of 512 ids", torch.cat([torch.randint(0, 11, (F * B,), generator=g),
                                                                       torch.full((B,), 512)]))):
    lengths = lengths.to(dev)
    offsets = ops.asynchronous_complete_cumsum(lengths)
    n = int(offsets[-1])
    values = torch.randint(0, 10 ** 9, (n,), device=dev)
    weights = torch.rand(n, device=dev)
    indices = torch.randperm(B, generator=g).to(dev)
    for w, wl in ((None, ""), (weights, " + weights")):
        report(name, f"{label}{wl}", lambda: ops.keyed_jagged_index_select_dim1(values, lengths, offsets, indices, B, w, n),
               lambda: comp[name](values, lengths, offsets, indices, B, w, n), n * (8 + (4 if w is not None else 0)))

print(f"\nworst comp / ours: {worst[0][0]:.2f} ({worst[0][1]}, {worst[0][2]})")


# ---- the scan's GPU time alone: 20 calls captured into one graph and replayed, no host in the way ----
def graph_time(fn, k=20, reps=20):
    fn()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        for _ in range(k):
            fn()
    return timeit(graph.replay, reps) / k


print("\nGPU time per call inside a graph (us): the scan kernel in inclusive mode (the op itself hands rows past "
      f"{J.ONE_BLOCK_SCAN} elements to torch.cumsum), torch.cumsum, a clone")
print(f"{'N':>9s} {'dtype':>6s} | {'kernel':>8s} {'complete':>8s} {'torch':>8s} {'clone':>8s}")
for n in (4096, 8192, 16384, 1 << 20, 1 << 23):
    for dtype in (torch.int64, torch.int32):
        x = torch.randint(0, 100, (n,), device=dev, dtype=dtype)
        print(f"{n:9d} {str(dtype)[6:]:>6s} | {graph_time(lambda: J._cumsum_cuda(J.INCLUSIVE, x, kernel_only=True)):8.2f} "
              f"{graph_time(lambda: ops.asynchronous_complete_cumsum(x)):8.2f} "
              f"{graph_time(lambda: torch.cumsum(x, 0, dtype=dtype)):8.2f} {graph_time(lambda: x.clone()):8.2f}", flush=True)
