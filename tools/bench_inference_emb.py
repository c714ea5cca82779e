"""Inference embedding lookup on the C2 table shape (10 M x 128-D fp32, one table) for a 131 K-token sequence batch (Zipf-0.99 keys,
no pooling), three ways in one process:

  fused     InferenceEmbeddingCollection, INFERENCE_EMB::inference_emb_forward (one launch, csrc/inference_emb.hip)
  composed  the same collection with fused=False: get_table_range, expand_table_ids, table_lookup, index_select + add, gather
  eval      the one-kernel eval forward of the training module (BatchedDynamicEmbeddingTablesV2.eval())

Each call is bracketed by HIP events on the stream (what a caller waits for, launch gaps of the multi-launch leg included);
median and minimum of --iters calls after --warmup.  Usage: bench_inference_emb.py [--iters N] [--warmup W] [--unknown SHARE] [--out FILE]
(default FILE: profiles/inference_emb_bench.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import dynamicemb_extensions as ext  # noqa: E402
from dynamicemb.batched_dynamicemb_tables import BatchedDynamicEmbeddingTablesV2  # noqa: E402
from dynamicemb.dynamicemb_config import DynamicEmbPoolingMode, DynamicEmbTableOptions, EmbOptimType  # noqa: E402
from dynamicemb.exportable_tables import InferenceEmbeddingCollection  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--known", type=int, default=4_000_000)
ap.add_argument("--tokens", type=int, default=131072)
ap.add_argument("--unknown", type=float, default=0.03, help="share of the tokens whose key is in no table")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inference_emb_bench.txt"))
a = ap.parse_args()

dev = torch.device("cuda")
D = 128
g = torch.Generator(device=dev)
g.manual_seed(0)
# `known` distinct keys, Zipf-0.99 over them (rank r -> key perm[r]), a few per cent of the tokens unknown
perm = (torch.randperm(a.known, device=dev, generator=g) * 2654435761 + 12345) % (1 << 44)
w = torch.arange(1, a.known + 1, device=dev, dtype=torch.float64).pow_(-0.99)
cdf = torch.cumsum(w, 0)
cdf /= cdf[-1].clone()
ranks = torch.searchsorted(cdf, torch.rand(a.tokens, device=dev, dtype=torch.float64, generator=g)).clamp_(max=a.known - 1)
keys = perm[ranks]
keys = torch.where(torch.rand(a.tokens, device=dev, generator=g) < a.unknown, keys + (1 << 50), keys).contiguous()
offsets = torch.tensor([0, a.tokens], dtype=torch.int64, device=dev)

opt = DynamicEmbTableOptions(dim=D, max_capacity=a.rows, index_type=torch.int64, embedding_dtype=torch.float32)
coll = InferenceEmbeddingCollection([opt], True, -1, device=dev)
ht = coll.hash_table
coll.weight.uniform_(-1, 1)
coll.weight[0] = 0
failed = 0
for s in range(0, a.known, 1 << 20):
    k = perm[s: s + (1 << 20)].contiguous()
    idx = ext.table_insert(ht.table_storage_, ht.table_bucket_offsets_, ht.bucket_capacity_, ht.bucket_sizes, k, torch.zeros_like(k),
                           None, 0, ht._ref_counter, None, None)
    failed += int((idx < 0).sum().item())


def timed(fn):
    with torch.no_grad():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def leg(fused):
    coll.fused = fused
    return coll(keys, offsets)


with torch.no_grad():
    same = torch.equal(leg(True), leg(False))
    found = float((leg(True).abs().sum(1) > 0).float().mean().item())
res = {"fused": timed(lambda: leg(True)), "composed": timed(lambda: leg(False))}
print({k: f"{v[0]:.1f} us" for k, v in res.items()}, flush=True)

train = BatchedDynamicEmbeddingTablesV2([opt], pooling_mode=DynamicEmbPoolingMode.NONE, optimizer=EmbOptimType.SGD,
                                        output_dtype=torch.float32, device=dev)
train.train()
for s in range(0, a.known, 1 << 20):   # a training forward inserts the keys it does not know
    k = perm[s: s + (1 << 20)].contiguous()
    train(k, torch.tensor([0, k.numel()], dtype=torch.int64, device=dev))
train.eval()
res["eval"] = timed(lambda: train(keys, offsets))
with torch.no_grad():
    same_eval = bool((train(keys, offsets).abs().sum(1) > 0).float().mean().item() == found)
lines = [f"inference embedding lookup, {a.rows} x {D} fp32 rows, {a.known} keys loaded ({failed} refused), {a.tokens} tokens "
         f"(Zipf-0.99, {found:.3f} found), no pooling; us per call over {a.iters} calls after {a.warmup}: median / min",
         f"fused == composed bit for bit: {same}; the training module finds the same share of the tokens: {same_eval}"]
for name, (med, mn) in res.items():
    lines.append(f"{name:9s} {med:8.1f} {mn:8.1f}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "a" if a.unknown != 0.03 else "w") as f:   # (a run with another share of unknown keys adds to the file)
    f.write(text)
