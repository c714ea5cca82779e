"""The C2 training step (bench.py's key stream, 10 M x 128-D fp32, B = 65,536 bags, SGD) under the LFU score strategy, timed
three ways in one process: no per-key frequency weights, all-ones weights (bit-identical results, the weighted kernels), and
random integer weights in 1..8.  One JSON line: ms per step (forward + backward, wall clock over `steps` after `warmup`) and
whether the weighted steps stayed on path (c) and the plan.
Usage: bench_lfu_weights.py [--steps 50] [--warmup 10] [--rows 10000000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "recsys-examples_amd"), ROOT]
import torch  # noqa: E402

from bench import zipf_batches  # noqa: E402


def build(rows, dim, dev):
    from dynamicemb.batched_dynamicemb_tables import BatchedDynamicEmbeddingTablesV2
    from dynamicemb.dynamicemb_config import (DynamicEmbInitializerArgs, DynamicEmbInitializerMode, DynamicEmbPoolingMode,
                                              DynamicEmbScoreStrategy, DynamicEmbTableOptions, EmbOptimType)

    opt = DynamicEmbTableOptions(dim=dim, max_capacity=rows, embedding_dtype=torch.float32, index_type=torch.int64,
                                 score_strategy=DynamicEmbScoreStrategy.LFU,
                                 initializer_args=DynamicEmbInitializerArgs(mode=DynamicEmbInitializerMode.UNIFORM, lower=-0.01, upper=0.01))
    m = BatchedDynamicEmbeddingTablesV2([opt], feature_table_map=[0], pooling_mode=DynamicEmbPoolingMode.SUM, output_dtype=torch.bfloat16,
                                        optimizer=EmbOptimType.SGD, learning_rate=0.1, device=dev)
    m.train()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=65536)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    batches = zipf_batches(a.rows, 0.99, a.batch, 8, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    weights = {"none": [None] * len(batches),
               "ones": [torch.ones(k.numel(), dtype=torch.int64, device=dev) for k, _ in batches],
               "random_1_8": [torch.randint(1, 9, (k.numel(),), dtype=torch.int64, device=dev, generator=g) for k, _ in batches]}
    res = {"tool": "bench_lfu_weights", "config": f"C2 LFU: 1 x {a.rows} x {a.dim}-D fp32, B = {a.batch}, SGD, bf16 out",
           "keys_per_step": int(batches[0][0].numel())}
    for name, ws in weights.items():
        m = build(a.rows, a.dim, dev)
        grad = torch.full((a.batch, a.dim), 1e-3, dtype=torch.bfloat16, device=dev)
        pathc = []

        def run(k):
            for i in range(k):
                keys, off = batches[i % len(batches)]
                out = m(keys, off, per_sample_weights=ws[i % len(batches)])
                pathc.append(bool(m._plan_ok and m._fused))
                out.backward(grad)

        run(a.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(a.steps)
        torch.cuda.synchronize()
        res[f"ms_{name}"] = round((time.perf_counter() - t0) / a.steps * 1e3, 4)
        res[f"plan_{name}"] = all(pathc)
        del m
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
