"""Phase break-down of the C2 step's kernels from the s_memtime stamps of a profiling build (csrc/stamps.h).

    python recsys-examples_amd/build.py --variant stamps -DMI355_STAMPS=1
    MI355_LIB=$PWD/recsys-examples_amd/lib/librecsys_amd_stamps.so python tools/index_phase_stamps.py [--batch 65536]

Per kernel: average shader cycles between consecutive stamps of thread 0 of every block (the stamp BEFORE a barrier and the one
AFTER it separate a phase's own work from the wait for the block's slowest wave), block life times, and when blocks start and end
on the constant 100 MHz wall clock (first start = 0)."""
import argparse, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recsys-examples_amd")); sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
import mi355_native

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--batches", type=int, default=6, help="distinct batches run before the stamped step (300: the table is 3/4 full, "
                "new keys meet full buckets: the eviction regime)")
a = ap.parse_args()
dev = torch.device("cuda")
batches = bench.zipf_batches(a.rows, 0.99, a.batch, a.batches, dev)
module = bench.build_module(a.rows, 128, dev)
module.train()
grad = (torch.randn(a.batch, 128, device=dev) * 0.01).to(torch.bfloat16)
if a.batches <= 6:
    with torch.no_grad():
        for k, o in batches:
            module._forward_impl(k, o, train=True)
for k, o in batches:
    out, st = module._forward_impl(k, o, train=True)
    nu = int(st.uoff[-1])      # (read before the backward hands the step's buffer back)
    last = (k.cpu().numpy(), st.rev.cpu().numpy(), st.slots[:nu].cpu().numpy(), st.csr_cnt[:nu].cpu().numpy())
    module._backward_impl(st, grad)
torch.cuda.synchronize()
lib = ctypes.CDLL(mi355_native.LIB_PATH)

PROBE = ["start -> LDS init + key loads issued (sync)", "hash + mod + digest prefetch issue", "wait: barrier", "LDS dedup (CAS / count)",
         "wait: barrier", "partition hist + global atomic + first key-word load issue", "wait: barrier", "probe (key compare, scores, s_tab)",
         "wait: barrier", "records out", "per-occurrence outputs + init rows"]
PART = ["start -> record loads issued + LDS init", "wait: barrier", "merge (LDS hash insert + counts)", "wait: barrier",
        "deferred / hot counts / publish sums", "local scans", "look-back", "outputs", "-"]
SCAT = ["start -> index hops issued + bag range search", "wait: barrier", "bag marks + max-scan", "wait for index hops", "stores"]


SPANS = []


def dump(fn, nblk, nph, names, title, nlive=None):
    f = getattr(lib, fn, None)
    if f is None:
        print(f"{title}: no {fn} in this library (not a stamps build)")
        return
    buf = np.zeros((nblk, nph + 2), np.uint64)
    f.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    assert f(buf.ctypes.data, buf.nbytes) == 0
    live = buf[:, 0] != 0
    d = buf[live].astype(np.float64)
    blk = np.nonzero(live)[0]
    if d.shape[0] == 0:
        print(f"{title}: no stamps recorded")
        return
    print(f"== {title}: {d.shape[0]} blocks stamped")
    life = d[:, nph - 1] - d[:, 0]
    if names:
        for i, nm in enumerate(names):
            if i + 1 >= nph:
                break
            x = d[:, i + 1] - d[:, i]
            print(f"   {nm:62s} avg {x.mean():8.0f}  p50 {np.median(x):8.0f}  max {x.max():8.0f} cyc  ({100 * x.sum() / life.sum():5.1f} %)")
    print(f"   block life (shader cycles): avg {life.mean():.0f}  p50 {np.median(life):.0f}  max {life.max():.0f}")
    w0, w1 = d[:, nph], d[:, nph + 1]
    ok = w1 > 0
    recent = w0 > w0.max() - 6000        # (blocks only an earlier launch used keep their old stamps: drop what is > 60 us older)
    d, w0, w1, ok, life, blk = d[recent], w0[recent], w1[recent], ok[recent], life[recent], blk[recent]
    t0 = w0.min()
    SPANS.append((title.split(":")[0].split(" (")[0], w0.min() / 100.0, w1[ok].max() / 100.0))
    print(f"   wall clock (us, 100 MHz): starts {((w0 - t0) / 100).min():.2f} .. {((w0 - t0) / 100).max():.2f}  "
          f"ends p10 {np.percentile((w1[ok] - t0) / 100, 10):.2f}  p50 {np.median((w1[ok] - t0) / 100):.2f}  p90 {np.percentile((w1[ok] - t0) / 100, 90):.2f}  "
          f"max {((w1[ok] - t0) / 100).max():.2f};  block wall life avg {((w1[ok] - w0[ok]) / 100).mean():.2f} us"
          f"  -> {life[ok].mean() / ((w1[ok] - w0[ok]) / 100).mean() / 1e3:.2f} GHz")
    if not names:
        st = np.sort((w0 - t0) / 100)
        en = np.sort((w1[ok] - t0) / 100)
        qs = [0, 10, 25, 50, 75, 90, 100]
        print("   start percentiles (us):", " ".join(f"{np.percentile(st, q):.1f}" for q in qs))
        print("   end   percentiles (us):", " ".join(f"{np.percentile(en, q):.1f}" for q in qs))
    return blk[ok], (w1[ok] - t0) / 100, d[ok]


def partition_load(keys, rev, slots, cnt):
    """Per slot-range partition of the stamped step, rebuilt on the host from the step's own outputs (a partition is `spp`
    consecutive slots; the probe kernel cuts the batch into contiguous tiles of `tl` keys and emits one record per (tile, key)):
    (tile, key) records, CSR entries, records with more than 8 occurrences, unique rows, and the batch rank of its hottest key."""
    tb = module.table
    n, nu = len(keys), len(slots)
    lib.mi355_demb_forward_fused_partitions.argtypes = [ctypes.c_longlong] * 3
    P = lib.mi355_demb_forward_fused_partitions(n, 1, tb.num_buckets_)
    C = tb.bucket_capacity_
    spp = (-(-(tb.capacity_ + 1) // P) + C - 1) // C * C
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    tl = min(max((-(-n // ncu) + 63) // 64 * 64, 256), 2048 if n > ncu * 1024 else 1024)
    part_u = (slots // spp).astype(np.int64)
    assert (np.diff(part_u) >= 0).all(), "unique rows are not in partition order"
    pair, pc = np.unique((np.arange(n) // tl) * nu + rev, return_counts=True)      # one record per (tile, unique row)
    pp = part_u[pair % nu]
    rec = np.bincount(pp, minlength=P)
    ent = np.bincount(pp, weights=pc, minlength=P).astype(np.int64)
    big = np.bincount(pp, weights=pc > 8, minlength=P).astype(np.int64)
    uni = np.bincount(part_u, minlength=P)
    assert (ent == np.bincount(part_u, weights=cnt, minlength=P)).all()
    rank = np.empty(nu, np.int64)
    rank[np.argsort(-cnt, kind="stable")] = np.arange(1, nu + 1)
    top = np.full(P, nu + 1, np.int64)
    np.minimum.at(top, part_u, rank)
    return P, rec, ent, big, uni, top


def tail_report(blk, end, d, names, load):
    """the five partition blocks that end last, their load, and whether they are the owners of the batch's hottest keys"""
    P, rec, ent, big, uni, top = load
    print(f"   per partition: records mean {rec.mean():.0f} max {rec.max()}  entries mean {ent.mean():.0f} max {ent.max()}  "
          f"long records (> 8) mean {big.mean():.1f} max {big.max()}  unique rows mean {uni.mean():.0f} max {uni.max()}")
    last = np.argsort(-end)[:5]
    for i in last:
        p = blk[i]
        ph = np.diff(d[i, :len(names) + 1])
        j = int(np.argmax(ph / np.maximum(np.median(np.diff(d[:, :len(names) + 1], axis=1), axis=0), 1)))
        print(f"   partition {p:4d} ends {end[i]:6.2f} us: {rec[p]:5d} records {ent[p]:6d} entries {big[p]:4d} long {uni[p]:4d} unique, "
              f"hottest key rank {top[p]:5d}; phase furthest over its p50: '{names[j]}' {ph[j]:.0f} cyc")
    owners = set(np.argsort(top)[:5].tolist())
    print(f"   owners of the 5 hottest keys: {sorted(owners)}; of the 5 last-ending blocks {len(owners & set(blk[last].tolist()))} are among them; "
          f"corr(end, entries) {np.corrcoef(end, ent[blk])[0, 1]:.2f}  corr(end, records) {np.corrcoef(end, rec[blk])[0, 1]:.2f}  "
          f"corr(end, long records) {np.corrcoef(end, big[blk])[0, 1]:.2f}")


PROBE_C = ['start -> loads issued + LDS init + barrier 0', 'hash + bucket + digest prefetch issue + bag marks', 'wait: barrier A', 'LDS dedup (+ pair histogram) + bag scan half 1', 'wait: barrier B', 'reservation issued, reps, list starts, 2 key words issued, bag scan half 2', 'wait: barrier C', 'list starts, probe resolve, scores, reserved bases', 'wait: barrier D', '-', 'records + per-occurrence outputs']
if True:
    dump("mi355_debug_stamps_probe", 1024, 12, PROBE_C, "probe_c_kernel")
else:
    dump("mi355_debug_stamps_probe", 1024, 12, PROBE, "fused_probe_kernel")
if os.environ.get("MI355_FUSED_PART", "2") == "1":
    dump("mi355_debug_stamps_part", 1024, 10, PART, "fused_part_kernel")
    dump("mi355_debug_stamps_scatter", 2048, 6, SCAT, "csr_scatter_kernel")
PART2 = ["start -> record loads issued + LDS init", "wait: barrier", "merge (LDS hash insert + counts + rank bases out)", "wait: barrier",
         "entry scan + publish sums", "look-back", "outputs per unique row", "outputs per record (CSR entries <= 8)", "wait: barrier + long lists, hot-row tasks"]
PART_L = ["init + barrier", "merge pass", "wait: barrier", "eviction check, entry sums, block scan, publish", "look-back",
          "unique-row outputs (+ keys)", "wait: barrier", "output pass (CSR entries)", "tail", "-"]
EVICT = ["entry -> bucket lock taken", "re-probe of the bucket", "score scan: the lane's minimum + its eligibility",
         "group arg-min, lock / digest / score stores", "row initialisation issued", "(drain) + key published", "LDS hash insert, record, unlock",
         "rest of the pass (other keys)", "-"]
if os.environ.get("MI355_FUSED_PART", "2") != "1":
    dump("mi355_debug_stamps_evict", 1024, 10, EVICT, "part_evict: FIRST deferred key of every partition block that had one (any step so far)")
if False:
    dump("mi355_debug_stamps_part", 1024, 10, PART_L[:9], "part3_lean (partition role of the gather's launch)")
elif os.environ.get("MI355_FUSED_PART", "2") != "1":
    r = dump("mi355_debug_stamps_part", 1024, 10, PART2, "fused_part3_kernel")
    if r is not None and len(r[0]) > 1:
        tail_report(*r, PART2, partition_load(*last))
    dump("mi355_debug_stamps_fgather", 16384, 2, None, "gather_pooled_late_kernel (thread 0 of each block)")
dump("mi355_debug_stamps_gather", 16384, 2, None, "gather_pooled_pipe_kernel (thread 0 of each block)")
dump("mi355_debug_stamps_bwd", 16384, 2, None, "bwd_kernel (thread 0 of each block)")

print("== absolute wall clock of the last step (us): first block start .. last block end, and the gap to the previous kernel")
SPANS.sort(key=lambda x: x[1])
base = SPANS[0][1] if SPANS else 0
prev_end = None
for name, a0, a1 in SPANS:
    gap = "" if prev_end is None else f"   gap after previous: {a0 - prev_end:6.2f}"
    print(f"   {name:60s} {a0 - base:8.2f} .. {a1 - base:8.2f}{gap}")
    prev_end = a1
