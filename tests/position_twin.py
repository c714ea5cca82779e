"""CPU restatement of the HSTU positional encoder's arithmetic in float64 and plain torch, for the tests of hstu_position:
the row -> table-row index maps, the two forward sums, the per-table-row gradient sums with the figures an error bound needs
(number of terms and sum of magnitudes per element), a per-sample split of a jagged tensor, and a generator of timestamps
whose time buckets do not depend on the last bits of sqrt / log.  Written from the specification in include/recsys_amd.h."""
import torch

NUM_TIME_BUCKETS = 2048
TIME_BUCKET_INCREMENTS = 60.0
MARGIN = 0.05  # least distance of a generated bucket value to a bucket boundary


def _seq_of_rows(offsets):
    """(sequence b, row n inside it) of every row of a jagged tensor with these offsets"""
    offsets = offsets.to(torch.int64).cpu()
    lengths = offsets[1:] - offsets[:-1]
    b = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    n = torch.arange(int(offsets[-1])) - offsets[:-1][b]
    return b, n


def position_index(offsets, high_inds, K, ind_offsets=None):
    """table row of every jagged row: min(n + ind_offset, high) where n + ind_offset >= high, clamped into [0, K - 1]"""
    b, n = _seq_of_rows(offsets)
    high = high_inds.to(torch.int64).cpu()[b]
    i = n if ind_offsets is None else n + ind_offsets.to(torch.int64).cpu()[b]
    return torch.where(i >= high, high, i).clamp(0, K - 1)


def add_position_embeddings(jagged, offsets, high_inds, dense, scale=1.0, ind_offsets=None):
    """(out, |jagged * scale| + |dense row|) in float64; the scale is the fp32 value the kernel receives"""
    idx = position_index(offsets, high_inds, dense.size(0), ind_offsets)
    s = float(torch.tensor(scale, dtype=torch.float32))
    a = jagged.detach().cpu().double() * s
    d = dense.detach().cpu().double()[idx]
    return a + d, a.abs() + d.abs()


def rows_sum(d_out, idx, K):
    """per table row k: (sum of d_out rows with idx == k, sum of their magnitudes, their number M), float64"""
    g = d_out.detach().cpu().double()
    total = torch.zeros(K, g.size(1), dtype=torch.float64).index_add_(0, idx, g)
    mags = torch.zeros(K, g.size(1), dtype=torch.float64).index_add_(0, idx, g.abs())
    count = torch.zeros(K, dtype=torch.float64).index_add_(0, idx, torch.ones(idx.numel(), dtype=torch.float64))
    return total, mags, count


def timestamp_position_index(offsets, lengths, num_targets, interleave_targets, max_contextual_seq_len, Np):
    b, n = _seq_of_rows(offsets)
    high = lengths.to(torch.int64).cpu()
    if num_targets is not None:
        high = high - num_targets.to(torch.int64).cpu() * (2 if interleave_targets else 1)
    high = high[b]
    p = high - torch.minimum(n, high) + max_contextual_seq_len
    p = p.clamp(max=Np - 1)
    p = torch.where(n < max_contextual_seq_len, n, p)
    return p.clamp(0, Np - 1)


def time_deltas(offsets, timestamps, time_delta=0):
    """time from every row to the last row of its sequence"""
    b, _ = _seq_of_rows(offsets)
    ts = timestamps.to(torch.int64).cpu()
    return ts[offsets.to(torch.int64).cpu()[1:][b] - 1] - ts + time_delta


def bucket_value(dt, fn, increments=TIME_BUCKET_INCREMENTS, scale=1.0, dtype=torch.float64):
    """the real number whose integer part is the time bucket, evaluated in `dtype`"""
    x = dt.to(dtype).clamp(min=1e-6) / torch.tensor(increments, dtype=dtype)
    x = torch.sqrt(x) if fn == "sqrt" else torch.log(x)
    return x * torch.tensor(scale, dtype=dtype)


def time_bucket(dt, fn, num_time_buckets=NUM_TIME_BUCKETS, dtype=torch.float64):
    return torch.trunc(bucket_value(dt, fn, dtype=dtype)).clamp(0, num_time_buckets).to(torch.int64)


def buckets_are_safe(dt, fn, num_time_buckets=NUM_TIME_BUCKETS):
    """True where the bucket value keeps MARGIN from every boundary 1 .. num_time_buckets, so that fp32 and fp64 agree"""
    v = bucket_value(dt, fn)
    frac = v - torch.floor(v)
    return (v <= 1 - MARGIN) | (v >= num_time_buckets + MARGIN) | ((frac >= MARGIN) & (frac <= 1 - MARGIN))


def make_timestamps(offsets, fn, seed, recent=None):
    """int64 timestamps [N]: the last row of every sequence has dt = 0, the others a dt whose bucket value keeps MARGIN from
    every bucket boundary; the second row of a sequence lies AFTER its last (negative dt, bucket 0) and the third far in the
    past (sqrt: beyond the last bucket).  recent = (b, count): `count` rows of sequence b fall inside bucket 0."""
    g = torch.Generator().manual_seed(seed)
    b, n = _seq_of_rows(offsets)
    rows = b.numel()
    v = torch.randint(0, 300 if fn == "sqrt" else 12, (rows,), generator=g).double() \
        + 0.1 + 0.8 * torch.rand(rows, generator=g, dtype=torch.float64)
    dt = torch.round(60.0 * (v * v if fn == "sqrt" else torch.exp(v))).to(torch.int64)
    dt[~buckets_are_safe(dt, fn)] = 0
    dt[n == 1] = -7
    dt[n == 2] = 300_000_000 if fn == "sqrt" else 45
    if recent is not None:
        rb, count = recent
        pick = (b == rb) & (n < count)
        dt[pick] = torch.randint(0, 55, (int(pick.sum()),), generator=g)
    off = offsets.to(torch.int64).cpu()
    last = off[1:][b] - 1
    dt[torch.arange(rows) == last] = 0
    assert bool(buckets_are_safe(dt, fn).all())
    return 1_700_000_000 - dt


def add_timestamp_position_embeddings(seq, pos_emb, ts_emb, p, t):
    """float64 value of seq + (pos_emb[p] + ts_emb[t]) (the roundings are the kernel's business)"""
    return seq.detach().cpu().double() + pos_emb.detach().cpu().double()[p] + ts_emb.detach().cpu().double()[t]


def split_rows(offsets_a, offsets_b):
    """row indices of the merged tensor that make up part A and part B, sample by sample"""
    oa, ob = offsets_a.to(torch.int64).cpu(), offsets_b.to(torch.int64).cpu()
    ia, ib = [], []
    for i in range(oa.numel() - 1):
        la, lb = int(oa[i + 1] - oa[i]), int(ob[i + 1] - ob[i])
        start = int(oa[i] + ob[i])
        ia.extend(range(start, start + la))
        ib.extend(range(start + la, start + la + lb))
    return torch.tensor(ia, dtype=torch.int64), torch.tensor(ib, dtype=torch.int64)


def unit_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}[dtype]


def ulp(x, dtype):
    """spacing of `dtype` at the magnitudes of x (float64 in, float64 out)"""
    _, e = torch.frexp(x.double().abs())
    return torch.ldexp(torch.full_like(x, unit_roundoff(dtype), dtype=torch.float64), e)

