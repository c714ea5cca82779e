"""Loop twin of the seven FBGEMM jagged ops of fbgemm_jagged_ops: every output element is produced by a Python loop and one
indexing statement, straight from the semantics of the ops (no cumsum, no gather, no where).  Tensors go in and come out
on the CPU; the tests move GPU results over before comparing with torch.equal."""
import torch

_WRAP = {torch.int32: 32, torch.int64: 64}


def _wrap(x: int, dtype) -> int:
    """x as the two's-complement integer of `dtype` (torch.cumsum wraps)"""
    bits = _WRAP[dtype]
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def _scan_row(row, dtype, mode):
    vals = [int(v) for v in row.tolist()]
    out, run = ([0] if mode == "complete" else []), 0
    for v in vals:
        if mode == "exclusive":
            out.append(_wrap(run, dtype))
        run += v
        if mode != "exclusive":
            out.append(_wrap(run, dtype))
    return out


def cumsum(t: torch.Tensor, mode: str) -> torch.Tensor:
    """mode: complete ([..., N] -> [..., N + 1], leading zero), inclusive, exclusive"""
    t = t.cpu()
    if t.dim() == 2:
        assert mode == "complete"
        return torch.tensor([_scan_row(r, t.dtype, mode) for r in t], dtype=t.dtype).reshape(t.size(0), t.size(1) + 1)
    return torch.tensor(_scan_row(t, t.dtype, mode), dtype=t.dtype)


def jagged_to_padded_dense(values: torch.Tensor, offsets: torch.Tensor, max_len: int, padding_value=0.0) -> torch.Tensor:
    """values [T, D] or [T] -> [B, max_len, D] or [B, max_len]"""
    values, off = values.cpu(), [int(o) for o in offsets.tolist()]
    B = len(off) - 1
    out = torch.full((B, max_len) + tuple(values.shape[1:]), padding_value, dtype=values.dtype)
    for b in range(B):
        for pos in range(min(off[b + 1] - off[b], max_len)):
            out[b, pos] = values[off[b] + pos]
    return out


def dense_to_jagged(dense: torch.Tensor, offsets: torch.Tensor, total_L=None) -> torch.Tensor:
    """dense [B, N, D] or [B, N] -> [total, D] or [total]; rows past N of a long sample and rows of no sample are zeros"""
    dense, off = dense.cpu(), [int(o) for o in offsets.tolist()]
    B, N = dense.size(0), dense.size(1)
    total = off[-1] if total_L is None else total_L
    out = torch.zeros((total,) + tuple(dense.shape[2:]), dtype=dense.dtype)
    for b in range(B):
        for pos in range(min(off[b + 1] - off[b], N)):
            if off[b] + pos < total:
                out[off[b] + pos] = dense[b, pos]
    return out


def jagged_to_padded_dense_grad(grad_out: torch.Tensor, offsets: torch.Tensor, rows: int) -> torch.Tensor:
    """adjoint of jagged_to_padded_dense in the values: value row off[b] + pos receives grad_out[b, pos]; truncated rows and
    rows of no sample receive nothing"""
    grad_out, off = grad_out.cpu(), [int(o) for o in offsets.tolist()]
    B, N = grad_out.size(0), grad_out.size(1)
    g = torch.zeros((rows,) + tuple(grad_out.shape[2:]), dtype=grad_out.dtype)
    for b in range(B):
        for pos in range(min(off[b + 1] - off[b], N)):
            g[off[b] + pos] = grad_out[b, pos]
    return g


def dense_to_jagged_grad(grad_values: torch.Tensor, offsets: torch.Tensor, B: int, N: int) -> torch.Tensor:
    """adjoint of dense_to_jagged in dense: dense[b, pos] receives grad_values[off[b] + pos]; padded positions nothing"""
    grad_values, off = grad_values.cpu(), [int(o) for o in offsets.tolist()]
    g = torch.zeros((B, N) + tuple(grad_values.shape[1:]), dtype=grad_values.dtype)
    for b in range(B):
        for pos in range(min(off[b + 1] - off[b], N)):
            if off[b] + pos < grad_values.size(0):
                g[b, pos] = grad_values[off[b] + pos]
    return g


def keyed_jagged_index_select_dim1(values, lengths, offsets, indices, batch_size, weights=None):
    """[values, lengths] or [values, lengths, weights]: output bag (f, j) is input bag (f, indices[j]); an index outside
    [0, batch_size) gives an empty bag"""
    values, lengths = values.cpu(), lengths.cpu()
    weights = None if weights is None else weights.cpu()
    off, idx, B = [int(o) for o in offsets.tolist()], [int(i) for i in indices.tolist()], batch_size
    F = lengths.numel() // B if B else 0
    out_lengths, src = [], []
    for f in range(F):
        for i in idx:
            n = int(lengths[f * B + i]) if 0 <= i < B else 0
            out_lengths.append(n)
            src.extend(range(off[f * B + i], off[f * B + i] + n) if n else [])
    out_values = torch.empty(len(src), dtype=values.dtype)
    out_weights = None if weights is None else torch.empty(len(src), dtype=weights.dtype)
    for k, s in enumerate(src):
        out_values[k] = values[s]
        if weights is not None:
            out_weights[k] = weights[s]
    out = [out_values, torch.tensor(out_lengths, dtype=lengths.dtype).reshape(-1)]
    return out if weights is None else out + [out_weights]
