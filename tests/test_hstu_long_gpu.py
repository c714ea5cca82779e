"""HSTU attention past 1 024 rows per sequence against the float64 oracle, forward AND backward, element by element.

Above 1 024 rows the library runs code the short tests never reach: hstu_fwd_q2_kernel (64 query rows per wave), K / V / P rings that
wrap dozens of times, paired row blocks and the column-major block map on dense batches, the backward's P / dS exchange with up to
72 x 72 tiles per (sequence, head) in its dense, triangular and chunked layouts, contextual rows, target groups and windows that cross
many 128-row blocks, key walks over dozens of cache pages.  The rest of the suite checks those paths against each other (bit
identity) or through properties; a bit-identity between sibling kernels holds whenever both share an error.  Here every element of
out / dq / dk / dv goes against oracle/hstu_oracle.py under the rule of tests/test_hstu_gpu.py, unchanged:

    |x - ref| <= 1e-3 |ref| + 1 ulp + k 2^-(bits + 2) mag        k = 2 (out), 4 (dq, dk, dv); bits = 7 (bf16), 10 (fp16)

with mag the accumulated magnitude of the element's summands (hstu_attn_magnitudes).  The rule bounds the rounding of each summand, so it
does not loosen with the length (tests/test_hstu_long_cpu.py: a bf16 emulation of the kernels' arithmetic uses half of it at 2 300 rows).

Inputs: numpy generators seeded from the case name; q, k, v uniform in (-1, 1), dout in (0, 1), rounded to the operand type before both
sides see them; alpha = d^-0.5, two heads.  The oracle's results are cached per case, shared by the tests that use the same inputs."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import hstu_oracle as ho
from test_hstu_gpu import _assert_drab, _close_elementwise, _run, _run_rab

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 2

# batch -> (lengths, contextual rows, targets, max_seqlen = scaling_seqlen or None for the longest sequence)
_BATCHES = {
    # both sides of the 1 024-row threshold, ragged ends that are no multiple of 32, an empty and a one-token sequence; 72 x 72 exchange
    # tiles; contextual rows (up to 200) and targets (up to 1 000) that cross 128-row blocks
    "jag": ([1025, 2300, 1, 0, 1536, 64, 1024, 129], [3, 200, 0, 0, 128, 5, 70, 1], [100, 1000, 1, 0, 7, 3, 500, 60], None),
    "short": ([1025, 1300, 1, 0, 64], [130, 5, 0, 0, 3], [300, 200, 1, 0, 10], None),
    # dense: B H = 8 columns of 16 row blocks, the last one ragged (1950 = 15 x 128 + 30): column-major map, paired row blocks
    "dense": ([1950] * 4, [200, 0, 130, 5], [1000, 300, 0, 64], None),
    # max_seqlen above every length (what a training configuration passes): the 64-row forward on short sequences, a grid of mostly
    # empty blocks, the exchange sized from 64 x 64 tiles
    "cfg_s": ([300, 1, 0, 129, 64, 77], [5, 0, 0, 9, 1, 2], [7, 1, 0, 20, 3, 0], 2048),
    "cfg_l": ([1100, 300, 1, 0, 129, 777], [70, 5, 0, 0, 1, 130], [500, 7, 1, 0, 60, 200], 2048),
}
# mode -> (causal, contexts and targets, target group size, window)
_MODES = {
    "causal": (True, False, 1, None),
    "noncausal": (False, False, 1, None),
    "ctx_targets": (True, True, 1, None),
    "tgt_groups": (True, "targets", 4, None),
    "ctx_targets_g2": (True, True, 2, None),
    "w300_0": (False, False, 1, (300, 0)),
    "w70_33": (False, False, 1, (70, 33)),
}


def _seed(name):
    return zlib.crc32(name.encode())


def _draw(rng, lo, hi, shape, tdt):
    """uniform in (lo, hi), rounded to the operand type: float32 numpy (what the oracle reads) holding values the type represents"""
    return torch.from_numpy(rng.uniform(lo, hi, shape).astype(np.float32)).to(tdt).float().numpy()


def _dev(x, tdt):
    return torch.from_numpy(x).to(DEV).to(tdt)


@functools.lru_cache(maxsize=None)
def _case(name):
    """"<batch>-d<head dim>-<mode>[-fp16]" -> inputs, oracle outputs, gradients and magnitudes (computed once per case)"""
    parts = name.split("-")
    batch, d, mode = parts[0], int(parts[1][1:]), parts[2]
    tdt = torch.float16 if parts[-1] == "fp16" else torch.bfloat16
    lengths, ctx, tgt, N = _BATCHES[batch]
    causal, ct, grp, window = _MODES[mode]
    lengths = np.asarray(lengths)
    N = int(lengths.max()) if N is None else N
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    T = int(off[-1])
    rng = np.random.default_rng(_seed(name))
    q, k, v = (_draw(rng, -1, 1, (T, H, d), tdt) for _ in range(3))
    dout = _draw(rng, 0, 1, (T, H, d), tdt)
    targets = np.asarray(tgt) if ct else None
    contexts = np.asarray(ctx) if ct is True else None
    if ct:
        assert (targets + (0 if contexts is None else contexts) <= lengths).all()
    alpha = d ** -0.5
    kw = dict(causal=causal, num_targets=targets, num_contextuals=contexts, target_group_size=grp, local_window=window)
    ref = (ho.hstu_attn_fwd(q, k, v, off, alpha, N, **kw),) + tuple(ho.hstu_attn_bwd(dout, q, k, v, off, alpha, N, **kw))
    mags = ho.hstu_attn_magnitudes(dout, q, k, v, off, alpha, N, **kw)
    for a in ref + tuple(mags):
        a.setflags(write=False)
    return SimpleNamespace(name=name, d=d, tdt=tdt, bits=10 if tdt == torch.float16 else 7, lengths=lengths, off=off, N=N, T=T, alpha=alpha,
                           causal=causal, targets=targets, contexts=contexts, grp=grp, window=window, q=q, k=k, v=v, dout=dout, ref=ref,
                           mags=mags)


def _gpu(c):
    """forward + backward of the case through hstu_attn_varlen_func (which sets the dense-batch hints): out, (dq, dk, dv)"""
    q, k, v, dout = (_dev(x, c.tdt) for x in (c.q, c.k, c.v, c.dout))
    out, grads = _run(q, k, v, c.off, c.N, c.targets, c.contexts, c.grp, c.causal, c.alpha, dout=dout, scaling=c.N, window=c.window)
    assert out.dtype == c.tdt and all(g.dtype == c.tdt for g in grads)
    return out.detach(), grads


def _check(c, out, grads):
    """every element of out, dq, dk, dv against the oracle"""
    for got, want, mag, kk in zip((out,) + tuple(grads), c.ref, c.mags, (2, 4, 4, 4)):
        assert got.shape == want.shape and float(got.float().abs().max()) > 0
        _close_elementwise(got, want, mag, kk, bits=c.bits)


@pytest.mark.parametrize("mode", ["causal", "noncausal", "ctx_targets", "tgt_groups", "w300_0", "w70_33"])
def test_long_jagged_batch_vs_oracle(mode):
    """d = 256 on sequences of 0 .. 2 300 rows: the 64-row forward (max_seqlen > 1 024) on long and short sequences of one batch, the
    exchange backward with 72 tiles a side (triangular layout under the plain causal mask, square otherwise), under every mask rule --
    contextual rows and targets crossing 128-row blocks, target groups, windows wider and narrower than a block."""
    c = _case(f"jag-d256-{mode}")
    _check(c, *_gpu(c))


@pytest.mark.parametrize("case", ["short-d64-causal", "short-d64-ctx_targets_g2", "short-d128-causal", "short-d128-ctx_targets_g2",
                                  "short-d256-causal-fp16"])
def test_generic_kernels_and_fp16_at_length_vs_oracle(case):
    """the one-kind kernels of head dims 64 and 128 and the fp16 build of the d = 256 ones, past 1 024 rows (fp16: an eighth of the bf16
    tolerance)"""
    c = _case(case)
    _check(c, *_gpu(c))


def test_rab_at_length_vs_oracle():
    """a relative bias routes d = 256 to the one-kind hstu_fwd_kernel and the bias backward: 1 100 rows, with drab (compared as the
    rab tests of tests/test_hstu_gpu.py compare it)"""
    name = "rab-d256-causal"
    rng = np.random.default_rng(_seed(name))
    lengths = np.array([1100, 1, 130])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    B, T, d, N = lengths.size, int(off[-1]), 256, int(lengths.max())
    tdt = torch.bfloat16
    q, k, v = (_draw(rng, -1, 1, (T, H, d), tdt) for _ in range(3))
    dout = _draw(rng, 0, 1, (T, H, d), tdt)
    rab = _draw(rng, -2, 2, (B, H, N, N), tdt)
    alpha = d ** -0.5
    out, grads, drab = _run_rab(*(_dev(x, tdt) for x in (q, k, v, rab)), off, N, None, None, 1, (-1, 0), alpha, _dev(dout, tdt))
    kw = dict(causal=True, rab=rab)
    ref = ho.hstu_attn_fwd(q, k, v, off, alpha, N, **kw)
    dq, dk, dv, dr = ho.hstu_attn_bwd(dout, q, k, v, off, alpha, N, **kw)
    mags = ho.hstu_attn_magnitudes(dout, q, k, v, off, alpha, N, **kw)
    for got, want, mag, kk in zip((out,) + tuple(grads), (ref, dq, dk, dv), mags, (2, 4, 4, 4)):
        _close_elementwise(got, want, mag, kk)
    _assert_drab(drab, dr)


@pytest.mark.parametrize("case", ["jag-d256-causal", "jag-d256-ctx_targets", "short-d64-causal"])
def test_exchange_layouts_at_length(case, monkeypatch):
    """The three layouts of the backward's P / dS exchange at length: dense (the default here) against the oracle; chunked under a cap
    that holds two units of the longest sequence (jagged layout: xch_tile per sequence, triangular qg (qg + 1) / 2 + kg under the plain
    causal mask, the chunk plan) and none at all (the recomputing passes) bit for bit equal to the dense one."""
    import hstu.hstu_attn_interface as hi

    c = _case(case)
    L = hi.lib()
    B = c.lengths.size
    dense = L.mi355_hstu_attn_bwd_ds_bytes(B, H, c.d, c.N)
    assert dense > 0
    monkeypatch.setattr(hi, "_DS_MAX_BYTES", max(dense, 4 << 30))
    out, g_dense = _gpu(c)
    _check(c, out, g_dense)
    ng = (c.N + 31) // 32
    tri = c.causal and c.contexts is None
    umax = ng * (ng + 1) // 2 if tri else ng * ng
    regions = 2 if c.d >= 128 else 1
    cap = 4096 + regions * int(2.3 * umax) * 2048
    capped = L.mi355_hstu_attn_bwd_ds_bytes_capped(B, H, c.d, c.N, c.T, cap, int(tri))
    assert 0 < capped <= cap < dense
    for limit, label in ((cap, "in chunks"), (0, "recomputing")):
        monkeypatch.setattr(hi, "_DS_MAX_BYTES", limit)
        o, g = _gpu(c)
        assert torch.equal(o, out)
        for a, b, t in zip(g, g_dense, ("dq", "dk", "dv")):
            assert torch.equal(a, b), f"{label}: {t} differs from the dense exchange by {(a.float() - b.float()).abs().max().item()}"


@pytest.mark.parametrize("case", ["dense-d256-causal", "dense-d256-ctx_targets", "dense-d64-causal"])
def test_dense_long_batch_vs_oracle(case):
    """every length == max_seqlen, B H = 8 columns of 16 row blocks: the column-major block map in the forward and in every backward
    launch, (heavy, light) row-block pairs in the d = 256 forward, a ragged last block -- all eight columns, every element"""
    c = _case(case)
    assert (c.lengths == c.N).all() and (c.lengths.size * H) % 8 == 0 and (c.N + 127) // 128 >= 16 and c.N % 128
    _check(c, *_gpu(c))


@pytest.mark.parametrize("case", ["cfg_s-d256-causal", "cfg_s-d256-ctx_targets", "cfg_l-d256-causal", "cfg_l-d256-ctx_targets",
                                  "cfg_l-d64-causal", "cfg_l-d64-ctx_targets"])
def test_max_seqlen_above_every_length_vs_oracle(case):
    """max_seqlen = scaling_seqlen = 2 048 over sequences of at most 300 / 1 100 rows: kernels, grid and exchange follow max_seqlen"""
    c = _case(case)
    assert c.N == 2048 and c.lengths.max() < c.N
    _check(c, *_gpu(c))


@pytest.mark.parametrize("d", [64, 256])
def test_delta_q_and_paged_keys_past_1024_vs_oracle(d):
    """inference forward over 1 500 / 0 / 1 037 cached keys + 40 new history rows + ~30 candidates per sequence: (a) contiguous keys
    (delta-q), (b) the same keys walked through 32-token pages in a random order, the new history written by append_kvcache -- both
    against the oracle element by element (hstu_attn_magnitudes_delta_q)"""
    from hstu import append_kvcache, hstu_attn_varlen_func

    rng = np.random.default_rng(_seed(f"paged-d{d}"))
    B, P, tdt = 3, 32, torch.bfloat16
    old, new_hist, num_cand = np.array([1500, 0, 1037]), np.array([40, 40, 40]), np.array([30, 27, 33])
    qlen, cachelen = new_hist + num_cand, old + new_hist
    klen = cachelen + num_cand
    q_off = np.concatenate([[0], np.cumsum(qlen)]).astype(np.int32)
    k_off = np.concatenate([[0], np.cumsum(klen)]).astype(np.int32)
    o_off = np.concatenate([[0], np.cumsum(old)])
    T = int(q_off[-1])
    qn, k_new, v_new = (_draw(rng, -1, 1, (T, H, d), tdt) for _ in range(3))       # [new history | candidates] per sequence
    k_old, v_old = (_draw(rng, -1, 1, (int(old.sum()), H, d), tdt) for _ in range(2))
    full = lambda o, n: np.concatenate([x for b in range(B) for x in (o[o_off[b]:o_off[b + 1]], n[q_off[b]:q_off[b + 1]])])
    k_full, v_full = full(k_old, k_new), full(v_old, v_new)
    alpha, scaling = d ** -0.5, float(klen.max())
    ref = ho.hstu_attn_fwd_delta_q(qn, k_full, v_full, q_off, k_off, alpha, scaling, True, num_cand)
    mag = ho.hstu_attn_magnitudes_delta_q(qn, k_full, v_full, q_off, k_off, alpha, scaling, True, num_cand)
    ti = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(DEV)
    q, kn, vn = (_dev(x, tdt) for x in (qn, k_new, v_new))
    out_a = hstu_attn_varlen_func(q, _dev(k_full, tdt), _dev(v_full, tdt), ti(q_off), ti(k_off), None, None, int(qlen.max()),
                                  int(klen.max()), scaling, None, ti(num_cand), window_size=(-1, 0), alpha=alpha)
    _close_elementwise(out_a, ref, mag, 2)
    # (b) paged: the old history written page by page, the new history appended with append_kvcache
    npg = (cachelen + P - 1) // P
    assert npg.max() >= 40
    perm = rng.permutation(int(npg.sum()) + 3)[:int(npg.sum())]
    page_off = np.concatenate([[0], np.cumsum(npg)])
    last = cachelen - (npg - 1) * P
    cache = torch.zeros(int(npg.sum()) + 3, 2, P, H, d, dtype=tdt, device=DEV)
    for b in range(B):
        j = np.arange(int(old[b]))
        pg = torch.from_numpy(perm[page_off[b] + j // P]).to(DEV)
        slot = torch.from_numpy(j % P).to(DEV)
        cache[:, 0][pg, slot] = _dev(k_old[o_off[b]:o_off[b + 1]], tdt)
        cache[:, 1][pg, slot] = _dev(v_old[o_off[b]:o_off[b + 1]], tdt)
    batch_idx = np.repeat(np.arange(B), new_hist)
    positions = np.concatenate([old[b] + np.arange(new_hist[b]) for b in range(B)])
    cand_off = np.concatenate([[0], np.cumsum(num_cand)])
    append_kvcache(kn, vn, ti(batch_idx), ti(positions), ti(cand_off), ti([int(new_hist.sum())]), 0, cache, ti(perm), ti(page_off),
                   ti(last), 0)
    kc, vc, koff = ho.gather_paged_kv(k_new, v_new, q_off, num_cand, cache.float().cpu().numpy(), page_off, perm, last)
    np.testing.assert_array_equal(kc, k_full)          # append_kvcache put every token where the walk finds it
    np.testing.assert_array_equal(vc, v_full)
    np.testing.assert_array_equal(koff, k_off)
    out_b = hstu_attn_varlen_func(q, kn, vn, ti(q_off), ti(k_off), None, None, int(qlen.max()), int(klen.max()), scaling, None,
                                  ti(num_cand), window_size=(-1, 0), alpha=alpha, kv_cache=cache, page_offsets=ti(page_off),
                                  page_ids=ti(perm), last_page_lens=ti(last))
    _close_elementwise(out_b, ref, mag, 2)
    assert torch.equal(out_a, out_b)                    # same keys, same order of operations
