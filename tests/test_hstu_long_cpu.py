"""CPU side of tests/test_hstu_long_gpu.py: the element-wise rule those tests hold the long-sequence kernels to can be met, shown
without a GPU -- a bf16 emulation of the kernels' arithmetic (S in fp32, P and dS rounded to bf16, fp32 accumulation, bf16 outputs)
passes `_close_elementwise` with the same k at 2 300 rows -- and the oracle's delta-q magnitudes are those of the training call where
the two coincide."""
import zlib

import numpy as np
import pytest
import torch

from oracle import hstu_oracle as ho
from test_hstu_gpu import _close_elementwise


def _inputs(name, T, H, d):
    """q, k, v uniform in (-1, 1), dout in (0, 1), rounded to bf16 (float32 tensors holding bf16 values)"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    mk = lambda lo, hi: torch.from_numpy(rng.uniform(lo, hi, (T, H, d)).astype(np.float32)).bfloat16().float()
    return mk(-1, 1), mk(-1, 1), mk(-1, 1), mk(0, 1)


def _bf16_emulation(q, k, v, dout, off, alpha, scaling, targets, ctx, grp):
    """The kernels' arithmetic on the CPU: bf16 operands, S = q k^T and dP = dO v^T accumulated in fp32, P and dS rounded to bf16 in
    front of the second GEMMs, fp32 accumulation there, outputs rounded to bf16."""
    r16 = lambda t: t.bfloat16().float()
    out, dq, dk, dv = (torch.zeros_like(q) for _ in range(4))
    for b in range(len(off) - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        if hi == lo:
            continue
        m = torch.from_numpy(ho.valid_mask(hi - lo, True, None if targets is None else targets[b], None if ctx is None else ctx[b],
                                           grp)).float()
        for h in range(q.shape[1]):
            qs, ks, vs, ds_ = q[lo:hi, h], k[lo:hi, h], v[lo:hi, h], dout[lo:hi, h]
            s = alpha * (qs @ ks.T)
            sig = torch.sigmoid(s)
            p = r16(s * sig / scaling * m)
            dsc = r16((ds_ @ vs.T) * m * (sig * (1 + s * (1 - sig))) * (alpha / scaling))
            out[lo:hi, h] = r16(p @ vs)
            dv[lo:hi, h] = r16(p.T @ ds_)
            dq[lo:hi, h] = r16(dsc @ ks)
            dk[lo:hi, h] = r16(dsc.T @ qs)
    return out, dq, dk, dv


@pytest.mark.parametrize("case", ["causal_2300", "ctx_targets_1100"])
def test_bf16_emulation_meets_the_elementwise_rule_at_length(case):
    """(the rule bounds the rounding of every summand, so it does not loosen with the length: 2 300 rows use about half of the
    output's band and less than half of the gradients')"""
    H, d = 2, 256
    if case == "causal_2300":
        lengths, targets, ctx, grp = [2300], None, None, 1
    else:   # contextual rows and targets that both cross 128-row blocks, groups of 4
        lengths, targets, ctx, grp = [1100, 129], np.array([500, 60]), np.array([200, 1]), 4
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    N = int(max(lengths))
    q, k, v, dout = _inputs(case, int(off[-1]), H, d)
    alpha = d ** -0.5
    got = _bf16_emulation(q, k, v, dout, off, alpha, float(N), targets, ctx, grp)
    qn, kn, vn, dn = (t.numpy() for t in (q, k, v, dout))
    ref = (ho.hstu_attn_fwd(qn, kn, vn, off, alpha, N, True, targets, ctx, grp),) + tuple(
        ho.hstu_attn_bwd(dn, qn, kn, vn, off, alpha, N, True, targets, ctx, grp))
    mags = ho.hstu_attn_magnitudes(dn, qn, kn, vn, off, alpha, N, True, targets, ctx, grp)
    for x, want, mag, kk in zip(got, ref, mags, (2, 4, 4, 4)):
        assert float(x.abs().max()) > 0
        _close_elementwise(x, want, mag, kk)


@pytest.mark.parametrize("mode", ["causal", "ctx_targets", "noncausal", "window", "rab"])
def test_delta_q_magnitudes_equal_the_training_magnitudes_when_every_key_has_a_query(mode):
    rng = np.random.default_rng(zlib.crc32(mode.encode()))
    lengths = np.array([70, 1, 0, 33])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    T, H, d, N = int(off[-1]), 2, 32, 70
    q, k, v = (rng.uniform(-1, 1, (T, H, d)) for _ in range(3))
    kw, kwd = {}, {}
    if mode == "ctx_targets":
        kw = dict(num_targets=np.array([9, 0, 0, 5]), num_contextuals=np.array([3, 1, 0, 0]), target_group_size=2)
    elif mode == "noncausal":
        kw = dict(causal=False)
    elif mode == "window":
        kw, kwd = dict(local_window=(9, 4)), dict(window=(9, 4))
    elif mode == "rab":
        kw = dict(rab=rng.uniform(-2, 2, (lengths.size, H, N, N)))
    want = ho.hstu_attn_magnitudes(None, q, k, v, off, 0.2, N, **kw)[0]
    kw.pop("local_window", None)
    got = ho.hstu_attn_magnitudes_delta_q(q, k, v, off, off, 0.2, N, **kw, **kwd)
    np.testing.assert_array_equal(got, want)
    assert want.max() > 0
