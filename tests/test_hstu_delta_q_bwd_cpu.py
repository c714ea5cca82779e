"""The yardstick of the delta-q backward tests (tests/test_hstu_delta_q_bwd_gpu.py), pinned on the CPU.

A delta-q call (the queries of a sequence are the last Lq of its Lk keys) is the self-attention call on q padded with zero rows
in front, up to Lk rows per sequence: a zero query row contributes SiLU(0) = 0 everywhere.  So the oracle needs no delta-q
backward of its own -- `ho.hstu_attn_bwd` on (q_pad, dout_pad) gives dk / dv / drab as they are and dq in the last Lq rows.  Pinned
here: (1) the forward identity, exactly, for every mask kind; (2) the padded-oracle gradients against torch.autograd in float64 on
an independent dense restatement (einsum -> + rab -> * alpha -> SiLU -> / scaling -> mask -> einsum, the queries placed at the END
of the padded key axis as pad_input_delta_q of the reference's corelib/hstu/test.py places them)."""
import numpy as np
import pytest
import torch

from oracle import hstu_oracle as ho

LK = [70, 33, 1, 40]
LQ = [9, 33, 1, 0]
H, D = 2, 16
ALPHA, SCALE = 0.25, 70.0

MODES = {
    "causal": dict(causal=True),
    "full": dict(causal=False),
    "targets_g2": dict(causal=True, num_targets=np.array([6, 5, 1, 0]), target_group_size=2),
    "ctx_targets": dict(causal=True, num_targets=np.array([4, 3, 0, 0]), num_contextuals=np.array([3, 2, 1, 0]), target_group_size=1),
    "window_7_2": dict(local_window=(7, 2)),
    "rab": dict(causal=True, rab=True),
}


def _case(mode):
    rng = np.random.default_rng(len(mode))
    offq = np.concatenate([[0], np.cumsum(LQ)])
    offk = np.concatenate([[0], np.cumsum(LK)])
    q = rng.uniform(-1, 1, (offq[-1], H, D))
    k, v = rng.uniform(-1, 1, (offk[-1], H, D)), rng.uniform(-1, 1, (offk[-1], H, D))
    dout = rng.uniform(0, 1, (offq[-1], H, D))
    kw = dict(MODES[mode])
    if kw.get("rab"):
        kw["rab"] = rng.uniform(-1, 1, (len(LK), H, max(LK), max(LK)))
    return q, k, v, dout, offq, offk, kw


def pad_rows(x, offq, offk):
    """rows of x (per sequence Lq) moved to the END of that sequence's Lk rows, zeros in front"""
    out = np.zeros((int(offk[-1]),) + x.shape[1:], x.dtype)
    for b in range(len(offq) - 1):
        lq = int(offq[b + 1] - offq[b])
        out[int(offk[b + 1]) - lq:int(offk[b + 1])] = x[int(offq[b]):int(offq[b + 1])]
    return out


def unpad_rows(x, offq, offk):
    return np.concatenate([x[int(offk[b + 1]) - int(offq[b + 1] - offq[b]):int(offk[b + 1])] for b in range(len(offq) - 1)])


@pytest.mark.parametrize("mode", list(MODES))
def test_delta_q_forward_is_the_padded_self_attention_forward(mode):
    q, k, v, _, offq, offk, kw = _case(mode)
    dkw = {("window" if a == "local_window" else a): b for a, b in kw.items()}
    got = ho.hstu_attn_fwd_delta_q(q, k, v, offq, offk, ALPHA, SCALE, **dkw)
    want = unpad_rows(ho.hstu_attn_fwd(pad_rows(q, offq, offk), k, v, offk, ALPHA, SCALE, **kw), offq, offk)
    assert np.abs(got - want).max() == 0.0


def _dense_mask(Lk, b, kw):
    if "local_window" in kw:
        return ho.local_mask(Lk, *kw["local_window"])
    nt, nc = kw.get("num_targets"), kw.get("num_contextuals")
    return ho.valid_mask(Lk, kw.get("causal", True), None if nt is None else nt[b], None if nc is None else nc[b],
                         kw.get("target_group_size", 1))


@pytest.mark.parametrize("mode", list(MODES))
def test_padded_oracle_gradients_match_autograd_on_a_dense_restatement(mode):
    q, k, v, dout, offq, offk, kw = _case(mode)
    res = ho.hstu_attn_bwd(pad_rows(dout, offq, offk), pad_rows(q, offq, offk), k, v, offk, ALPHA, SCALE, **kw)
    dq_o, dk_o, dv_o = unpad_rows(res[0], offq, offk), res[1], res[2]
    # the dense restatement: [B, N, H, D] with the keys at the front of the padded axis and the queries at its end minus (N - Lk)
    B, N = len(LK), max(LK)
    tq, tk, tv = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (q, k, v))
    rab = torch.tensor(kw["rab"], dtype=torch.float64, requires_grad=True) if "rab" in kw else None
    Q = torch.zeros(B, N, H, D, dtype=torch.float64)
    K, V, DO = torch.zeros_like(Q), torch.zeros_like(Q), torch.zeros_like(Q)
    M = torch.zeros(B, 1, N, N, dtype=torch.float64)
    Qs, Ks, Vs = [], [], []
    for b in range(B):
        lq, lk = LQ[b], LK[b]
        Qs.append(torch.cat([torch.zeros(lk - lq, H, D, dtype=torch.float64), tq[offq[b]:offq[b + 1]], torch.zeros(N - lk, H, D, dtype=torch.float64)]))
        Ks.append(torch.cat([tk[offk[b]:offk[b + 1]], torch.zeros(N - lk, H, D, dtype=torch.float64)]))
        Vs.append(torch.cat([tv[offk[b]:offk[b + 1]], torch.zeros(N - lk, H, D, dtype=torch.float64)]))
        DO[b, lk - lq:lk] = torch.tensor(dout[offq[b]:offq[b + 1]])
        M[b, 0, lk - lq:lk, :lk] = torch.tensor(_dense_mask(lk, b, kw)[lk - lq:].astype(np.float64))
    Q, K, V = torch.stack(Qs), torch.stack(Ks), torch.stack(Vs)
    s = torch.einsum("bihd,bjhd->bhij", Q, K)
    if rab is not None:
        s = s + rab
    p = torch.nn.functional.silu(s * ALPHA) / SCALE * M
    out = torch.einsum("bhij,bjhd->bihd", p, V)
    grads = torch.autograd.grad(out, [tq, tk, tv] + ([rab] if rab is not None else []), DO)
    for got, want in ((dq_o, grads[0]), (dk_o, grads[1]), (dv_o, grads[2])):
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-10, atol=1e-300)
    if rab is not None:
        np.testing.assert_allclose(res[3], grads[3].numpy(), rtol=1e-10, atol=1e-300)
        for b in range(B):   # rows in front of the first query and everything outside the sequence: zero
            assert not res[3][b, :, :LK[b] - LQ[b]].any() and not res[3][b, :, LK[b]:].any() and not res[3][b, :, :, LK[b]:].any()
