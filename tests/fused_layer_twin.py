"""The fused HSTU layer restated in float64 torch, differentiated by autograd:

    xn = layer_norm(x; w_in, b_in)          z = xn @ W_uvqk + b_uvqk        a = silu(z)       u, v, q, k = split(a)
    o  = hstu_attention(q, k, v)            (silu(alpha q k^T) / scaling_seqlen under the mask, times v)
    t  = dropout(layer_norm(o; w_out, b_out) * u)                           out = t @ W_proj (+ x)

The attention mask of every sequence is oracle.hstu_oracle.valid_mask, laid out block-diagonally over the T tokens; the dropout
mask is norm_twin.keep_mask (mask 0 of this project's Philox stream), so training with dropout_ratio > 0 is exact.
`layer(...)` takes the functions that do the norm, the linear step and the SiLU, so that the same composition in a storage
dtype with torch's own ops (the tests' "native" layer) shares the masks and the data flow with the twin."""
from types import SimpleNamespace

import numpy as np
import torch

import norm_twin
from oracle.hstu_oracle import valid_mask

PARAMS = ("x", "w_uvqk", "b_uvqk", "w_proj", "w_in", "b_in", "w_out", "b_out")


def config(lengths, hidden, H, d, num_targets=None, num_contextuals=None, target_group_size=1, alpha=None, eps=1e-5, p=0.0,
           training=False, seed=0, residual=True, causal=True, learnable_input_norm=True):
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    max_seqlen = int(max(lengths)) if len(lengths) else 0
    return SimpleNamespace(lengths=list(lengths), offsets=offsets, T=int(offsets[-1]), B=len(lengths), hidden=hidden, H=H, d=d,
                           num_targets=num_targets, num_contextuals=num_contextuals, target_group_size=target_group_size,
                           alpha=1.0 / d ** 0.5 if alpha is None else alpha, eps=eps, p=p, training=training, seed=seed,
                           residual=residual, causal=causal, max_seqlen=max_seqlen, scaling_seqlen=max_seqlen,
                           learnable_input_norm=learnable_input_norm)


def make_params(cfg, seed=0):
    """float64 CPU tensors: O(1) activations, xavier-scaled weights, norm weights near 1"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    n = 4 * cfg.H * cfg.d
    p = {"x": r(cfg.T, cfg.hidden),
         "w_uvqk": r(cfg.hidden, n) * (2.0 / (cfg.hidden + n)) ** 0.5 * 2.0, "b_uvqk": 0.1 * r(n),
         "w_proj": r(cfg.H * cfg.d, cfg.hidden) * (2.0 / (cfg.H * cfg.d + cfg.hidden)) ** 0.5,
         "w_out": 1 + 0.1 * r(cfg.H * cfg.d), "b_out": 0.1 * r(cfg.H * cfg.d)}
    if cfg.learnable_input_norm:
        p["w_in"], p["b_in"] = 1 + 0.1 * r(cfg.hidden), 0.1 * r(cfg.hidden)
    else:
        p["w_in"] = p["b_in"] = None
    return p


def dense_mask(cfg):
    """bool [T, T]: token i sees token j (same sequence, the sequence's valid_mask)"""
    m = np.zeros((cfg.T, cfg.T), dtype=bool)
    for b in range(cfg.B):
        lo, hi = int(cfg.offsets[b]), int(cfg.offsets[b + 1])
        if hi > lo:
            m[lo:hi, lo:hi] = valid_mask(hi - lo, cfg.causal, None if cfg.num_targets is None else cfg.num_targets[b],
                                         None if cfg.num_contextuals is None else cfg.num_contextuals[b], cfg.target_group_size)
    return torch.from_numpy(m)


def dropout_factor(cfg):
    """float64 [T, H d]: keep / (1 - p), ones when nothing is dropped"""
    if not cfg.training or cfg.p == 0.0:
        return torch.ones(cfg.T, cfg.H * cfg.d, dtype=torch.float64)
    return norm_twin.keep_mask(cfg.seed, cfg.T, cfg.H * cfg.d, 0, cfg.p).double() / (1.0 - cfg.p)


def _ln64(x, w, b, eps):
    m = x.mean(1, keepdim=True)
    xh = (x - m) / torch.sqrt(((x - m) ** 2).mean(1, keepdim=True) + eps)
    return xh if w is None else xh * w + b


def _silu64(z):
    return z / (1.0 + torch.exp(-z))


def attention(q, k, v, mask, alpha, scaling_seqlen, silu=_silu64):
    """q, k, v [T, H, d], mask bool [T, T] -> [T, H, d]; dense over all tokens, the mask keeps the sequences apart"""
    s = torch.einsum("ihd,jhd->hij", q, k) * alpha
    p = silu(s) / scaling_seqlen * mask.to(s.dtype)
    return torch.einsum("hij,jhd->ihd", p, v)


def layer(p, cfg, mask, drop, ln=_ln64, linear=lambda x, w, b: x @ w if b is None else x @ w + b, silu=_silu64):
    """the layer's output for the parameter dict p; mask / drop on p's device, drop in p's dtype"""
    H, d = cfg.H, cfg.d
    xn = ln(p["x"], p["w_in"], p["b_in"], cfg.eps)
    a = silu(linear(xn, p["w_uvqk"], p["b_uvqk"]))
    u, v, q, k = a.split(H * d, dim=-1)
    o = attention(q.reshape(-1, H, d), k.reshape(-1, H, d), v.reshape(-1, H, d), mask, cfg.alpha, cfg.scaling_seqlen, silu)
    t = ln(o.reshape(-1, H * d), p["w_out"], p["b_out"], cfg.eps) * u * drop
    out = linear(t, p["w_proj"], None)
    return out + p["x"] if cfg.residual else out


def run(layer_fn, p, dout):
    """(out, {name: grad}) of layer_fn(p) for the upstream gradient dout; p's tensors are detached copies that require grad"""
    q = {k: (None if t is None else t.detach().clone().requires_grad_(True)) for k, t in p.items()}
    out = layer_fn(q)
    names = [k for k in PARAMS if q.get(k) is not None]
    grads = torch.autograd.grad(out, [q[k] for k in names], dout.to(out.dtype))
    return out.detach(), dict(zip(names, grads))


def twin(p64, cfg, dout):
    mask, drop = dense_mask(cfg), dropout_factor(cfg)
    return run(lambda q: layer(q, cfg, mask, drop), p64, dout.detach().cpu().double())
