"""Beam-search decode attention of the semantic-ID generative-retrieval family on MI355X.

`beam_decode_attn` has the signature, defaults and return value of the reference's
`corelib/gr_decode_atten/interface.py` (beam_decode_attn / BeamDecodeAttn); the work is done by
`mi355_beam_decode_attn` (csrc/beam_decode.hip): a flash-decoding context kernel on the MFMA with split-KV and GQA packing,
and a beam kernel that gathers the top-k beam rows and merges everything by log-sum-exp.  Forward only.

    q:            [B, 1, W, Hq, D]                 bf16 / fp16
    k/v_context:  [B, Sk, Hkv, D] (any batch / row / head strides), or [total_k, Hkv, D] with cu_seqlens_k [B + 1]
    k/v_beam:     [B, decode_nums * W, Hkv, D]
    topk_indices: [B, 1, Hq, max_decode_nums, W]   int32 / int64 (heads of a GQA group share the indices of its first head)
    out:          [B, 1, W, Hq, D]  dtype of q;    lse: [B, 1, W, Hq]  fp32

Both backend names of the reference ("dsl", "3kernel") run the one path here, and `seqused_k` / `cu_seqlens_k` work with
either.  There is no eager fallback: without the library or a GPU the call raises.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

import mi355_native as N
from mi355_native import rows_aligned as _rows_aligned

KEY_TILE = 64      # keys per tile of the context kernel (csrc/softmax_tile_dev.h: kSmKeys)
ROW_TILE = 128     # packed query rows (beam x group head) per workgroup (kSmRows)
NUM_CUS = 256
# Split rule, read off the _num_splits sweep of profiles/beam_decode_bench.txt: split until the launch has as many
# workgroups as the CUs hold at once (the context kernel runs one workgroup per CU at D = 128, where a wave takes 247 VGPRs,
# and two at D = 64), but keep at least SPLIT_MIN_TILES key tiles in a split: below that the partials' round trip and the
# merge cost more than the split gains.
SPLIT_MIN_TILES = 4


def _blocks_per_cu(D: int) -> int:
    return 2 if D <= 64 else 1


_BACKENDS = ("dsl", "3kernel")


class BeamDecodeError(N.NativeError, ValueError):
    """An argument the kernels cannot take.  Both a NativeError (like every refusal of this package) and a ValueError."""


def num_splits(B: int, W: int, Hq: int, Hkv: int, D: int, Sk_max: int) -> int:
    """KV splits of the context kernel for a launch on 256 CUs: 1 when the grid already fills them, never more than the
    number of key tiles (no split is empty for the longest sample), never 0."""
    tiles = -(-max(int(Sk_max), 0) // KEY_TILE)
    if tiles <= 1:
        return 1
    G = max(Hq // max(Hkv, 1), 1)
    blocks = max(B * Hkv * -(-(W * G) // ROW_TILE), 1)
    if blocks >= NUM_CUS:
        return 1
    want = -(-(NUM_CUS * _blocks_per_cu(D)) // blocks)
    return max(1, min(want, tiles // SPLIT_MIN_TILES, tiles))


def _validate_inputs(q, k_context, v_context, k_beam, v_beam, topk_indices, decode_nums, jagged_k_context=False):
    def bad(msg):
        raise BeamDecodeError(msg)

    for name, t in (("q", q), ("k_context", k_context), ("v_context", v_context), ("k_beam", k_beam), ("v_beam", v_beam),
                    ("topk_indices", topk_indices)):
        if not isinstance(t, torch.Tensor):
            bad(f"{name} must be a tensor, got {type(t).__name__}")
    if q.dim() != 5:
        bad(f"q must be 5-D [B, Sq, W, Hq, D], got shape {tuple(q.shape)}")
    batch, seqlen_q, beam_width, head_q, dim = q.shape
    if jagged_k_context:
        if k_context.dim() != 3:
            bad(f"k_context must be 3-D [total_k, Hkv, D] in jagged mode, got shape {tuple(k_context.shape)}")
        head_kv = k_context.shape[1]
    else:
        if k_context.dim() != 4:
            bad(f"k_context must be 4-D [B, Sk, Hkv, D], got shape {tuple(k_context.shape)}")
        if k_context.shape[0] != batch:
            bad(f"k_context batch: expected {batch}, got shape {tuple(k_context.shape)}")
        head_kv = k_context.shape[2]
    if v_context.shape != k_context.shape:
        bad(f"v_context shape {tuple(v_context.shape)} differs from k_context shape {tuple(k_context.shape)}")
    if k_context.shape[-1] != dim:
        bad(f"k_context head dim: expected {dim}, got shape {tuple(k_context.shape)}")
    if not isinstance(decode_nums, int) or decode_nums < 0:
        bad(f"decode_nums must be a non-negative int, got {decode_nums!r}")
    want = (batch, decode_nums * beam_width, head_kv, dim)
    if tuple(k_beam.shape) != want:
        bad(f"k_beam shape: expected {want}, got {tuple(k_beam.shape)}")
    if v_beam.shape != k_beam.shape:
        bad(f"v_beam shape {tuple(v_beam.shape)} differs from k_beam shape {tuple(k_beam.shape)}")
    if topk_indices.dim() != 5 or tuple(topk_indices.shape[:3]) != (batch, seqlen_q, head_q) or \
            topk_indices.shape[4] != beam_width:
        bad(f"topk_indices must be [B={batch}, Sq={seqlen_q}, Hq={head_q}, max_decode_nums, W={beam_width}], "
            f"got shape {tuple(topk_indices.shape)}")
    if decode_nums > topk_indices.shape[3]:
        bad(f"decode_nums {decode_nums} exceeds max_decode_nums of topk_indices shape {tuple(topk_indices.shape)}")
    if head_kv == 0 or head_q % head_kv != 0:
        bad(f"head_q {head_q} is no multiple of head_kv {head_kv}")
    if q.dtype not in (torch.float16, torch.bfloat16):
        bad(f"q must be fp16 or bf16, got {q.dtype}")
    if not (q.dtype == k_context.dtype == v_context.dtype == k_beam.dtype == v_beam.dtype):
        bad(f"q / k / v dtypes differ: {q.dtype}, {k_context.dtype}, {v_context.dtype}, {k_beam.dtype}, {v_beam.dtype}")
    if topk_indices.dtype not in (torch.int32, torch.int64):
        bad(f"topk_indices must be int32 or int64, got {topk_indices.dtype}")
    if seqlen_q != 1:
        bad(f"decode mode: seqlen_q must be 1, got q shape {tuple(q.shape)}")
    if dim not in (64, 128):
        bad(f"head dim must be 64 or 128, got q shape {tuple(q.shape)}")
    for name, t in (("q", q), ("k_context", k_context), ("v_context", v_context), ("k_beam", k_beam), ("v_beam", v_beam)):
        if t.numel() and t.stride(-1) != 1:
            bad(f"{name} must have stride(-1) == 1, got strides {tuple(t.stride())}")


def _require_gpu(**tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise BeamDecodeError(f"{name} must be a GPU tensor (there is no CPU path), got device {t.device}")


def _forward(q, k_context, v_context, k_beam, v_beam, topk_indices, decode_nums, softmax_scale, seqused_k, cu_seqlens_k,
             out, ns):
    B, _, W, Hq, D = q.shape
    jagged = cu_seqlens_k is not None
    Hkv = k_context.shape[1] if jagged else k_context.shape[2]
    Sk = 0 if jagged else k_context.shape[1]
    total_k = k_context.shape[0] if jagged else 0
    if ns is None:
        # (the longest sample is not known without a host read: size for the allocated length; a jagged batch for its mean)
        ns = num_splits(B, W, Hq, Hkv, D, -(-total_k // max(B, 1)) if jagged else Sk)
    ns = int(ns)
    if ns < 1:
        raise BeamDecodeError(f"_num_splits must be >= 1, got {ns}")
    q, k_context, v_context = _rows_aligned(q), _rows_aligned(k_context), _rows_aligned(v_context)
    k_beam, v_beam = _rows_aligned(k_beam), _rows_aligned(v_beam)
    dev = q.device
    res = out if (out is not None and out.is_contiguous()) else torch.empty(B, 1, W, Hq, D, device=dev, dtype=q.dtype)
    lse = torch.empty(B, 1, W, Hq, device=dev, dtype=torch.float32)
    lib = N.lib()
    ws_bytes = lib.mi355_beam_decode_workspace_bytes(B, W, Hq, D, ns)
    ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)
    if jagged:
        kc_s = (0, k_context.stride(0), k_context.stride(1))
        vc_s = (0, v_context.stride(0), v_context.stride(1))
    else:
        kc_s, vc_s = k_context.stride()[:3], v_context.stride()[:3]
    ts = topk_indices.stride()
    N.check(lib.mi355_beam_decode_attn(
        N.ptr(q), q.stride(0), q.stride(2), q.stride(3),
        N.ptr(k_context), N.ptr(v_context), *kc_s, *vc_s, Sk, total_k,
        N.ptr(seqused_k), N.ptr(cu_seqlens_k),
        N.ptr(k_beam), N.ptr(v_beam), *k_beam.stride()[:3], *v_beam.stride()[:3],
        N.ptr(topk_indices), 0 if topk_indices.dtype == torch.int32 else 1, ts[0], ts[2], ts[3], ts[4],
        B, W, Hq, Hkv, D, decode_nums, float(softmax_scale), ns,
        N.ptr(res), N.ptr(lse), N.dt(q), N.ptr(ws), ws.numel(), N.stream()), "mi355_beam_decode_attn")
    return res, lse


class BeamDecodeAttn(torch.autograd.Function):
    """Beam-search decode attention (forward only)."""

    @staticmethod
    def forward(ctx, q, k_context, v_context, k_beam, v_beam, topk_indices, decode_nums, softmax_scale, backend,
                seqused_k=None, cu_seqlens_k=None, out=None, _num_splits=None):
        if backend not in _BACKENDS:
            raise BeamDecodeError(f"backend must be one of {_BACKENDS}, got {backend!r}")
        res, lse = _forward(q.detach(), k_context.detach(), v_context.detach(), k_beam.detach(), v_beam.detach(),
                            topk_indices, decode_nums, softmax_scale, seqused_k, cu_seqlens_k, out, _num_splits)
        if out is not None and res is out:
            ctx.mark_dirty(out)
        return res, lse

    @staticmethod
    def backward(ctx, *args):
        raise NotImplementedError("Beam decode attention is forward-only")


def beam_decode_attn(
    q: torch.Tensor,
    k_context: torch.Tensor,
    v_context: torch.Tensor,
    k_beam: torch.Tensor,
    v_beam: torch.Tensor,
    topk_indices: torch.Tensor,
    decode_nums: int,
    softmax_scale: Optional[float] = None,
    return_lse: bool = False,
    out: Optional[torch.Tensor] = None,
    backend: str = "dsl",
    seqused_k: Optional[torch.Tensor] = None,
    cu_seqlens_k: Optional[torch.Tensor] = None,
    _num_splits: Optional[int] = None,
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Returns (out [B, 1, W, Hq, D] in the dtype of q, lse [B, 1, W, Hq] fp32 or None).  `out`, when given, is filled in
    place and returned.  `_num_splits` forces the KV split count of the context kernel (default: num_splits())."""
    if backend not in _BACKENDS:
        raise BeamDecodeError(f"backend must be one of {_BACKENDS}, got {backend!r}")
    if seqused_k is not None and cu_seqlens_k is not None:
        raise BeamDecodeError("cu_seqlens_k and seqused_k are mutually exclusive")
    _validate_inputs(q, k_context, v_context, k_beam, v_beam, topk_indices, decode_nums,
                     jagged_k_context=cu_seqlens_k is not None)
    B = q.shape[0]
    if seqused_k is not None:
        if seqused_k.dim() != 1 or seqused_k.shape[0] != B or seqused_k.dtype != torch.int32:
            raise BeamDecodeError(f"seqused_k must be int32 [B={B}], got {seqused_k.dtype} {tuple(seqused_k.shape)}")
        seqused_k = seqused_k.contiguous()
    if cu_seqlens_k is not None:
        if cu_seqlens_k.dim() != 1 or cu_seqlens_k.shape[0] != B + 1 or cu_seqlens_k.dtype != torch.int32:
            raise BeamDecodeError(f"cu_seqlens_k must be int32 [B+1={B + 1}], got {cu_seqlens_k.dtype} "
                                  f"{tuple(cu_seqlens_k.shape)}")
        cu_seqlens_k = cu_seqlens_k.contiguous()
    if out is not None and (out.shape != q.shape or out.dtype != q.dtype or out.device != q.device):
        raise BeamDecodeError(f"out must match q: shape {tuple(q.shape)} {q.dtype}, got {tuple(out.shape)} {out.dtype}")
    _require_gpu(q=q, k_context=k_context, v_context=v_context, k_beam=k_beam, v_beam=v_beam, topk_indices=topk_indices,
                 seqused_k=seqused_k, cu_seqlens_k=cu_seqlens_k, out=out)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(q.shape[-1])

    res, lse = BeamDecodeAttn.apply(q, k_context, v_context, k_beam, v_beam, topk_indices, decode_nums, softmax_scale,
                                    backend, seqused_k, cu_seqlens_k, out, _num_splits)
    if out is not None and res is not out:
        out.copy_(res)
        res = out
    return res, (lse if return_lse else None)
