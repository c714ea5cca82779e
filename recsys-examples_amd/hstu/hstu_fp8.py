"""FP8 (OCP e4m3fn) HSTU attention: the quantisers and the forward of the reference's hopper interface
(corelib/hstu/hopper/hstu_attn_interface.py:32-350) on the gfx950 kernels of csrc/hstu_fp8.hip.

* `quantize_for_two_directions`, `quantize_for_block_scale`, `quantize_for_head_batch_tensor` and
  `get_bm_and_bn_block_size_fwd` keep the reference's names, arguments and return tuples, and return the same fp8 bytes
  and descales (tests/golden/hstu_fp8_quant_golden.npz).  The reference loops over the batch in Python; here each tensor
  takes one launch (two for modes 3 / 4 / 5).  The public functions return exactly-sized descale tensors, which costs one
  device-to-host read of the tile count in modes 1 and 2 (the reference reads every length back).
* `varlen_fwd` takes the argument list of `hstu_hopper_cuda.varlen_fwd` (hstu_attn_interface.py:294-350) and returns
  (out, rab): fp16 out computed on the fp8 operands, self-attention only.
* `varlen_bwd` takes the argument list of `hstu_hopper_cuda.varlen_bwd` (hstu_api.cpp:809-1010) and returns
  (dq, dk, dv, None), fp16, computed on fp8 q / k / v / dout; `quantize_for_backward` quantises them as the reference's
  `HSTUAttnVarlenFunc.backward` does (hstu_attn_interface.py:586-660), with `get_bm_and_bn_block_size_bwd`'s mode-2 blocks.
* `HstuAttnFp8Func` backs `hstu_attn_varlen_func(..., quant_mode=0..5)`: quantise, FP8 forward.  Its backward is by default
  the bf16 / fp16 one at the unquantised inputs with dout cast to their dtype (a straight-through estimator); with
  `fp8_backward=True` it is `varlen_bwd(**quantize_for_backward(...))`, the reference's FP8 backward.
Refused by name: rab / func / delta-q / paged KV under FP8, head_dim 32, e5m2.
"""
from __future__ import annotations

import ctypes

import torch

import mi355_native as N
from mi355_native import check, lib, ptr, stream

_FP8 = torch.float8_e4m3fn
_FP8_TYPES = tuple(t for t in (getattr(torch, n, None) for n in ("float8_e4m3fn", "float8_e5m2", "float8_e4m3fnuz",
                                                                    "float8_e5m2fnuz")) if t is not None)


def is_fp8(t) -> bool:
    return t is not None and t.dtype in _FP8_TYPES


def get_bm_and_bn_block_size_fwd(rab, dim):
    """(q block, k / v block) of the mode-2 quantiser (hstu_attn_interface.py:194-212 of the reference)"""
    if rab is not None:
        return (128, 128) if dim == 64 else (128, 64)
    return (128, 128) if dim in (64, 128) else (128, 64)


def get_bm_and_bn_block_size_bwd():
    """(q / dout block, k / v block) of the backward's mode-2 quantisation (the reference's function of that name)"""
    return 64, 128


def _check_x(x, fp8_type, name):
    if fp8_type != _FP8:
        raise NotImplementedError(f"{name}: fp8_type {fp8_type} is not supported (e4m3fn only; e5m2 is not built)")
    if x.dim() != 3:
        raise ValueError(f"AssertError: x in {name} should be three dimensions")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"{name}: x must be bf16 or fp16")
    if x.shape[-1] not in (32, 64, 128, 256):
        raise RuntimeError(f"{name}: head_dim must be one of 32, 64, 128, 256")
    return x.contiguous()


def _offsets(seq_offsets, x):
    off = seq_offsets.to(device=x.device, dtype=torch.int32).contiguous()
    return off, off.numel() - 1


def _cu_blocks(off, B, bs):
    """per-sequence count of bs-token tiles, prefix-summed on the device ([B + 1] int32, the reference's cu_seqlens_*_descale)"""
    cu = torch.empty(B + 1, dtype=torch.int32, device=off.device)
    check(lib().mi355_hstu_fp8_cu_blocks(ptr(off), B, int(bs), ptr(cu), stream()), "hstu_fp8_cu_blocks")
    return cu


def _bound(T, B, bs):
    return int(lib().mi355_hstu_fp8_blocks_bound(int(T), int(B), int(bs)))


def _quantize(kind, x, off=None, B=0, bs=0, cu=None, nblk=0, descale=None, dstride=0, amax=None):
    T, H, D = x.shape
    y = torch.empty(x.shape, dtype=_FP8, device=x.device)
    check(lib().mi355_hstu_fp8_quantize(kind, ptr(x), int(x.dtype == torch.float16), T, H, D, ptr(off), B, int(bs), ptr(cu),
                                        int(nblk), ptr(y), ptr(descale), int(dstride), ptr(amax), stream()),
          "hstu_fp8_quantize")
    return y


def _two_directions(x, off, B, with_vt=True):
    """mode 1 without the host read: descale_vt keeps its bound-sized tile dimension"""
    T, H, D = x.shape
    ds = torch.zeros(H, T + 128, dtype=torch.float32, device=x.device)
    xq = _quantize(1, x, descale=ds, dstride=T + 128)
    if not with_vt:
        return xq, ds, None, None, None
    cu = _cu_blocks(off, B, 128)
    nb = _bound(T, B, 128)
    dvt = torch.empty(max(nb, 1), H, D, dtype=torch.float32, device=x.device)
    xt = _quantize(2, x, off, B, 128, cu, nb, dvt, H * D)
    return xq, ds, xt, dvt, cu


def quantize_for_two_directions(x, seq_offsets, fp8_type=torch.float8_e4m3fn):
    """mode 1: (x_quantized, x_descale [H, total + 128], xt_quantized, xt_descale [tiles, H, d], cu_seqlens_xt_descale)"""
    x = _check_x(x, fp8_type, "quantize_for_two_directions")
    off, B = _offsets(seq_offsets, x)
    xq, ds, xt, dvt, cu = _two_directions(x, off, B)
    return xq, ds, xt, dvt[:int(cu[-1])], cu


def _block_scale(x, off, B, block_size):
    T, H, D = x.shape
    cu = _cu_blocks(off, B, block_size)
    nb = max(_bound(T, B, block_size), 1)
    ds = torch.empty(H, nb, dtype=torch.float32, device=x.device)
    xq = _quantize(3, x, off, B, block_size, cu, nb, ds, nb)
    return xq, ds, cu


def quantize_for_block_scale(x, seq_offsets, block_size=128, fp8_type=torch.float8_e4m3fn):
    """mode 2: (x_quantized, x_descale [H, tiles], cu_seqlens_x_descale)"""
    x = _check_x(x, fp8_type, "quantize_for_block_scale")
    off, B = _offsets(seq_offsets, x)
    xq, ds, cu = _block_scale(x, off, B, int(block_size))
    return xq, ds[:, :int(cu[-1])].contiguous(), cu


def quantize_for_head_batch_tensor(x, seq_offsets, quant_mode=3, fp8_type=torch.float8_e4m3fn):
    """modes 3 / 4 / 5: (x_quantized, x_descale [B, H] / [B] / [1])"""
    x = _check_x(x, fp8_type, "quantize_for_head_batch_tensor")
    if quant_mode not in (3, 4, 5):
        raise ValueError("AssertError: quant_mode in quantize_for_head_batch_tensor should be 3, 4 or 5")
    off, B = _offsets(seq_offsets, x)
    T, H, D = x.shape
    shape = {3: (B, H), 4: (B,), 5: (1,)}[quant_mode]
    ds = torch.zeros(shape, dtype=torch.float32, device=x.device)
    amax = torch.zeros(max(ds.numel(), 1), dtype=torch.int32, device=x.device)
    cu = _cu_blocks(off, B, 128)
    xq = _quantize(quant_mode + 1, x, off, B, 128, cu, _bound(T, B, 128), ds, 0, amax)
    return xq, ds


def quantize_qkv(q, k, v, cu_seqlens, quant_mode):
    """the reference's quantisation of hstu_attn_varlen_func(quant_mode=m) (HSTUAttnVarlenFunc.forward,
    hstu_attn_interface.py:478-560): the keyword arguments of varlen_fwd, with no host read"""
    off, B = _offsets(cu_seqlens, q)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    if quant_mode == 0:
        one = torch.ones(1, dtype=torch.float32, device=q.device)
        return dict(q=_quantize(0, q), k=_quantize(0, k), v=_quantize(0, v), descale_q=one, descale_k=one, descale_v=one)
    if quant_mode == 1:
        q8, dq, _, _, _ = _two_directions(q, off, B, with_vt=False)
        k8, dk, _, _, _ = _two_directions(k, off, B, with_vt=False)
        # v's per-token form is not read by the forward (the PV product uses vt): only the vt quantiser runs
        T, H, D = v.shape
        cu = _cu_blocks(off, B, 128)
        nb = _bound(T, B, 128)
        dvt = torch.empty(max(nb, 1), H, D, dtype=torch.float32, device=q.device)
        vt = _quantize(2, v, off, B, 128, cu, nb, dvt, H * D)
        return dict(q=q8, k=k8, v=vt, vt=vt, descale_q=dq, descale_k=dk, descale_v=None, descale_vt=dvt,
                    cu_seqlens_descale_vt=cu)
    if quant_mode == 2:
        bm, bn = get_bm_and_bn_block_size_fwd(None, q.shape[-1])
        q8, dq, cq = _block_scale(q, off, B, bm)
        k8, dk, ck = _block_scale(k, off, B, bn)
        v8, dv, _ = _block_scale(v, off, B, bn)
        return dict(q=q8, k=k8, v=v8, descale_q=dq, descale_k=dk, descale_v=dv, cu_seqlens_block_descale_q=cq,
                    cu_seqlens_block_descale_kv=ck)
    out = [quantize_for_head_batch_tensor(t, off, quant_mode) for t in (q, k, v)]
    return dict(q=out[0][0], k=out[1][0], v=out[2][0], descale_q=out[0][1], descale_k=out[1][1], descale_v=out[2][1])


def quantize_for_backward(q, k, v, dout, cu_seqlens, quant_mode):
    """the reference's quantisation in HSTUAttnVarlenFunc.backward (hstu_attn_interface.py:586-660) of the saved q / k / v
    and the incoming dout: the keyword arguments of varlen_bwd, with no host read.  Mode 1 keeps qt / kt / dout_t (the
    per-column-per-128-token direction, token-major like every other operand here) and quantises v per token only; the
    other modes return dout_t / q_t / k_t as None, as the reference passes them."""
    if quant_mode is None or isinstance(quant_mode, bool) or int(quant_mode) not in range(6):
        raise ValueError(f"quantize_for_backward: quant_mode must be 0 .. 5, got {quant_mode!r}")
    mode = int(quant_mode)
    ts = (q, k, v, dout)
    for t, name in zip(ts, ("q", "k", "v", "dout")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape != q.shape:
            raise RuntimeError(f"quantize_for_backward: {name} must be a (total, nheads, head_dim) tensor shaped like q")
        if t.dtype not in (torch.bfloat16, torch.float16) or t.dtype != q.dtype:
            raise RuntimeError(f"quantize_for_backward: {name} must be bf16 or fp16, of q's dtype")
    if q.shape[-1] == 32:
        raise NotImplementedError("head dimension 32 is not supported under FP8 (the reference's FP8 set is 64, 128, 256)")
    if q.shape[-1] not in (64, 128, 256):
        raise RuntimeError("quantize_for_backward: head_dim must be one of 64, 128, 256")
    if cu_seqlens is None or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2:
        raise RuntimeError("quantize_for_backward: cu_seqlens must be a 1-D tensor of batch + 1 offsets")
    if not q.is_cuda:
        raise RuntimeError("quantize_for_backward: the tensors must be on the GPU")
    off, B = _offsets(cu_seqlens, q)
    q, k, v, dout = (t.contiguous() for t in ts)
    if mode == 0:
        one = torch.ones(1, dtype=torch.float32, device=q.device)
        return dict(dout=_quantize(0, dout), dout_t=None, q=_quantize(0, q), q_t=None, k=_quantize(0, k), k_t=None,
                    v=_quantize(0, v), descale_q=one, descale_k=one, descale_v=one, descale_do=one)
    if mode == 1:
        q8, dq, qt, dqt, cq = _two_directions(q, off, B)
        k8, dk, kt, dkt, ck = _two_directions(k, off, B)
        v8, dv, _, _, _ = _two_directions(v, off, B, with_vt=False)
        do8, ddo, dot, ddot, _ = _two_directions(dout, off, B)
        return dict(dout=do8, dout_t=dot, q=q8, q_t=qt, k=k8, k_t=kt, v=v8, descale_q=dq, descale_qt=dqt, descale_k=dk,
                    descale_kt=dkt, descale_v=dv, descale_do=ddo, descale_dot=ddot, cu_seqlens_descale_qt=cq,
                    cu_seqlens_descale_kt=ck)
    if mode == 2:
        bm, bn = get_bm_and_bn_block_size_bwd()
        q8, dq, cq = _block_scale(q, off, B, bm)
        k8, dk, ck = _block_scale(k, off, B, bn)
        v8, dv, _ = _block_scale(v, off, B, bn)
        do8, ddo, _ = _block_scale(dout, off, B, bm)
        return dict(dout=do8, dout_t=None, q=q8, q_t=None, k=k8, k_t=None, v=v8, descale_q=dq, descale_k=dk, descale_v=dv,
                    descale_do=ddo, cu_seqlens_q_block_descale=cq, cu_seqlens_kv_block_descale=ck)
    out = [quantize_for_head_batch_tensor(t, off, mode) for t in (q, k, v, dout)]
    return dict(dout=out[3][0], dout_t=None, q=out[0][0], q_t=None, k=out[1][0], k_t=None, v=out[2][0], descale_q=out[0][1],
                descale_k=out[1][1], descale_v=out[2][1], descale_do=out[3][1])


def _f32(t, name):
    if t is None or t.dtype != torch.float32 or not t.is_cuda:
        raise RuntimeError(f"{name} must be a float32 device tensor")
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise RuntimeError(f"{name} must have a contiguous last dimension")
    return t


def _i32(t, n, name):
    if t is None or t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous int32 tensor of batch + 1 entries")
    return t


def varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, scaling_seqlen, num_contexts, num_targets,
               target_group_size, window_size_left, window_size_right, alpha, rab, func, quant_mode, vt=None,
               cu_seqlens_descale_vt=None, descale_q=None, descale_k=None, descale_v=None, descale_vt=None,
               cu_seqlens_block_descale_q=None, cu_seqlens_block_descale_kv=None):
    """hstu_hopper_cuda.varlen_fwd (hstu_attn_interface.py:294-350 of the reference) for quant_mode 0 .. 5: q / k / v (and
    vt in mode 1) are float8_e4m3fn [total, H, d] quantised by the functions above; returns (out fp16, rab)."""
    if quant_mode is None or int(quant_mode) not in range(6):
        raise ValueError(f"varlen_fwd: quant_mode must be 0 .. 5 here, got {quant_mode}")
    mode = int(quant_mode)
    if mode == 1 and vt is not None and vt.stride(-1) != 1:
        vt = vt.contiguous()   # (the reference hands vt over token-contiguous: .transpose(0, 2).contiguous().transpose(0, 2))
    if rab is not None:
        raise NotImplementedError("rab is not supported under FP8 (quant_mode >= 0)")
    if func is not None:
        raise NotImplementedError("func is not supported under FP8 (quant_mode >= 0)")
    for t, name in ((q, "q"), (k, "k"), (v, "v")) + (((vt, "vt"),) if mode == 1 else ()):
        if t is None or t.dtype != _FP8:
            if t is not None and is_fp8(t):
                raise NotImplementedError(f"{name}: {t.dtype} is not supported (e4m3fn only)")
            raise RuntimeError(f"{name} must be a float8_e4m3fn tensor")
        if t.dim() != 3 or t.shape != q.shape or t.stride(-1) != 1 or not t.is_cuda:
            raise RuntimeError("q, k, v must be (total, nheads, head_dim) device tensors of equal shape with a contiguous last dimension")
    T, H, D = q.shape
    if D == 32:
        raise NotImplementedError("head dimension 32 is not supported under FP8 (the reference's FP8 set is 64, 128, 256)")
    if D not in (64, 128, 256):
        raise RuntimeError("head_dim must be one of 64, 128, 256")
    same = cu_seqlens_q.data_ptr() == cu_seqlens_k.data_ptr() or (
        cu_seqlens_q.shape == cu_seqlens_k.shape and q.shape[0] == k.shape[0] and int(max_seqlen_q) == int(max_seqlen_k))
    if not same:
        raise NotImplementedError("delta-q (cu_seqlens_q != cu_seqlens_k) is not supported under FP8 (quant_mode >= 0)")
    B = cu_seqlens_q.numel() - 1
    cu = _i32(cu_seqlens_q, B + 1, "cu_seqlens_q")
    for t, name in ((num_contexts, "num_contexts"), (num_targets, "num_targets")):
        if t is not None and (t.dtype != torch.int32 or t.numel() != B):
            raise RuntimeError(f"{name} must be an int32 tensor of batch entries")
    wl = -1 if window_size_left < 0 else int(window_size_left)
    wr = -1 if window_size_right < 0 else int(window_size_right)
    if (num_contexts is not None or num_targets is not None) and (wl, wr) != (-1, 0):
        raise ValueError("context / target masks need the causal mask (-1, 0): undefined behaviour otherwise")
    if scaling_seqlen is None or scaling_seqlen == -1:
        scaling_seqlen = max_seqlen_q
    dq = dk = dv = None
    sq = sk = sv = 0
    cvt = cbq = cbkv = None
    bn = 0
    if mode == 1:
        dq, dk, dv = (_f32(descale_q, "descale_q"), _f32(descale_k, "descale_k"), _f32(descale_vt, "descale_vt"))
        if dq.dim() != 2 or dk.dim() != 2 or dq.shape[0] != H or dk.shape[0] != H or dq.shape[1] < T or dk.shape[1] < T:
            raise RuntimeError("mode 1: descale_q / descale_k must be [nheads, >= total]")
        if dv.dim() != 3 or dv.shape[1:] != (H, D) or not dv.is_contiguous():
            raise RuntimeError("mode 1: descale_vt must be a contiguous [tiles, nheads, head_dim] tensor")
        sq, sk, sv = dq.stride(0), dk.stride(0), dv.stride(0)
        cvt = _i32(cu_seqlens_descale_vt, B + 1, "cu_seqlens_descale_vt")
        v = vt
    elif mode == 2:
        dq, dk, dv = (_f32(descale_q, "descale_q"), _f32(descale_k, "descale_k"), _f32(descale_v, "descale_v"))
        if any(t.dim() != 2 or t.shape[0] != H for t in (dq, dk, dv)):
            raise RuntimeError("mode 2: descale_q / descale_k / descale_v must be [nheads, blocks]")
        sq, sk, sv = dq.stride(0), dk.stride(0), dv.stride(0)
        cbq = _i32(cu_seqlens_block_descale_q, B + 1, "cu_seqlens_block_descale_q")
        cbkv = _i32(cu_seqlens_block_descale_kv, B + 1, "cu_seqlens_block_descale_kv")
        bn = get_bm_and_bn_block_size_fwd(None, D)[1]
    elif mode >= 3:
        want = {3: B * H, 4: B, 5: 1}[mode]
        dq, dk, dv = (_f32(descale_q, "descale_q"), _f32(descale_k, "descale_k"), _f32(descale_v, "descale_v"))
        if any(t.numel() != want or not t.is_contiguous() for t in (dq, dk, dv)):
            raise RuntimeError(f"mode {mode}: descale_q / descale_k / descale_v must be contiguous with {want} entries")
    out = torch.empty((T, H, D), dtype=torch.float16, device=q.device)
    check(lib().mi355_hstu_attn_fwd_fp8(mode, ptr(q), ptr(k), ptr(v), ptr(out), q.stride(0), k.stride(0), v.stride(0),
                                        out.stride(0), q.stride(1), k.stride(1), v.stride(1), out.stride(1), ptr(cu), B, H, D,
                                        int(max_seqlen_q), ptr(num_contexts), ptr(num_targets), int(target_group_size), wl, wr,
                                        N.c_f(float(alpha)), N.c_f(float(scaling_seqlen)), ptr(dq), ptr(dk), ptr(dv), sq, sk, sv,
                                        ptr(cvt), ptr(cbq), ptr(cbkv), bn, stream()), "hstu_attn_fwd_fp8")
    return out, rab


class HstuAttnFp8Func(torch.autograd.Function):
    """hstu_attn_varlen_func(quant_mode=0..5): quantise + FP8 forward (fp16 out).  Backward: with fp8_backward, the
    reference's FP8 backward (quantize_for_backward of the saved inputs and dout, then varlen_bwd; the fp16 gradients cast to
    the inputs' dtype); otherwise the bf16 / fp16 backward at the unquantised inputs with dout cast to their dtype
    (straight-through)."""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens, max_seqlen, scaling_seqlen, num_contexts, num_targets, target_group_size, wl, wr,
                alpha, quant_mode, fp8_backward=False):
        kw = quantize_qkv(q, k, v, cu_seqlens, quant_mode)
        out, _ = varlen_fwd(cu_seqlens_q=cu_seqlens, cu_seqlens_k=cu_seqlens, max_seqlen_q=max_seqlen, max_seqlen_k=max_seqlen,
                            scaling_seqlen=scaling_seqlen, num_contexts=num_contexts, num_targets=num_targets,
                            target_group_size=target_group_size, window_size_left=wl, window_size_right=wr, alpha=alpha,
                            rab=None, func=None, quant_mode=quant_mode, **kw)
        ctx.save_for_backward(q, k, v, cu_seqlens, num_contexts, num_targets)
        ctx.meta = (max_seqlen, scaling_seqlen, target_group_size, wl, wr, alpha)
        ctx.quant = (quant_mode, bool(fp8_backward))
        return out

    @staticmethod
    def backward(ctx, dout):
        from .hstu_attn_interface import hstu_varlen_bwd, hstu_varlen_bwd_window

        q, k, v, cu, nc, nt = ctx.saved_tensors
        max_seqlen, scaling, g, wl, wr, alpha = ctx.meta
        mode, fp8_backward = ctx.quant
        dout = dout.to(q.dtype)
        if fp8_backward:
            kw = quantize_for_backward(q, k, v, dout, cu, mode)
            dq, dk, dv, _ = varlen_bwd(dq=None, dk=None, dv=None, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=max_seqlen,
                                       max_seqlen_k=max_seqlen, scaling_seqlen=scaling, num_contexts=nc, num_targets=nt,
                                       target_group_size=g, window_size_left=wl, window_size_right=wr, alpha=alpha,
                                       quant_mode=mode, **kw)
            dq, dk, dv = dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)
        elif not (wl == -1 and wr in (-1, 0)):
            dq, dk, dv = hstu_varlen_bwd_window(dout, q, k, v, cu, max_seqlen, scaling, wl, wr, alpha)
        else:
            dq, dk, dv = hstu_varlen_bwd(dout, q, k, v, cu, max_seqlen, scaling, nc, nt, g, wr == 0, alpha)
        return dq, dk, dv, None, None, None, None, None, None, None, None, None, None, None


def _grad_out(t, like, name):
    """the caller's dq / dk / dv when it is an fp16 tensor of the right shape (written in place), else a new fp16 one (the
    reference's dq.to(torch::kFloat16), hstu_api.cpp:915-918)"""
    if t is not None and t.dtype == torch.float16 and t.shape == like.shape and t.stride(-1) == 1 and t.device == like.device:
        return t
    return torch.empty(like.shape, dtype=torch.float16, device=like.device)


def varlen_bwd(dout, dout_t, q, q_t, k, k_t, v, dq, dk, dv, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
               scaling_seqlen, num_contexts, num_targets, target_group_size, window_size_left, window_size_right, alpha,
               quant_mode, rab=None, has_drab=False, func=None, descale_q=None, descale_qt=None, descale_k=None,
               descale_kt=None, descale_v=None, descale_do=None, descale_dot=None, cu_seqlens_descale_qt=None,
               cu_seqlens_descale_kt=None, cu_seqlens_q_block_descale=None, cu_seqlens_kv_block_descale=None,
               deterministic=False):
    """hstu_hopper_cuda.varlen_bwd (hstu_api.cpp:809-1010 of the reference) for quant_mode 0 .. 5: dout / q / k / v (and
    dout_t / q_t / k_t in mode 1) are float8_e4m3fn [total, H, d] from quantize_for_backward; returns (dq, dk, dv, None),
    fp16.  Always deterministic (no atomics): `deterministic` is accepted and ignored."""
    if quant_mode is None or isinstance(quant_mode, bool) or int(quant_mode) not in range(6):
        raise ValueError(f"varlen_bwd: quant_mode must be 0 .. 5 here, got {quant_mode!r}")
    mode = int(quant_mode)
    if rab is not None or has_drab:
        raise NotImplementedError("rab / has_drab are not supported under FP8 (quant_mode >= 0)")
    if func is not None:
        raise NotImplementedError("func is not supported under FP8 (quant_mode >= 0)")
    ops = [(dout, "dout"), (q, "q"), (k, "k"), (v, "v")]
    if mode == 1:
        ops += [(dout_t, "dout_t"), (q_t, "q_t"), (k_t, "k_t")]
    for t, name in ops:
        if t is None or t.dtype != _FP8:
            if t is not None and is_fp8(t):
                raise NotImplementedError(f"{name}: {t.dtype} is not supported (e4m3fn only)")
            raise RuntimeError(f"{name} must be a float8_e4m3fn tensor")
    if q.dim() != 3:
        raise RuntimeError("q must be (total, nheads, head_dim)")
    T, H, D = q.shape
    if D == 32:
        raise NotImplementedError("head dimension 32 is not supported under FP8 (the reference's FP8 set is 64, 128, 256)")
    if D not in (64, 128, 256):
        raise RuntimeError("head_dim must be one of 64, 128, 256")
    same = cu_seqlens_q.data_ptr() == cu_seqlens_k.data_ptr() or (
        cu_seqlens_q.shape == cu_seqlens_k.shape and k.shape[0] == T and int(max_seqlen_q) == int(max_seqlen_k))
    if not same:
        raise NotImplementedError("delta-q (cu_seqlens_q != cu_seqlens_k) is not supported under FP8 (quant_mode >= 0)")
    if mode == 1:   # (the reference hands the transposed directions over token-contiguous)
        dout_t, q_t, k_t = (t if t.stride(-1) == 1 else t.contiguous() for t in (dout_t, q_t, k_t))
        ops = [(dout, "dout"), (q, "q"), (k, "k"), (v, "v"), (dout_t, "dout_t"), (q_t, "q_t"), (k_t, "k_t")]
    for t, name in ops:
        if t.shape != q.shape or t.stride(-1) != 1 or not t.is_cuda:
            raise RuntimeError(f"{name} must be a (total, nheads, head_dim) device tensor shaped like q with a contiguous last "
                               "dimension")
    B = cu_seqlens_q.numel() - 1
    cu = _i32(cu_seqlens_q, B + 1, "cu_seqlens_q")
    for t, name in ((num_contexts, "num_contexts"), (num_targets, "num_targets")):
        if t is not None and (t.dtype != torch.int32 or t.numel() != B):
            raise RuntimeError(f"{name} must be an int32 tensor of batch entries")
    wl = -1 if window_size_left < 0 else int(window_size_left)
    wr = -1 if window_size_right < 0 else int(window_size_right)
    if (num_contexts is not None or num_targets is not None) and (wl, wr) != (-1, 0):
        raise ValueError("context / target masks need the causal mask (-1, 0): undefined behaviour otherwise")
    if scaling_seqlen is None or scaling_seqlen == -1:
        scaling_seqlen = max_seqlen_q
    ds = dict(q=descale_q, qt=descale_qt, k=descale_k, kt=descale_kt, v=descale_v, do=descale_do, dot=descale_dot)
    strides = dict.fromkeys(ds, 0)
    cqt = ckt = cbq = cbkv = None
    if mode >= 1:
        for n in ("q", "k", "v", "do"):
            ds[n] = _f32(ds[n], f"descale_{n}")
    if mode == 1:
        for n in ("qt", "kt", "dot"):
            ds[n] = _f32(ds[n], f"descale_{n}")
            if ds[n].dim() != 3 or ds[n].shape[1:] != (H, D) or not ds[n].is_contiguous():
                raise RuntimeError(f"mode 1: descale_{n} must be a contiguous [tiles, nheads, head_dim] tensor")
        for n in ("q", "k", "v", "do"):
            if ds[n].dim() != 2 or ds[n].shape[0] != H or ds[n].shape[1] < T:
                raise RuntimeError(f"mode 1: descale_{n} must be [nheads, >= total]")
        strides = {n: ds[n].stride(0) for n in ds}
        cqt = _i32(cu_seqlens_descale_qt, B + 1, "cu_seqlens_descale_qt")
        ckt = _i32(cu_seqlens_descale_kt, B + 1, "cu_seqlens_descale_kt")
    elif mode == 2:
        if any(ds[n].dim() != 2 or ds[n].shape[0] != H for n in ("q", "k", "v", "do")):
            raise RuntimeError("mode 2: descale_q / descale_k / descale_v / descale_do must be [nheads, blocks]")
        strides.update({n: ds[n].stride(0) for n in ("q", "k", "v", "do")})
        cbq = _i32(cu_seqlens_q_block_descale, B + 1, "cu_seqlens_q_block_descale")
        cbkv = _i32(cu_seqlens_kv_block_descale, B + 1, "cu_seqlens_kv_block_descale")
    elif mode >= 3:
        want = {3: B * H, 4: B, 5: 1}[mode]
        if any(ds[n].numel() != want or not ds[n].is_contiguous() for n in ("q", "k", "v", "do")):
            raise RuntimeError(f"mode {mode}: descale_q / descale_k / descale_v / descale_do must be contiguous with {want} "
                               "entries")
    if mode != 1:
        dout_t = q_t = k_t = None
        ds["qt"] = ds["kt"] = ds["dot"] = None
    dq, dk, dv = _grad_out(dq, q, "dq"), _grad_out(dk, k, "dk"), _grad_out(dv, v, "dv")
    ins = (dout, dout_t, q, q_t, k, k_t, v, dq, dk, dv)
    rs = (ctypes.c_int64 * 10)(*[t.stride(0) if t is not None else 0 for t in ins])
    hs = (ctypes.c_int64 * 10)(*[t.stride(1) if t is not None else 0 for t in ins])
    dss = (ctypes.c_int64 * 7)(*[strides[n] for n in ("q", "qt", "k", "kt", "v", "do", "dot")])
    addr = lambda arr: ctypes.cast(arr, ctypes.c_void_p)
    check(lib().mi355_hstu_attn_bwd_fp8(mode, ptr(dout), ptr(dout_t), ptr(q), ptr(q_t), ptr(k), ptr(k_t), ptr(v), ptr(dq),
                                        ptr(dk), ptr(dv), addr(rs), addr(hs), ptr(cu), B, H, D, int(max_seqlen_q),
                                        ptr(num_contexts), ptr(num_targets), int(target_group_size), wl, wr,
                                        N.c_f(float(alpha)), N.c_f(float(scaling_seqlen)), ptr(ds["q"]), ptr(ds["qt"]),
                                        ptr(ds["k"]), ptr(ds["kt"]), ptr(ds["v"]), ptr(ds["do"]), ptr(ds["dot"]), addr(dss),
                                        ptr(cqt), ptr(ckt), ptr(cbq), ptr(cbkv), stream()), "hstu_attn_bwd_fp8")
    return dq, dk, dv, None
