"""The fused HSTU layer on MI355X: `fused_hstu_op` and `FusedHSTULayerFunction` with the 29 parameters, order and defaults of
the reference (examples/hstu/ops/fused_hstu_op.py:75-1173), composed from this package's own pieces:

    y = layer_norm(input)                      hstu_norm      (csrc/norm_ops.hip)
    z = y @ w_uvqk + b_uvqk;  a = silu(z)      hstu_addmm     (rocBLAS / hipBLASLt GEMM, csrc/act_ops.hip)
    u, v, q, k = split(a)                      views of the one [T, (2 dl + 2 da) H] buffer
    o = hstu_attention(q, k, v)                hstu           (csrc/hstu_attn.hip)
    t = dropout(layer_norm(o) * u)             hstu_norm
    out = t @ w_proj (+ input)                 hstu_addmm

`from fused_hstu_op import fused_hstu_op` is the one import modules/fused_hstu_layer.py needs.  The backward allocates one
buffer, duvqk: the LN-mul-dropout backward writes du into its u slice, the attention backward dq / dk / dv into the other three,
and one kernel turns it in place into the gradient of z and sums the bias gradient on the way.  Then the two GEMMs, and the
input norm's backward adds the residual gradient before its one rounding.

What differs from the reference, all of it stated here:
* attn_backend: any object with a `.name` of TRITON, PYTORCH or CUTLASS (the example's configs.KernelBackend, or the enum
  below); all three run the HIP attention.  Under TRITON the reference's restrictions hold: num_contextuals is one int for the
  batch (a tensor gives its first element) and target_group_size is 1.
* num_contextuals may be an int under every backend: 0 / None is no context, n > 0 an int32 [B] tensor filled with n.
* linear_dim_per_head != attention_dim_per_head raises ValueError: the kernels take V with K's head dim.
* recompute_input_silu recomputes silu(z) with the forward's kernel, so the recomputed u, v, q, k are bit-equal.
* residual=False runs torch.mm: no zero tensor is made.
* T == 0 returns an empty [0, hidden] without a launch; its backward gives zero parameter gradients.
* dropout is this package's Philox stream (hstu_norm), not Triton's.
"""
import enum
from typing import Optional, Tuple, Union

import torch

from hstu_addmm import triton_addmm_silu_bwd, triton_addmm_silu_fwd, triton_silu_fwd
from hstu_norm import (triton_layer_norm_mul_dropout_bwd, triton_layer_norm_mul_dropout_fwd, triton_weighted_layer_norm_bwd,
                       triton_weighted_layer_norm_fwd)

__all__ = ["KernelBackend", "FusedHSTULayerFunction", "fused_hstu_op"]


class KernelBackend(enum.Enum):
    TRITON = "TRITON"
    PYTORCH = "PYTORCH"
    CUTLASS = "CUTLASS"


def _backend_name(attn_backend) -> str:
    name = getattr(attn_backend, "name", attn_backend)
    if name not in KernelBackend.__members__:
        raise ValueError(f"attn_backend must be one of {list(KernelBackend.__members__)}, got {attn_backend!r}")
    return name


def _attn():
    import hstu  # noqa: F401  (lazy: registers the attention entry points on first use)
    from hstu import hstu_attn_interface

    return hstu_attn_interface


def _contexts(num_contextuals, batch: int, device, one_for_batch: bool) -> Optional[torch.Tensor]:
    """the attention's int32 [B] context counts, or None for none; `one_for_batch` (TRITON) lets a tensor stand for its first
    entry alone, read back to the host"""
    if one_for_batch and isinstance(num_contextuals, torch.Tensor):
        num_contextuals = int(num_contextuals.flatten()[0]) if num_contextuals.numel() else 0
    if num_contextuals is None:
        return None
    if isinstance(num_contextuals, int):
        if num_contextuals < 0:
            raise ValueError("num_contextuals must not be negative")
        return None if num_contextuals == 0 else torch.full((batch,), num_contextuals, dtype=torch.int32, device=device)
    return num_contextuals.to(torch.int32)


def _split(buf: torch.Tensor, H: int, d: int):
    """u [T, H d] and v, q, k [T, H, d]: views of the [T, 4 H d] buffer"""
    u, v, q, k = buf.split(H * d, dim=-1)
    return u, v.view(-1, H, d), q.view(-1, H, d), k.view(-1, H, d)


class FusedHSTULayerFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input: torch.Tensor, seqlen_offsets: torch.Tensor, max_seqlen: int, scaling_seqlen: int,
                linear_uvqk_weight: torch.Tensor, linear_uvqk_bias: torch.Tensor, linear_proj_weight: torch.Tensor,
                num_heads: int, linear_dim_per_head: int, attention_dim_per_head: int, ln_eps: float, dropout_ratio: float,
                training: bool, input_norm_weight: Optional[torch.Tensor] = None, input_norm_bias: Optional[torch.Tensor] = None,
                output_norm_weight: Optional[torch.Tensor] = None, output_norm_bias: Optional[torch.Tensor] = None,
                attn_backend=KernelBackend.CUTLASS, num_targets: Optional[torch.Tensor] = None,
                num_contextuals: Union[int, Optional[torch.Tensor]] = None, target_group_size: int = 1, alpha: float = 1.0,
                causal: bool = True, seed: Optional[int] = None, residual: bool = True,
                wgrad_stream: Optional[torch.cuda.Stream] = None, wgrad_event: Optional[torch.cuda.Event] = None,
                recompute_input_layernorm: bool = False, recompute_input_silu: bool = False) -> torch.Tensor:
        backend = _backend_name(attn_backend)
        if input.dim() != 2:
            raise ValueError("input tensor must be 2D")
        if linear_uvqk_bias.dim() != 1:
            raise ValueError("linear_uvqk_bias must be 1D")
        if linear_dim_per_head != attention_dim_per_head:
            raise ValueError("linear_dim_per_head must equal attention_dim_per_head: the attention kernels take V with K's head dim")
        if (input_norm_weight is None) != (input_norm_bias is None):
            raise ValueError("input_norm_weight and input_norm_bias are given together or not at all")
        if output_norm_weight is None or output_norm_bias is None:
            raise ValueError("output_norm_weight and output_norm_bias must be provided")
        if backend == "TRITON" and target_group_size != 1:
            raise ValueError(f"attn_backend TRITON has no target groups: target_group_size is {target_group_size}, not 1")
        if scaling_seqlen is None or scaling_seqlen == -1:
            scaling_seqlen = max_seqlen
        H, d = int(num_heads), int(attention_dim_per_head)
        T, hidden = input.shape
        if linear_uvqk_weight.shape != (hidden, 4 * H * d) or linear_uvqk_bias.numel() != 4 * H * d:
            raise ValueError(f"linear_uvqk_weight must be [{hidden}, {4 * H * d}] and linear_uvqk_bias [{4 * H * d}]")
        if linear_proj_weight.shape != (H * d, hidden):
            raise ValueError(f"linear_proj_weight must be [{H * d}, {hidden}]")
        ctx.learnable_input_norm = input_norm_weight is not None
        ctx.meta = (H, d, float(ln_eps), float(dropout_ratio), bool(training), int(max_seqlen), scaling_seqlen,
                    int(target_group_size), float(alpha), bool(causal), bool(residual))
        ctx.wgrad = (wgrad_stream, wgrad_event)
        ctx.recompute = (bool(recompute_input_layernorm), bool(recompute_input_silu))
        ctx.empty = T == 0
        if ctx.empty:
            ctx.save_for_backward(linear_uvqk_weight, linear_uvqk_bias, linear_proj_weight, input_norm_weight, input_norm_bias,
                                  output_norm_weight, output_norm_bias)
            return input.new_empty((0, hidden))
        A = _attn()
        A.check_operand_type(input.dtype, d)   # (refused before anything is launched)
        cu = seqlen_offsets.to(torch.int32)
        contexts = _contexts(num_contextuals, cu.numel() - 1, input.device, backend == "TRITON")
        targets = None if num_targets is None else num_targets.to(torch.int32)

        if not causal and (contexts is not None or targets is not None):
            raise ValueError("num_contextuals and num_targets are defined for the causal mask only")

        # 1. input layer norm   2. projection with bias, SiLU into a buffer of its own (z is what the backward keeps)
        normed, in_mean, in_rstd, in_block, in_warps = triton_weighted_layer_norm_fwd(
            x=input, weight=input_norm_weight, bias=input_norm_bias, eps=ln_eps)
        z, act = triton_addmm_silu_fwd(x=normed, w=linear_uvqk_weight, y=linear_uvqk_bias, silu=True)
        if recompute_input_layernorm:
            normed = None
        # 3. u, v, q, k   4. attention
        u, v, q, k = _split(act, H, d)
        attn_out = A.hstu_varlen_fwd(q, k, v, cu, int(max_seqlen), scaling_seqlen, contexts, targets, int(target_group_size),
                                     bool(causal), float(alpha)).view(T, H * d)
        # 5. output norm, times u, dropout
        y, out_mean, out_rstd, out_block, out_warps, ret_seed = triton_layer_norm_mul_dropout_fwd(
            x=attn_out, u=u, weight=output_norm_weight, bias=output_norm_bias, eps=ln_eps, dropout_ratio=dropout_ratio,
            training=training, concat_ux=False, seed=seed)
        del u, v, q, k
        if recompute_input_silu:
            act = None   # the last reference: the buffer goes back to the allocator here
        # 6. output projection (+ residual)
        if residual:
            out, _ = triton_addmm_silu_fwd(x=y, w=linear_proj_weight, y=input, silu=False)
        else:
            out = torch.mm(y, linear_proj_weight)
        ctx.launch = (in_block, in_warps, out_block, out_warps, ret_seed)
        ctx.save_for_backward(input, input_norm_weight, input_norm_bias, in_mean, in_rstd, normed, linear_uvqk_weight, z, act, cu,
                              contexts, targets, attn_out, output_norm_weight, output_norm_bias, out_mean, out_rstd, y,
                              linear_proj_weight)
        return out

    @staticmethod
    def backward(ctx, grad_output) -> Tuple[Optional[torch.Tensor], ...]:
        H, d, eps, dropout_ratio, training, max_seqlen, scaling_seqlen, group, alpha, causal, residual = ctx.meta
        wgrad_stream, wgrad_event = ctx.wgrad

        def result(g_input, g_uvqk_w, g_uvqk_b, g_proj_w, g_in_w, g_in_b, g_out_w, g_out_b):
            return (g_input, None, None, None, g_uvqk_w, g_uvqk_b, g_proj_w, None, None, None, None, None, None,
                    g_in_w, g_in_b, g_out_w, g_out_b) + (None,) * 12

        if ctx.empty:
            uvqk_w, uvqk_b, proj_w, in_w, in_b, out_w, out_b = ctx.saved_tensors
            zeros = [None if p is None else torch.zeros_like(p) for p in (uvqk_w, uvqk_b, proj_w, in_w, in_b, out_w, out_b)]
            return result(grad_output.new_empty(grad_output.shape), *zeros)
        (input, in_w, in_b, in_mean, in_rstd, normed, uvqk_w, z, act, cu, contexts, targets, attn_out, out_w, out_b, out_mean,
         out_rstd, y, proj_w) = ctx.saved_tensors
        in_block, in_warps, out_block, out_warps, seed = ctx.launch
        A = _attn()
        T = input.size(0)
        duvqk = torch.empty_like(z)
        pre_du, pre_dv, pre_dq, pre_dk = _split(duvqk, H, d)
        # 1. output projection: grad of y, of its weight (side stream when given), and of the residual (grad_output itself)
        grad_y, g_proj_w, grad_residual = triton_addmm_silu_bwd(x=y, w=proj_w, z=None, grad_output=grad_output, is_y_1d=False,
                                                                wgrad_stream=wgrad_stream, wgrad_event=wgrad_event)
        if act is None:
            act = triton_silu_fwd(z)   # the forward's kernel on the forward's z: bit-equal u, v, q, k
        u, v, q, k = _split(act, H, d)
        # 2. LN-mul-dropout backward, du into its slice
        grad_attn, _, g_out_w, g_out_b, _ = triton_layer_norm_mul_dropout_bwd(
            dy=grad_y, x=attn_out, u=u, weight=out_w, bias=out_b, mean=out_mean, rstd=out_rstd, BLOCK_D=out_block,
            num_warps=out_warps, eps=eps, training=training, dropout_ratio=dropout_ratio, seed=seed, concat_ux=False,
            compute_y=False, wait_event=wgrad_event, du=pre_du)
        # 3. attention backward, dq / dk / dv into theirs
        A.hstu_varlen_bwd(grad_attn.view(T, H, d), q, k, v, cu, max_seqlen, scaling_seqlen, contexts, targets, group, causal, alpha,
                          dq=pre_dq, dk=pre_dk, dv=pre_dv)
        del u, v, q, k, act
        # (recompute_input_layernorm: the normed input again from the saved statistics)
        if normed is None:
            normed = triton_weighted_layer_norm_fwd(x=input, weight=in_w, bias=in_b, eps=eps, mean=in_mean, rstd=in_rstd)[0]
        # 4. SiLU backward + bias gradient over duvqk in place   5. the two GEMMs
        grad_normed, g_uvqk_w, g_uvqk_b = triton_addmm_silu_bwd(x=normed, w=uvqk_w, z=z, grad_output=duvqk, is_y_1d=True,
                                                                silu=True, wgrad_stream=wgrad_stream, wgrad_event=wgrad_event,
                                                                dz_out=duvqk)
        # 6. input norm backward; the residual gradient joins before the rounding
        g_input, g_in_w, g_in_b = triton_weighted_layer_norm_bwd(
            dy=grad_normed, x=input, weight=in_w, bias=in_b, mean=in_mean, rstd=in_rstd, learnable=ctx.learnable_input_norm,
            eps=eps, BLOCK_D=in_block, num_warps=in_warps, dx_accumulate=grad_residual if residual else None,
            wait_event=wgrad_event)
        return result(g_input, g_uvqk_w, g_uvqk_b, g_proj_w, g_in_w, g_in_b, g_out_w, g_out_b)


def fused_hstu_op(input: torch.Tensor, seqlen_offsets: torch.Tensor, max_seqlen: int, scaling_seqlen: int,
                  linear_uvqk_weight: torch.Tensor, linear_uvqk_bias: torch.Tensor, linear_proj_weight: torch.Tensor,
                  num_heads: int, linear_dim_per_head: int, attention_dim_per_head: int, ln_eps: float, dropout_ratio: float,
                  training: bool, input_norm_weight: Optional[torch.Tensor] = None, input_norm_bias: Optional[torch.Tensor] = None,
                  output_norm_weight: Optional[torch.Tensor] = None, output_norm_bias: Optional[torch.Tensor] = None,
                  attn_backend=KernelBackend.CUTLASS, num_targets: Optional[torch.Tensor] = None,
                  num_contextuals: Union[int, Optional[torch.Tensor]] = None, target_group_size: int = 1, alpha: float = 1.0,
                  causal: bool = True, seed: Optional[int] = None, residual: bool = True,
                  wgrad_stream: Optional[torch.cuda.Stream] = None, wgrad_event: Optional[torch.cuda.Event] = None,
                  recompute_input_layernorm: bool = False, recompute_input_silu: bool = False) -> torch.Tensor:
    """One HSTU layer, [T, hidden] -> [T, hidden], differentiable in input, the three linear and the four norm parameters."""
    return FusedHSTULayerFunction.apply(
        input, seqlen_offsets, max_seqlen, scaling_seqlen, linear_uvqk_weight, linear_uvqk_bias, linear_proj_weight, num_heads,
        linear_dim_per_head, attention_dim_per_head, ln_eps, dropout_ratio, training, input_norm_weight, input_norm_bias,
        output_norm_weight, output_norm_bias, attn_backend, num_targets, num_contextuals, target_group_size, alpha, causal, seed,
        residual, wgrad_stream, wgrad_event, recompute_input_layernorm, recompute_input_silu)
