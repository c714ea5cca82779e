"""The HSTU layer norms on MI355X: layer norm, layer-norm-mul-dropout, group-norm-mul-dropout, swish layer norm and RMS norm,
forward and backward, with the names, argument order, defaults and return tuples of the reference
(examples/hstu/ops/triton_ops/triton_layer_norm.py:313-481, :537-906 and triton_norm_mul_dropout.py:361-525, :600-1182), over
the kernels of csrc/norm_ops.hip, csrc/group_norm_ops.hip and csrc/norm_family_ops.hip.

* fused_hstu_op.py of this package is built on them; paged_hstu_infer_layer.py and native_hstu_layer.py import them from
  here, the paged layer together with `from hstu_addmm import torch_addmm_silu_fwd, triton_addmm_silu_fwd`
  (INTEGRATION.md §4).  There is no Triton here and no eager fallback: CPU tensors raise.
* `BLOCK_D`, `BLOCK_H` and `num_warps` are the reference's launch parameters: computed by its formulas and returned, ignored when passed
  back in (the kernels choose their layout from D).
* x, dy, u, du and dx_accumulate are read and written in place with their strides; only a strided LAST dimension is copied.
* Dropout is this project's Philox stream (include/recsys_amd.h), not Triton's: a function of (seed, row, col, which, p).
* dweight / dbias are fp32 sums in a fixed order, bitwise reproducible.  D <= 8192.
* group norm: weight and bias are [num_heads]; mean and rstd are fp32 [N * num_heads]; u may be [N, H, L] with a head stride.
"""
from typing import Optional, Tuple

import torch

import mi355_native as N

__all__ = ["triton_weighted_layer_norm_fwd", "triton_weighted_layer_norm_bwd", "triton_layer_norm_mul_dropout_fwd",
           "triton_layer_norm_mul_dropout_bwd", "triton_layer_norm", "triton_norm_mul_dropout", "layer_norm", "norm_mul_dropout",
           "weighted_layer_norm_fwd", "weighted_layer_norm_bwd", "layer_norm_mul_dropout_fwd", "layer_norm_mul_dropout_bwd",
           "triton_group_norm_mul_dropout_fwd", "triton_group_norm_mul_dropout_bwd", "triton_swish_layer_norm", "triton_rms_norm",
           "group_norm_mul_dropout_fwd", "group_norm_mul_dropout_bwd", "swish_layer_norm", "rms_norm",
           "triton_swish_layer_norm_fwd", "triton_swish_layer_norm_bwd", "triton_rms_norm_fwd", "triton_rms_norm_bwd",
           "swish_layer_norm_fwd", "swish_layer_norm_bwd", "rms_norm_fwd", "rms_norm_bwd",
           "GroupNormMulDropoutFunction", "SwishLayerNormFunction", "RMSNormFunction"]


def _next_power_of_2(n: int) -> int:
    return 1 if n <= 1 else 1 << (int(n) - 1).bit_length()


def _launch_params(D: int, element_size: int) -> Tuple[int, int]:
    """BLOCK_D and num_warps of the reference (triton_layer_norm.py:340-345)"""
    block_d = min(65536 // element_size, _next_power_of_2(D))
    if D > block_d:
        raise RuntimeError("This layer norm doesn't support feature dim >= 64KB.")
    return block_d, min(max(block_d // 256, 1), 8)


def _require_gpu(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise N.NativeError("the layer norms expect GPU tensors (no CPU fallback exists)")
        if dev is not None and t.device != dev:
            raise ValueError("all tensors must be on one device")
        dev = t.device


def _rows(t: torch.Tensor) -> torch.Tensor:
    """a 2-D tensor whose last dimension is contiguous (any row stride)"""
    return t if t.stride(1) == 1 or t.size(1) == 1 else t.contiguous()


def _stride(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


def _u_layout(u: torch.Tensor, D: int, name: str = "u"):
    """(tensor, stride0, stride1, H, UD) of a [N, D] or [N, H, UD] tensor with a contiguous last dimension"""
    if u.dim() == 2:
        u = _rows(u)
        return u, _stride(u), D, 1, D
    if u.dim() != 3:
        raise ValueError(f"{name} must be 2-D or 3-D, got {u.dim()}-D")
    if u.stride(2) != 1 and u.size(2) != 1:
        u = u.contiguous()
    H, UD = u.size(1), u.size(2)
    s1 = u.stride(1) if H > 1 else UD
    s0 = u.stride(0) if u.size(0) > 1 else max(u.stride(0), (H - 1) * s1 + UD)
    return u, s0, s1, H, UD


def _check_rows(x, name="x"):
    if x.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got {x.dim()}-D")
    if x.dtype not in N._DT:
        raise N.NativeError(f"unsupported dtype {x.dtype}")


def _check_params(weight, bias, D):
    if weight.dim() != 1 or bias.dim() != 1 or weight.numel() != D or bias.numel() != D:
        raise ValueError(f"weight and bias must be 1-D with {D} elements")
    if weight.dtype != bias.dtype:
        raise ValueError("weight and bias must share one dtype")


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _du_layout(du: Optional[torch.Tensor], u: torch.Tensor, D: int):
    """(du, stride0, stride1): a new tensor like u, or the caller's after the check against u"""
    if du is None:
        du = torch.empty_like(u)
    if du.shape != u.shape or (du.stride(-1) != 1 and du.size(-1) != 1):
        raise ValueError("du must have the shape of u and a contiguous last dimension")
    _, ds0, ds1, _, _ = _u_layout(du, D, "du")
    return du, ds0, ds1


def _new_y(x: torch.Tensor, width: int) -> torch.Tensor:
    return torch.empty((x.size(0), width), dtype=x.dtype, device=x.device)


def _new_stat(x: torch.Tensor, n: int) -> torch.Tensor:
    return torch.empty((n,), dtype=torch.float32, device=x.device)


def _new_dparam(x: torch.Tensor, weight: torch.Tensor, n: int) -> torch.Tensor:
    return torch.empty((n,), dtype=weight.dtype, device=x.device)


def triton_weighted_layer_norm_fwd(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float,
                                   mean: Optional[torch.Tensor] = None, rstd: Optional[torch.Tensor] = None
                                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int, int]:
    """y = (x - mean) rstd weight + bias per row (weight None: a plain norm); returns (y, mean, rstd, BLOCK_D, num_warps).
    When `mean` and `rstd` are both passed they are used as given and nothing is recomputed."""
    _check_rows(x)
    _require_gpu(x, weight, bias, mean, rstd)
    x = _rows(x)
    rows, D = x.shape
    learnable = weight is not None
    if learnable:
        assert bias is not None
        _check_params(weight, bias, D)
        weight, bias = weight.contiguous(), bias.contiguous()
    y = _new_y(x, D)
    given = mean is not None and rstd is not None
    if mean is None:
        mean = _new_stat(x, rows)
    if rstd is None:
        rstd = _new_stat(x, rows)
    block_d, num_warps = _launch_params(D, x.element_size())
    N.check(N.lib().mi355_hstu_layer_norm_fwd(
        N.ptr(x), _stride(x), rows, D, N.dt(x), N.ptr(weight), N.ptr(bias), N.dt(weight) if learnable else N.dt(x), float(eps),
        N.ptr(y), D, N.ptr(mean), N.ptr(rstd), int(given), N.stream()), "mi355_hstu_layer_norm_fwd")
    return y, mean, rstd, block_d, num_warps


def triton_weighted_layer_norm_bwd(dy: torch.Tensor, x: torch.Tensor, weight: Optional[torch.Tensor],
                                   bias: Optional[torch.Tensor], mean: torch.Tensor, rstd: torch.Tensor, learnable: bool,
                                   eps: float, BLOCK_D: int, num_warps: int, dx_accumulate: Optional[torch.Tensor] = None,
                                   wait_event: Optional[torch.cuda.Event] = None
                                   ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(dx, dweight, dbias); dx_accumulate, when given, is added to dx in fp32 before the rounding."""
    _check_rows(x)
    _require_gpu(dy, x, weight, mean, rstd, dx_accumulate)
    x, dy = _rows(x), _rows(dy)
    acc = None if dx_accumulate is None else _rows(dx_accumulate)
    rows, D = x.shape
    dx = _new_y(x, D)
    dweight = dbias = ws = None
    lib = N.lib()
    if learnable:
        assert weight is not None and bias is not None
        weight = weight.contiguous()
        dweight, dbias = _new_dparam(x, weight, D), _new_dparam(x, weight, D)
        ws = _workspace(lib.mi355_hstu_layer_norm_bwd_workspace_bytes(rows, D), x.device)
    if wait_event is not None:
        wait_event.wait(torch.cuda.current_stream())
    N.check(lib.mi355_hstu_layer_norm_bwd(
        N.ptr(dy), _stride(dy), N.ptr(x), _stride(x), rows, D, N.dt(x), N.ptr(weight) if learnable else None,
        N.dt(weight) if learnable else N.dt(x), N.ptr(mean), N.ptr(rstd), N.ptr(acc), 0 if acc is None else _stride(acc),
        N.ptr(dx), D, N.ptr(dweight), N.ptr(dbias), N.ptr(ws), 0 if ws is None else ws.numel(), N.stream()),
        "mi355_hstu_layer_norm_bwd")
    return dx, dweight, dbias


def _draw_seed() -> int:
    # on the CPU generator, as the reference does (triton_norm_mul_dropout.py:397): torch.manual_seed governs it
    return int(torch.randint(low=0, high=2 ** 62, size=(1,), dtype=torch.int64).item())


def triton_layer_norm_mul_dropout_fwd(x: torch.Tensor, u: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float,
                                      dropout_ratio: float, training: bool, concat_ux: bool = False, seed: Optional[int] = None
                                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int, int, int]:
    """y = dropout(layer_norm(x) * u), or [dropout(u) | dropout(x) | dropout(ln * u)] with concat_ux;
    returns (y, mean, rstd, BLOCK_D, num_warps, seed)."""
    _check_rows(x)
    _require_gpu(x, u, weight, bias)
    x = _rows(x)
    rows, D = x.shape
    _check_params(weight, bias, D)
    weight, bias = weight.contiguous(), bias.contiguous()
    u, us0, us1, H, UD = _u_layout(u, D)
    y, mean, rstd = _new_y(x, 3 * D if concat_ux else D), _new_stat(x, rows), _new_stat(x, rows)
    if rows == 0:
        return y, mean, rstd, 0, 0, 0
    block_d, num_warps = _launch_params(D, x.element_size())
    if seed is None:
        seed = _draw_seed()
    N.check(N.lib().mi355_hstu_ln_mul_dropout_fwd(
        N.ptr(x), _stride(x), N.ptr(u), us0, us1, H, UD, rows, D, N.dt(x), N.ptr(weight), N.ptr(bias), N.dt(weight), float(eps),
        float(dropout_ratio), int(bool(training)), int(seed), int(bool(concat_ux)), N.ptr(y), y.size(1), N.ptr(mean), N.ptr(rstd),
        N.stream()), "mi355_hstu_ln_mul_dropout_fwd")
    return y, mean, rstd, block_d, num_warps, seed


def triton_layer_norm_mul_dropout_bwd(dy: torch.Tensor, x: torch.Tensor, u: torch.Tensor, weight: torch.Tensor,
                                      bias: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, BLOCK_D: int, num_warps: int,
                                      eps: float, training: bool, dropout_ratio: float, seed: Optional[int] = None,
                                      concat_ux: bool = False, compute_y: bool = False,
                                      wait_event: Optional[torch.cuda.Event] = None, du: Optional[torch.Tensor] = None
                                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(dx, du, dweight, dbias, y); `du`, when passed, is written in place with its own strides; y (compute_y) is the
    forward's output again, bit-equal."""
    _check_rows(x)
    _require_gpu(dy, x, u, weight, bias, mean, rstd, du)
    x, dy = _rows(x), _rows(dy)
    rows, D = x.shape
    _check_params(weight, bias, D)
    weight, bias = weight.contiguous(), bias.contiguous()
    u, us0, us1, H, UD = _u_layout(u, D)
    du, ds0, ds1 = _du_layout(du, u, D)
    y = _new_y(x, 3 * D if concat_ux else D) if compute_y else None
    dx, dweight, dbias = _new_y(x, D), _new_dparam(x, weight, D), _new_dparam(x, weight, D)
    lib = N.lib()
    ws = _workspace(lib.mi355_hstu_ln_mul_dropout_bwd_workspace_bytes(rows, D), x.device)
    if wait_event is not None:
        wait_event.wait(torch.cuda.current_stream())
    N.check(lib.mi355_hstu_ln_mul_dropout_bwd(
        N.ptr(dy), _stride(dy), N.ptr(x), _stride(x), N.ptr(u), us0, us1, H, UD, rows, D, N.dt(x), N.ptr(weight), N.ptr(bias),
        N.dt(weight), N.ptr(mean), N.ptr(rstd), float(dropout_ratio), int(bool(training)), int(seed or 0), int(bool(concat_ux)),
        N.ptr(dx), D, N.ptr(du), ds0, ds1, N.ptr(dweight), N.ptr(dbias), N.ptr(y), 0 if y is None else y.size(1), N.ptr(ws),
        ws.numel(), N.stream()), "mi355_hstu_ln_mul_dropout_bwd")
    return dx, du, dweight, dbias, y


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        y, mean, rstd, block_d, num_warps = triton_weighted_layer_norm_fwd(x=x, weight=weight, bias=bias, eps=eps)
        learnable = weight is not None
        if learnable:
            ctx.save_for_backward(x, weight, bias, mean, rstd)
        else:
            ctx.save_for_backward(x, mean, rstd)
        ctx.launch = (block_d, num_warps)
        ctx.eps, ctx.learnable = eps, learnable
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.learnable:
            x, weight, bias, mean, rstd = ctx.saved_tensors
        else:
            (x, mean, rstd), weight, bias = ctx.saved_tensors, None, None
        dx, dweight, dbias = triton_weighted_layer_norm_bwd(dy=dy, x=x, weight=weight, bias=bias, mean=mean, rstd=rstd,
                                                            learnable=ctx.learnable, eps=ctx.eps, BLOCK_D=ctx.launch[0],
                                                            num_warps=ctx.launch[1])
        return dx, dweight, dbias, None


class _LayerNormMulDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, weight, bias, eps, dropout_ratio, training, concat_ux, seed):
        y, mean, rstd, block_d, num_warps, seed = triton_layer_norm_mul_dropout_fwd(
            x=x, u=u, weight=weight, bias=bias, eps=eps, dropout_ratio=dropout_ratio, training=training, concat_ux=concat_ux,
            seed=seed)
        ctx.save_for_backward(x, u, weight, bias, mean, rstd)
        ctx.launch = (block_d, num_warps)
        ctx.eps, ctx.seed, ctx.training, ctx.concat_ux, ctx.dropout_ratio = eps, seed, training, concat_ux, dropout_ratio
        return y

    @staticmethod
    def backward(ctx, dy):
        x, u, weight, bias, mean, rstd = ctx.saved_tensors
        dx, du, dweight, dbias, _ = triton_layer_norm_mul_dropout_bwd(
            dy=dy, x=x, u=u, weight=weight, bias=bias, mean=mean, rstd=rstd, BLOCK_D=ctx.launch[0], num_warps=ctx.launch[1],
            eps=ctx.eps, training=ctx.training, dropout_ratio=ctx.dropout_ratio, seed=ctx.seed, concat_ux=ctx.concat_ux,
            compute_y=False)
        return dx, du, dweight, dbias, None, None, None, None, None


def _group_launch_params(linear_dim: int, num_heads: int, element_size: int) -> Tuple[int, int, int]:
    """BLOCK_D, BLOCK_H and num_warps of the reference (triton_norm_mul_dropout.py:877-887)"""
    block_d, block_h = _next_power_of_2(linear_dim), _next_power_of_2(num_heads)
    if block_d * block_h > 65536 // element_size:
        raise RuntimeError("This group norm doesn't support num_heads * linear_dim >= 64KB.")
    return block_d, block_h, min(max(block_d * block_h // 256, 1), 8)


def _check_group(x, u, weight, bias, num_heads, linear_dim):
    """(u, stride0, stride1) after the shape checks of the group norm"""
    _check_rows(x)
    if num_heads < 1 or linear_dim < 1 or x.shape[1] != num_heads * linear_dim:
        raise ValueError(f"x must have num_heads * linear_dim = {num_heads} * {linear_dim} columns, got {x.shape[1]}")
    if weight is None or weight.dim() != 1 or weight.numel() != num_heads:
        raise ValueError(f"weight must be 1-D with num_heads = {num_heads} elements")
    if bias is None or bias.dim() != 1 or bias.numel() != num_heads:
        raise ValueError(f"bias must be 1-D with num_heads = {num_heads} elements")
    if weight.dtype != bias.dtype:
        raise ValueError("weight and bias must share one dtype")
    if u.dim() == 3 and tuple(u.shape[1:]) != (num_heads, linear_dim):
        raise ValueError(f"a 3-D u must be [N, num_heads, linear_dim], got {tuple(u.shape)}")
    if u.size(0) != x.size(0) or u.numel() != x.numel():
        raise ValueError(f"u must hold the elements of x, got {tuple(u.shape)} for x {tuple(x.shape)}")
    u, s0, s1, _, _ = _u_layout(u, x.shape[1])
    return u, s0, (s1 if u.dim() == 3 else linear_dim)


def triton_group_norm_mul_dropout_fwd(x: torch.Tensor, u: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float,
                                      dropout_ratio: float, training: bool, concat_ux: bool = False, num_heads: int = 1,
                                      linear_dim: int = -1, seed: Optional[int] = None
                                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int, int, int, int]:
    """y = dropout(group_norm(x) * u) with num_heads groups of linear_dim columns and one weight / bias per group, or
    [dropout(u) | dropout(x) | dropout(gn * u)] with concat_ux; returns (y, mean, rstd, BLOCK_D, BLOCK_H, num_warps, seed)."""
    u, us0, us1 = _check_group(x, u, weight, bias, num_heads, linear_dim)
    _require_gpu(x, u, weight, bias)
    x = _rows(x)
    rows, D = x.shape
    weight, bias = weight.contiguous(), bias.contiguous()
    y, mean, rstd = _new_y(x, 3 * D if concat_ux else D), _new_stat(x, rows * num_heads), _new_stat(x, rows * num_heads)
    if rows == 0:
        return y, mean, rstd, 0, 0, 0, 0
    block_d, block_h, num_warps = _group_launch_params(linear_dim, num_heads, x.element_size())
    if seed is None:
        seed = _draw_seed()
    N.check(N.lib().mi355_hstu_gn_mul_dropout_fwd(
        N.ptr(x), _stride(x), N.ptr(u), us0, us1, num_heads, linear_dim, rows, D, N.dt(x), N.ptr(weight), N.ptr(bias),
        N.dt(weight), float(eps), float(dropout_ratio), int(bool(training)), int(seed), int(bool(concat_ux)), N.ptr(y), y.size(1),
        N.ptr(mean), N.ptr(rstd), N.stream()), "mi355_hstu_gn_mul_dropout_fwd")
    return y, mean, rstd, block_d, block_h, num_warps, seed


def triton_group_norm_mul_dropout_bwd(dy: torch.Tensor, x: torch.Tensor, u: torch.Tensor, weight: torch.Tensor,
                                      bias: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, BLOCK_D: int, BLOCK_H: int,
                                      num_warps: int, eps: float, training: bool, dropout_ratio: float,
                                      seed: Optional[int] = None, concat_ux: bool = False, num_heads: int = 1,
                                      linear_dim: int = -1, compute_y: bool = False, du: Optional[torch.Tensor] = None
                                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(dx, du, dweight, dbias, y); `du`, when passed, is written in place with its own strides; y (compute_y) is the
    forward's output again, bit-equal."""
    u, us0, us1 = _check_group(x, u, weight, bias, num_heads, linear_dim)
    _require_gpu(dy, x, u, weight, bias, mean, rstd, du)
    x, dy = _rows(x), _rows(dy)
    rows, D = x.shape
    weight, bias = weight.contiguous(), bias.contiguous()
    du, ds0, ds1 = _du_layout(du, u, D)
    if du.dim() == 2:
        ds1 = linear_dim
    y = _new_y(x, 3 * D if concat_ux else D) if compute_y else None
    dx, dweight, dbias = _new_y(x, D), _new_dparam(x, weight, num_heads), _new_dparam(x, weight, num_heads)
    lib = N.lib()
    ws = _workspace(lib.mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(rows, num_heads, linear_dim), x.device)
    N.check(lib.mi355_hstu_gn_mul_dropout_bwd(
        N.ptr(dy), _stride(dy), N.ptr(x), _stride(x), N.ptr(u), us0, us1, num_heads, linear_dim, rows, D, N.dt(x), N.ptr(weight),
        N.ptr(bias), N.dt(weight), N.ptr(mean), N.ptr(rstd), float(dropout_ratio), int(bool(training)), int(seed or 0),
        int(bool(concat_ux)), N.ptr(dx), D, N.ptr(du), ds0, ds1, N.ptr(dweight), N.ptr(dbias), N.ptr(y),
        0 if y is None else y.size(1), N.ptr(ws), ws.numel(), N.stream()), "mi355_hstu_gn_mul_dropout_bwd")
    return dx, du, dweight, dbias, y


class GroupNormMulDropoutFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, weight, bias, eps, dropout_ratio, training, concat_ux=False, num_heads=1, linear_dim=-1, seed=None):
        y, mean, rstd, block_d, block_h, num_warps, seed = triton_group_norm_mul_dropout_fwd(
            x=x, u=u, weight=weight, bias=bias, eps=eps, dropout_ratio=dropout_ratio, training=training, concat_ux=concat_ux,
            num_heads=num_heads, linear_dim=linear_dim, seed=seed)
        ctx.save_for_backward(x, u, weight, bias, mean, rstd)
        ctx.launch = (block_d, block_h, num_warps)
        ctx.eps, ctx.seed, ctx.training, ctx.concat_ux, ctx.dropout_ratio = eps, seed, training, concat_ux, dropout_ratio
        ctx.num_heads, ctx.linear_dim = num_heads, linear_dim
        return y

    @staticmethod
    def backward(ctx, dy):
        x, u, weight, bias, mean, rstd = ctx.saved_tensors
        dx, du, dweight, dbias, _ = triton_group_norm_mul_dropout_bwd(
            dy=dy, x=x, u=u, weight=weight, bias=bias, mean=mean, rstd=rstd, BLOCK_D=ctx.launch[0], BLOCK_H=ctx.launch[1],
            num_warps=ctx.launch[2], eps=ctx.eps, training=ctx.training, dropout_ratio=ctx.dropout_ratio, seed=ctx.seed,
            concat_ux=ctx.concat_ux, num_heads=ctx.num_heads, linear_dim=ctx.linear_dim, compute_y=False)
        return dx, du, dweight, dbias, None, None, None, None, None, None, None


def _check_weight(weight, D, name="weight"):
    if weight is None or weight.dim() != 1 or weight.numel() != D:
        raise ValueError(f"{name} must be 1-D with {D} elements")


def triton_swish_layer_norm_fwd(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float
                                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """y = x * sigmoid(layer_norm(x, weight, bias)); returns (y, mean, rstd).  (The reference has this only inside
    SwishLayerNormFunction, triton_layer_norm.py:763-816.)"""
    _check_rows(x)
    _check_weight(weight, x.shape[1])
    _check_weight(bias, x.shape[1], "bias")
    if weight.dtype != bias.dtype:
        raise ValueError("weight and bias must share one dtype")
    _require_gpu(x, weight, bias)
    x = _rows(x)
    rows, D = x.shape
    weight, bias = weight.contiguous(), bias.contiguous()
    y, mean, rstd = _new_y(x, D), _new_stat(x, rows), _new_stat(x, rows)
    N.check(N.lib().mi355_hstu_swish_layer_norm_fwd(
        N.ptr(x), _stride(x), rows, D, N.dt(x), N.ptr(weight), N.ptr(bias), N.dt(weight), float(eps), N.ptr(y), D, N.ptr(mean),
        N.ptr(rstd), N.stream()), "mi355_hstu_swish_layer_norm_fwd")
    return y, mean, rstd


def triton_swish_layer_norm_bwd(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, mean: torch.Tensor,
                                rstd: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dweight, dbias) of the swish layer norm"""
    _check_rows(x)
    _check_weight(weight, x.shape[1])
    _check_weight(bias, x.shape[1], "bias")
    _require_gpu(dy, x, weight, bias, mean, rstd)
    x, dy = _rows(x), _rows(dy)
    rows, D = x.shape
    weight, bias = weight.contiguous(), bias.contiguous()
    dx, dweight, dbias = _new_y(x, D), _new_dparam(x, weight, D), _new_dparam(x, weight, D)
    lib = N.lib()
    ws = _workspace(lib.mi355_hstu_swish_layer_norm_bwd_workspace_bytes(rows, D), x.device)
    N.check(lib.mi355_hstu_swish_layer_norm_bwd(
        N.ptr(dy), _stride(dy), N.ptr(x), _stride(x), rows, D, N.dt(x), N.ptr(weight), N.ptr(bias), N.dt(weight), N.ptr(mean),
        N.ptr(rstd), N.ptr(dx), D, N.ptr(dweight), N.ptr(dbias), N.ptr(ws), ws.numel(), N.stream()),
        "mi355_hstu_swish_layer_norm_bwd")
    return dx, dweight, dbias


def triton_rms_norm_fwd(x: torch.Tensor, weight: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """y = x * rstd * weight with rstd = 1 / sqrt(mean(x^2) + eps); returns (y, rstd).  (The reference has this only inside
    RMSNormFunction, triton_layer_norm.py:660-704.)"""
    _check_rows(x)
    _check_weight(weight, x.shape[1])
    _require_gpu(x, weight)
    x = _rows(x)
    rows, D = x.shape
    weight = weight.contiguous()
    y, rstd = _new_y(x, D), _new_stat(x, rows)
    N.check(N.lib().mi355_hstu_rms_norm_fwd(
        N.ptr(x), _stride(x), rows, D, N.dt(x), N.ptr(weight), N.dt(weight), float(eps), N.ptr(y), D, N.ptr(rstd), N.stream()),
        "mi355_hstu_rms_norm_fwd")
    return y, rstd


def triton_rms_norm_bwd(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, rstd: torch.Tensor
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dx, dweight) of the RMS norm"""
    _check_rows(x)
    _check_weight(weight, x.shape[1])
    _require_gpu(dy, x, weight, rstd)
    x, dy = _rows(x), _rows(dy)
    rows, D = x.shape
    weight = weight.contiguous()
    dx, dweight = _new_y(x, D), _new_dparam(x, weight, D)
    lib = N.lib()
    ws = _workspace(lib.mi355_hstu_rms_norm_bwd_workspace_bytes(rows, D), x.device)
    N.check(lib.mi355_hstu_rms_norm_bwd(
        N.ptr(dy), _stride(dy), N.ptr(x), _stride(x), rows, D, N.dt(x), N.ptr(weight), N.dt(weight), N.ptr(rstd), N.ptr(dx), D,
        N.ptr(dweight), N.ptr(ws), ws.numel(), N.stream()), "mi355_hstu_rms_norm_bwd")
    return dx, dweight


class SwishLayerNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        y, mean, rstd = triton_swish_layer_norm_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mean, rstd = ctx.saved_tensors
        dx, dweight, dbias = triton_swish_layer_norm_bwd(dy, x, weight, bias, mean, rstd)
        return dx, dweight, dbias, None


class RMSNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        y, rstd = triton_rms_norm_fwd(x, weight, eps)
        ctx.save_for_backward(x, weight, rstd)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, rstd = ctx.saved_tensors
        dx, dweight = triton_rms_norm_bwd(dy, x, weight, rstd)
        return dx, dweight, None


def triton_layer_norm(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    return _LayerNorm.apply(x, weight, bias, eps)


def triton_rms_norm(x: torch.Tensor, weight: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    return RMSNormFunction.apply(x, weight, eps)


def triton_swish_layer_norm(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], eps: float
                            ) -> torch.Tensor:
    return SwishLayerNormFunction.apply(x, weight, bias, eps)


def triton_norm_mul_dropout(x: torch.Tensor, u: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float,
                            dropout_ratio: float, training: bool, concat_ux: bool = False, group_norm: bool = False,
                            num_heads: int = 1, linear_dim: int = -1, seed: Optional[int] = None) -> torch.Tensor:
    """y = dropout(ln(x, weight, bias) * u); group_norm: the statistics and weight / bias are per head of linear_dim columns"""
    if group_norm:
        if not all(t.is_cuda for t in (x, u, weight, bias) if t is not None):
            raise NotImplementedError("group norm has no CPU implementation")
        return GroupNormMulDropoutFunction.apply(x, u, weight, bias, eps, dropout_ratio, training, concat_ux, num_heads,
                                                 linear_dim, seed)
    return _LayerNormMulDropout.apply(x, u, weight, bias, eps, dropout_ratio, training, concat_ux, seed)


layer_norm = triton_layer_norm
norm_mul_dropout = triton_norm_mul_dropout
weighted_layer_norm_fwd = triton_weighted_layer_norm_fwd
weighted_layer_norm_bwd = triton_weighted_layer_norm_bwd
layer_norm_mul_dropout_fwd = triton_layer_norm_mul_dropout_fwd
layer_norm_mul_dropout_bwd = triton_layer_norm_mul_dropout_bwd
group_norm_mul_dropout_fwd = triton_group_norm_mul_dropout_fwd
group_norm_mul_dropout_bwd = triton_group_norm_mul_dropout_bwd
swish_layer_norm = triton_swish_layer_norm
rms_norm = triton_rms_norm
swish_layer_norm_fwd = triton_swish_layer_norm_fwd
swish_layer_norm_bwd = triton_swish_layer_norm_bwd
rms_norm_fwd = triton_rms_norm_fwd
rms_norm_bwd = triton_rms_norm_bwd
