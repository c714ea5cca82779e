"""The two projections of the HSTU layer on MI355X: z = y + x @ w with an optional SiLU, forward and backward, with the
names, argument order, defaults and return tuples of the reference (examples/hstu/ops/triton_ops/triton_addmm.py:278-414,
ops/pt_ops/torch_addmm.py and triton_ops/triton_silu.py), over the kernels of csrc/act_ops.hip.

* `from hstu_addmm import torch_addmm_silu_fwd, triton_addmm_silu_fwd` is the import paged_hstu_infer_layer.py needs;
  fused_hstu_op.py of this package is built on the same functions.  Both forward names run one path here.
* The GEMMs are torch.addmm / torch.mm (hipBLASLt / rocBLAS), as the reference's backward GEMMs are cuBLAS; the bias or residual
  is the addend of the GEMM, written straight into `out` / `silu_out` when the caller passed one.
* Everything else is HIP: the SiLU (in place with keep_unfused_out=False), and in the backward ONE kernel that writes dz and,
  for a 1-D y, dy = sum(dz, 0) from the fp32 values before their rounding, in a fixed order (bitwise reproducible).
* `dz_out` is the one argument the reference lacks: the buffer dz is written into; it may be grad_output itself.
* There is no Triton here and no eager fallback: CPU tensors raise NativeError.
"""
from typing import Optional, Tuple

import torch

import mi355_native as N

__all__ = ["torch_addmm_silu_fwd", "triton_addmm_silu_fwd", "triton_addmm_silu_bwd", "triton_addmm", "triton_silu_fwd",
           "triton_silu_bwd", "triton_silu", "silu_bwd_dbias"]


def _require_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise N.NativeError("the HSTU projections expect GPU tensors (no CPU fallback exists)")


def _rows2d(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got {t.dim()}-D")
    if t.dtype not in N._DT:
        raise N.NativeError(f"unsupported dtype {t.dtype}")
    return t


def _unit_last(t: torch.Tensor) -> bool:
    return t.stride(1) == 1 or t.size(1) <= 1


def _stride(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


def _silu_into(z: torch.Tensor, s: torch.Tensor) -> None:
    rows, n = z.shape
    N.check(N.lib().mi355_hstu_silu_fwd(N.ptr(z), _stride(z), rows, n, N.dt(z), N.ptr(s), _stride(s), N.stream()),
            "mi355_hstu_silu_fwd")


def silu_bwd_dbias(grad_output: torch.Tensor, z: torch.Tensor, dz_out: Optional[torch.Tensor] = None, with_dbias: bool = True,
                   dbias_dtype: Optional[torch.dtype] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(dz, dbias) of s = silu(z) in one kernel: dz = g sig (1 + z (1 - sig)), dbias = sum over rows of dz before its rounding
    (None without with_dbias).  dz_out may be grad_output (in place)."""
    _rows2d(z, "z")
    _rows2d(grad_output, "grad_output")
    _require_gpu(grad_output, z, dz_out)
    if grad_output.shape != z.shape or grad_output.dtype != z.dtype:
        raise ValueError("grad_output and z must share shape and dtype")
    rows, n = z.shape
    if not _unit_last(z):
        z = z.contiguous()
    if dz_out is None:
        dz_out = torch.empty((rows, n), dtype=z.dtype, device=z.device)
    elif dz_out.shape != z.shape or dz_out.dtype != z.dtype or not _unit_last(dz_out):
        raise ValueError("dz_out must have the shape and dtype of z and a contiguous last dimension")
    if not _unit_last(grad_output):
        grad_output = grad_output.contiguous()
    lib = N.lib()
    dbias = ws = None
    if with_dbias:
        dbias = torch.empty((n,), dtype=dbias_dtype or z.dtype, device=z.device)
        ws = torch.empty(int(lib.mi355_hstu_silu_bwd_workspace_bytes(rows, n)), dtype=torch.uint8, device=z.device)
    N.check(lib.mi355_hstu_silu_bwd(
        N.ptr(grad_output), _stride(grad_output), N.ptr(z), _stride(z), rows, n, N.dt(z), N.ptr(dz_out), _stride(dz_out),
        N.ptr(dbias), N.dt(dbias) if with_dbias else N.dt(z), N.ptr(ws), 0 if ws is None else ws.numel(), N.stream()),
        "mi355_hstu_silu_bwd")
    return dz_out, dbias


def triton_addmm_silu_fwd(x: torch.Tensor, w: torch.Tensor, y: torch.Tensor, silu: bool = False, keep_unfused_out: bool = True,
                          out: torch.Tensor = None, silu_out: torch.Tensor = None
                          ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(z, silu(z) or None) with z = y + x @ w; y is [N] (a bias) or [M, N] (a residual).  The buffers are chosen as the
    reference chooses them: z is `out`, else `silu_out` unless keep_unfused_out asks for a buffer of its own; with
    keep_unfused_out=False and no separate buffers the SiLU runs in place and both results are one tensor."""
    _rows2d(x, "x")
    _rows2d(w, "w")
    _require_gpu(x, w, y, out, silu_out)
    rows, n = x.size(0), w.size(1)
    if x.size(1) != w.size(0):
        raise ValueError(f"x is {tuple(x.shape)} and w is {tuple(w.shape)}: the inner sizes differ")
    if y.dim() not in (1, 2) or y.size(-1) != n:
        raise ValueError(f"y must be [{n}] or [{rows}, {n}], got {tuple(y.shape)}")
    # z goes into `out`; failing that it shares silu_out, unless the caller wants the unfused values kept apart
    z = out
    if z is None:
        z = silu_out if silu_out is not None and not keep_unfused_out else x.new_empty((rows, n))
    act = None
    if silu:
        act = silu_out
        if act is None:
            act = torch.empty_like(z) if keep_unfused_out else z
        if not (_unit_last(z) and _unit_last(act)):
            raise ValueError("out and silu_out need a contiguous last dimension")
    if rows and n:
        torch.addmm(y, x, w, out=z)
        if silu:
            _silu_into(z, act)
    return z, act


torch_addmm_silu_fwd = triton_addmm_silu_fwd


def triton_addmm_silu_bwd(x: torch.Tensor, w: torch.Tensor, z: torch.Tensor, grad_output: torch.Tensor, is_y_1d: bool,
                          silu: bool = False, wgrad_stream: Optional[torch.cuda.Stream] = None,
                          wgrad_event: Optional[torch.cuda.Event] = None, dz_out: Optional[torch.Tensor] = None
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx, dw, dy) of z = y + x @ w (and silu(z) when `silu`).  One launch gives dz and the 1-D dy; dx = dz @ w.t() on the
    current stream; dw = x.t() @ dz on wgrad_stream when given, between wgrad_event.record / wait and a final record on that
    stream: the caller waits on wgrad_event before it reads dw."""
    _require_gpu(x, w, z, grad_output, dz_out)
    if (wgrad_stream is None) != (wgrad_event is None):
        raise ValueError("wgrad_stream and wgrad_event are given together or not at all")
    dy = None
    if silu:
        if z is None:
            raise ValueError("the SiLU backward needs z, the projection before its SiLU")
        dz, dy = silu_bwd_dbias(grad_output, z, dz_out=dz_out, with_dbias=is_y_1d)
    elif dz_out is None or dz_out is grad_output:
        dz = grad_output
    else:
        dz = dz_out.copy_(grad_output)
    if not is_y_1d:
        dy = dz
    elif dy is None:
        dy = dz.sum(0)
    dw = _weight_grad(x, dz, wgrad_stream, wgrad_event)
    return dz @ w.t(), dw, dy


def _weight_grad(x: torch.Tensor, dz: torch.Tensor, side: Optional[torch.cuda.Stream],
                 event: Optional[torch.cuda.Event]) -> torch.Tensor:
    """x.t() @ dz, on `side` when one is given.  `event` is recorded on the current stream and awaited by `side` before the
    GEMM, then recorded on `side` behind it: whoever reads the result waits on it.  Both streams are told of the tensors the
    other one made, so the caching allocator hands neither block out again while it is still in use."""
    if side is None:
        return x.t() @ dz
    here = torch.cuda.current_stream()
    event.record(here)
    with torch.cuda.stream(side):
        side.wait_event(event)
        dw = x.t() @ dz
        event.record(side)
    for t in (x, dz):
        t.record_stream(side)
    dw.record_stream(here)
    return dw


class _Projection(torch.autograd.Function):
    """triton_addmm's autograd node: the bias or residual comes first, as in torch.addmm"""

    @staticmethod
    def forward(ctx, y, x, w, silu):
        z, act = triton_addmm_silu_fwd(x, w, y, silu)
        ctx.bias_like, ctx.silu = y.dim() == 1, silu
        if silu:
            ctx.save_for_backward(x, w, z)
            return act
        ctx.save_for_backward(x, w)
        return z

    @staticmethod
    def backward(ctx, grad):
        x, w, *rest = ctx.saved_tensors
        dx, dw, dy = triton_addmm_silu_bwd(x, w, rest[0] if rest else None, grad, ctx.bias_like, ctx.silu)
        return dy, dx, dw, None


def triton_addmm(input: torch.Tensor, mat1: torch.Tensor, mat2: torch.Tensor, silu: bool = False) -> torch.Tensor:
    """input + mat1 @ mat2, then SiLU when asked, differentiable"""
    return _Projection.apply(input, mat1, mat2, silu)


def _as_rows(t: torch.Tensor) -> torch.Tensor:
    """any tensor as [rows, last] for the row kernels (a copy only when it is not contiguous)"""
    t = t.contiguous()
    return t.view(-1, t.size(-1)) if t.dim() >= 2 else t.view(1, -1)


def triton_silu_fwd(input: torch.Tensor) -> torch.Tensor:
    _require_gpu(input)
    if input.dtype not in N._DT:
        raise N.NativeError(f"unsupported dtype {input.dtype}")
    rows = _as_rows(input)
    out = torch.empty_like(rows)
    _silu_into(rows, out)
    return out.view(input.shape)


def triton_silu_bwd(grad_output: torch.Tensor, input: torch.Tensor) -> torch.Tensor:
    _require_gpu(grad_output, input)
    if input.dtype not in N._DT:
        raise N.NativeError(f"unsupported dtype {input.dtype}")
    dz, _ = silu_bwd_dbias(_as_rows(grad_output), _as_rows(input), with_dbias=False)
    return dz.view(input.shape)


class _SiluFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input):
        ctx.save_for_backward(input)
        return triton_silu_fwd(input)

    @staticmethod
    def backward(ctx, grad_output):
        (input,) = ctx.saved_tensors
        return triton_silu_bwd(grad_output, input)


def triton_silu(input: torch.Tensor) -> torch.Tensor:
    return _SiluFunction.apply(input)
