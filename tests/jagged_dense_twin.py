"""CPU restatement of the jagged x dense ops (csrc/jagged_bmm.hip) in float64, as per-sample loops in plain torch: the jagged x
dense product with its optional bias, its three gradients, the broadcast add and the per-sample row sum, with the magnitudes
their bounds need and the bounds themselves.  Inputs are upcast as they are.  Rows at or past offsets[-1] belong to no sample:
they are never read, and their rows of `out` and of `d_jagged` are zero.

Symbols: u the unit roundoff of the dtype written (2^-8 bf16, 2^-11 fp16, 2^-24 fp32), h = 2^-24 (half an fp32 ulp, relative),
sub half the smallest subnormal of the dtype written, mag the float64 sum of |a_i| |b_i| over the summands of an element (plus
|bias| where there is one), n the number of summands: K (K + 1 with a bias) for out, N for d_jagged, len_b for d_dense and d_bias.

  GEMM elements, bf16 / fp16 operands    |x - ref| <= u |ref| + 2 n h mag + sub
      The products are exact in fp32 (two 8- or 11-bit significands give at most 22 bits; no overflow or underflow at the test
      magnitudes).  Each of the n accumulations into the fp32 sum may err by a whole ulp of a partial sum that is never larger
      than mag, 2 h mag, in whatever order they are made: the MFMA's internal accumulate is not documented as round-to-nearest.
      Then the one rounding of the result, u |ref| (its argument is within the other terms of ref), and sub where it underflows.
  GEMM elements, fp32 operands           the same with n + 1 in place of n: each product is rounded too, h mag in all.
  d_bias                                 the GEMM form with n = len_b and mag = sum |d_out| (a product with an exact 1).
  broadcast add                          u |ref| + sub: one fp32 add, exact for 16-bit inputs up to its rounding, one rounding.
                                         (fp32: the add is the rounding.)
  row sums                               the form of norm_twin.bound_db: u |ref| + (n + 1) h mag + sub, mag = sum |x| over the
                                         sample's n rows: n fp32 additions of exact addends in any order, then the rounding.
Every bound is a function of float64 magnitudes of the inputs and the reference, never of the result under test.
"""
from types import SimpleNamespace

import torch

from act_twin import sub  # noqa: F401  (half the smallest subnormal of a dtype)
from norm_twin import unit_roundoff, worst  # noqa: F401  (worst: for the tests)

H32 = 2.0 ** -24


def _d(t):
    return None if t is None else t.detach().cpu().double()


def _bounds_of(offsets):
    """[(start, end)] per sample from offsets given as a list or a tensor"""
    o = [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    return list(zip(o[:-1], o[1:]))


def lengths_of(offsets):
    return torch.tensor([e - s for s, e in _bounds_of(offsets)], dtype=torch.float64)


def bmm_fwd(offsets, jagged, dense, bias=None):
    """out [L, N] and its mag; n = K (+ 1 with a bias)"""
    J, D, Bv = _d(jagged), _d(dense), _d(bias)
    out = torch.zeros(J.size(0), D.size(2), dtype=torch.float64)
    mag = torch.zeros_like(out)
    for b, (s, e) in enumerate(_bounds_of(offsets)):
        out[s:e] = J[s:e] @ D[b]
        mag[s:e] = J[s:e].abs() @ D[b].abs()
        if Bv is not None:
            out[s:e] += Bv[b]
            mag[s:e] += Bv[b].abs()
    return SimpleNamespace(out=out, mag=mag, n=D.size(1) + (0 if bias is None else 1))


def bmm_bwd(offsets, jagged, dense, d_out, with_bias=False):
    """d_jagged [L, K], d_dense [B, K, N], d_bias [B, N] (None without a bias), each with its mag; lengths [B]"""
    J, D, G = _d(jagged), _d(dense), _d(d_out)
    st = SimpleNamespace(d_jagged=torch.zeros_like(J), d_jagged_mag=torch.zeros_like(J), d_dense=torch.zeros_like(D),
                         d_dense_mag=torch.zeros_like(D), d_bias=None, d_bias_mag=None, lengths=lengths_of(offsets),
                         n_jagged=D.size(2))
    if with_bias:
        st.d_bias = torch.zeros(D.size(0), D.size(2), dtype=torch.float64)
        st.d_bias_mag = torch.zeros_like(st.d_bias)
    for b, (s, e) in enumerate(_bounds_of(offsets)):
        st.d_jagged[s:e] = G[s:e] @ D[b].t()
        st.d_jagged_mag[s:e] = G[s:e].abs() @ D[b].abs().t()
        st.d_dense[b] = J[s:e].t() @ G[s:e]
        st.d_dense_mag[b] = J[s:e].abs().t() @ G[s:e].abs()
        if with_bias:
            st.d_bias[b] = G[s:e].sum(0)
            st.d_bias_mag[b] = G[s:e].abs().sum(0)
    return st


def broadcast_add(offsets, jagged, dense):
    J, D = _d(jagged), _d(dense)
    out = torch.zeros_like(J)
    for b, (s, e) in enumerate(_bounds_of(offsets)):
        out[s:e] = J[s:e] + D[b]
    return out


def row_sum(offsets, rows):
    """sums [B, D] and their mag; lengths [B]"""
    R = _d(rows)
    B = len(_bounds_of(offsets))
    st = SimpleNamespace(sum=torch.zeros(B, R.size(1), dtype=torch.float64), lengths=lengths_of(offsets))
    st.mag = torch.zeros_like(st.sum)
    for b, (s, e) in enumerate(_bounds_of(offsets)):
        st.sum[b] = R[s:e].sum(0)
        st.mag[b] = R[s:e].abs().sum(0)
    return st


# ---- the bounds ----
def bound_gemm(ref, mag, n, dtype):
    """n: a number, or a tensor that broadcasts against ref (len_b per sample).  dtype: of the operands and of the result."""
    n = n + 1 if dtype == torch.float32 else n
    return unit_roundoff(dtype) * ref.abs() + 2 * n * H32 * mag + sub(dtype)


def bound_add(ref, dtype):
    return unit_roundoff(dtype) * ref.abs() + sub(dtype)


def bound_row_sum(st, dtype):
    return unit_roundoff(dtype) * st.sum.abs() + (st.lengths[:, None] + 1) * H32 * st.mag + sub(dtype)
