"""FP8 HSTU attention, the parts that need no device: the fp64 emulation of tests/test_hstu_fp8_gpu.py against the
dequantised values of the reference's quantisers (tests/golden/hstu_fp8_quant_golden.npz), the error bound, and the
argument checks that run before any launch."""
import importlib.util
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("hstu_fp8_gpu_suite", os.path.join(HERE, "test_hstu_fp8_gpu.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _golden_kw(case, mode, which_bs=None):
    z = np.load(G.GOLDEN)
    p = case + "/"
    f16, T, H, D = (int(v) for v in z[p + "meta"])
    f8 = lambda a: torch.from_numpy(a.copy()).view(torch.float8_e4m3fn)
    f32 = lambda a: torch.from_numpy(a.copy())
    x = torch.from_numpy(z[p + "x"].view(np.int16).copy()).view(torch.float16 if f16 else torch.bfloat16)
    off = z[p + "offsets"]
    if mode == 1:
        kw = dict(q=f8(z[p + "m1_x"]), k=f8(z[p + "m1_x"]), vt=f8(z[p + "m1_xt"]), descale_q=f32(z[p + "m1_descale"]),
                  descale_k=f32(z[p + "m1_descale"]), descale_vt=f32(z[p + "m1_descale_xt"]),
                  cu_seqlens_descale_vt=torch.from_numpy(z[p + "m1_cu"]))
        kw["v"] = kw["vt"]
    elif mode == 2:
        bm, bn = (int(v) for v in z[p + "m2_blocks"])
        kw = dict(q=f8(z[p + f"m2_{bm}_x"]), k=f8(z[p + f"m2_{bn}_x"]), v=f8(z[p + f"m2_{bn}_x"]),
                  descale_q=f32(z[p + f"m2_{bm}_descale"]), descale_k=f32(z[p + f"m2_{bn}_descale"]),
                  descale_v=f32(z[p + f"m2_{bn}_descale"]), cu_seqlens_block_descale_q=torch.from_numpy(z[p + f"m2_{bm}_cu"]),
                  cu_seqlens_block_descale_kv=torch.from_numpy(z[p + f"m2_{bn}_cu"]))
    elif mode == 0:
        kw = dict(q=f8(z[p + "m0_x"]), k=f8(z[p + "m0_x"]), v=f8(z[p + "m0_x"]))
    else:
        kw = dict(q=f8(z[p + f"m{mode}_x"]), k=f8(z[p + f"m{mode}_x"]), v=f8(z[p + f"m{mode}_x"]),
                  descale_q=f32(z[p + f"m{mode}_descale"]), descale_k=f32(z[p + f"m{mode}_descale"]),
                  descale_v=f32(z[p + f"m{mode}_descale"]))
    return x, off, kw


@pytest.mark.parametrize("mode", range(6))
@pytest.mark.parametrize("case", G._golden_cases())
def test_emulation_dequantises_to_the_input(case, mode):
    """the dequantised golden operands equal the input up to e4m3's rounding: 2^-4 relative, or half the subnormal step
    times the descale (which is what the emulation reads from each mode's descale layout)"""
    x, off, kw = _golden_kw(case, mode)
    x = x.double()
    for which in ("q", "v"):
        deq = G.dequantize(kw, mode, torch.from_numpy(off), which)
        if mode == 0:
            step = torch.ones_like(x)
        else:
            step = (deq.abs() > 0).double()
            nz = x.abs() > 0
            # the scale of each element: its dequantised value over its fp8 value where that is nonzero
            f = (kw["vt"] if (mode == 1 and which == "v") else kw[which]).double()
            sc = torch.where(f != 0, deq / torch.where(f != 0, f, torch.ones_like(f)), torch.zeros_like(f))
            step = sc.abs().max().expand_as(x) if not nz.any() else sc.abs()
            step = torch.where(sc == 0, torch.full_like(sc, float(sc.abs().max())), step)
        err = (deq - x).abs()
        assert (err <= 2.0 ** -4 * x.abs() + 2.0 ** -10 * step + 1e-30).all(), f"{case} mode {mode} {which}"


def test_emulation_bound_is_tight_on_exact_data_and_catches_a_wrong_descale():
    """exact fp8 operands and power-of-two descales: the emulation is exact in fp64; one wrong descale breaks the bound"""
    gen = torch.Generator().manual_seed(7)
    lengths, H, d = [70, 33], 2, 64
    off = torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32)
    T = int(off[-1])
    kw = dict(q=G._fp8_values((T, H, d), gen, "cpu"), k=G._fp8_values((T, H, d), gen, "cpu"),
              v=G._fp8_values((T, H, d), gen, "cpu"), descale_q=torch.tensor([[1.0, 2.0], [0.5, 4.0]]),
              descale_k=torch.ones(2, 2), descale_v=torch.ones(2, 2))
    emu, bound = G.emulate(kw, 3, off, 0.125, 70.0)
    assert torch.isfinite(emu).all() and (bound > 0).all()
    assert not G.violations(emu, emu, bound).any()
    kw2 = dict(kw, descale_q=torch.tensor([[1.0, 2.0], [0.5, 8.0]]))
    emu2, _ = G.emulate(kw2, 3, off, 0.125, 70.0)
    assert G.violations(emu2, emu, bound).any()
    # the bound is relative: 2^-4 of |P||V| dominates, the 2^-11 output term and the floor are small
    assert float((bound - 1e-6).max()) <= float(2.0 ** -3 * (emu.abs().max() + 1.0) * 64)


def test_emulation_mask_matches_the_oracle_rules():
    m = G.seq_mask(10, 0, torch.tensor([2]), torch.tensor([3]), 2, (-1, 0), "cpu")
    assert m[0, 6] and not m[0, 7]          # a contextual row sees the whole history, not the targets
    assert m[8, 7] and not m[9, 7] and m[9, 9]   # targets: groups of 2 from position 7
    w = G.seq_mask(10, 0, None, None, 1, (2, 1), "cpu")
    assert w[5, 3] and not w[5, 2] and w[5, 6] and not w[5, 7]


def test_argument_checks_before_any_launch():
    import hstu

    x = torch.zeros(10, 2, 64, dtype=torch.bfloat16)
    off = torch.tensor([0, 10], dtype=torch.int32)
    with pytest.raises(ValueError, match="three dimensions"):
        hstu.quantize_for_block_scale(x[0], off)
    with pytest.raises(NotImplementedError, match="e4m3fn"):
        hstu.quantize_for_head_batch_tensor(x, off, 3, fp8_type=torch.float8_e5m2)
    with pytest.raises(ValueError, match="3, 4 or 5"):
        hstu.quantize_for_head_batch_tensor(x, off, quant_mode=2)
    assert hstu.get_bm_and_bn_block_size_fwd(None, 64) == (128, 128)
    assert hstu.get_bm_and_bn_block_size_fwd(None, 128) == (128, 128)
    assert hstu.get_bm_and_bn_block_size_fwd(None, 256) == (128, 64)
    assert hstu.get_bm_and_bn_block_size_fwd(x, 128) == (128, 64)
    for bad in (6, -2, 1.0, True, "1"):
        with pytest.raises(ValueError, match="quant_mode"):
            hstu.hstu_attn_varlen_func(x, x, x, off, off, None, None, 10, 10, None, None, None, quant_mode=bad)
    rab = torch.zeros(1, 2, 10, 10, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="rab"):
        hstu.hstu_attn_varlen_func(x, x, x, off, off, None, None, 10, 10, None, None, None, rab=rab, quant_mode=0)
    with pytest.raises(NotImplementedError, match="func"):
        hstu.hstu_attn_varlen_func(x, x, x, off, off, None, None, 10, 10, None, None, None,
                                   func=torch.zeros(1, 1, 10, dtype=torch.int32), quant_mode=0)
    with pytest.raises(NotImplementedError, match="delta-q"):
        hstu.hstu_attn_varlen_func(x[:5], x, x, torch.tensor([0, 5], dtype=torch.int32), off, None, None, 5, 10, None, None,
                                   None, quant_mode=2)
    x32 = torch.zeros(10, 2, 32, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="head dimension 32"):
        hstu.hstu_attn_varlen_func(x32, x32, x32, off, off, None, None, 10, 10, None, None, None, quant_mode=5)
    x8 = x.to(torch.float8_e4m3fn)
    with pytest.raises(NotImplementedError, match="rab"):
        hstu.varlen_fwd(x8, x8, x8, off, off, 10, 10, None, None, None, 1, -1, 0, 1.0, rab, None, 3)
    with pytest.raises(NotImplementedError, match="e4m3fn"):
        hstu.varlen_fwd(x.to(torch.float8_e5m2), x8, x8, off, off, 10, 10, None, None, None, 1, -1, 0, 1.0, None, None, 3)
    with pytest.raises(ValueError, match="quant_mode"):
        hstu.varlen_fwd(x8, x8, x8, off, off, 10, 10, None, None, None, 1, -1, 0, 1.0, None, None, -1)
    from hstu import hstu_ops_gpu   # (the body of torch.ops.fbgemm.hstu_varlen_fwd_90; the op itself dispatches on device tensors)
    with pytest.raises(NotImplementedError, match="fp8"):
        hstu_ops_gpu._fwd_90(x8, x8, x8, off, off, None, None, 10, 10, 1.0, None, None, 1, -1, 0, 1.0, None,
                                            None, -1, 0)
