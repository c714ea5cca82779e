"""The backward writes dq / dk / dv where the caller says (strided views into one buffer: the packed dqkv of
hstu_attn_qkvpacked_func, the fused layer's duvqk split) instead of into three fresh tensors that are copied afterwards.

Strides change addresses, not arithmetic: the yardstick is the existing contiguous path (itself held to the oracle by
tests/test_hstu_gpu.py, test_hstu_long_gpu.py, test_hstu_delta_q_bwd_gpu.py) and EVERY comparison here is torch.equal.
Buffers around the views are filled with a sentinel: a store at a wrong stride lands in a guard slot or leaves the sentinel
in a gradient."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.0
LENS_A = [37, 1, 130]


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def _rand(seed, *shape, dtype=torch.bfloat16, lo=-1.0, hi=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(DEV).to(dtype)


def _func3(lens, extra=16):
    """n_func = 3: token i of a sequence sees the keys j < i // 2 + 1 and the band i + 2 <= j < i + 6 (clipped to the sequence)"""
    cols = []
    for L in lens:
        i = np.arange(L)
        cols.append(np.stack([i // 2 + 1, np.minimum(i + 2, L), np.minimum(i + 6, L)]))
    f = np.concatenate(cols + [np.zeros((3, extra), np.int64)], axis=1).astype(np.int32)
    return torch.from_numpy(f[None]).to(DEV)


def _packed_vs_unpacked(lens, H, d, dtype=torch.bfloat16, rab=False, func=False, **kw):
    from hstu import hstu_attn_qkvpacked_func, hstu_attn_varlen_func

    cu, T, N = _cu(lens), int(sum(lens)), int(max(lens))
    qkv = _rand(1, T, 3, H, d, dtype=dtype)
    dout = _rand(2, T, H, d, dtype=dtype, lo=0.0)
    kw = dict(kw, alpha=1.0 / d ** 0.5)
    if func:
        kw["func"] = _func3(lens)
    rabs = [None, None]
    if rab:
        r = _rand(3, len(lens), H, N, N, dtype=dtype, lo=-2.0, hi=2.0)
        rabs = [r.clone().requires_grad_(), r.clone().requires_grad_()]
    # the yardstick: three contiguous tensors through hstu_attn_varlen_func
    q, k, v = (qkv[:, i].contiguous().requires_grad_() for i in range(3))
    vk = dict(kw)
    out_u = hstu_attn_varlen_func(q, k, v, cu, cu, None, None, N, N, N, vk.pop("num_contexts", None), vk.pop("num_targets", None),
                                  rab=rabs[0], has_drab=rab, **vk)
    out_u.backward(dout)
    packed = qkv.clone().requires_grad_()
    out_p = hstu_attn_qkvpacked_func(packed, cu, cu, N, N, rab=rabs[1], has_drab=rab, **kw)
    out_p.backward(dout)
    assert torch.equal(out_p, out_u)
    assert packed.grad.shape == qkv.shape and packed.grad.is_contiguous()
    for i, (name, t) in enumerate((("dq", q), ("dk", k), ("dv", v))):
        assert torch.equal(packed.grad[:, i], t.grad), f"{name} of the packed call differs from the contiguous call"
    assert bool(torch.isfinite(packed.grad.float()).all()) and bool(packed.grad.float().abs().sum() > 0)
    if rab:
        assert torch.equal(rabs[1].grad, rabs[0].grad)


def test_packed_case_a_contexts_and_targets():
    _packed_vs_unpacked(LENS_A, 2, 64, window_size=(-1, 0), num_contexts=_i32([2, 0, 3]), num_targets=_i32([4, 0, 5]),
                        target_group_size=2)


@pytest.mark.parametrize("d", [32, 128])
def test_packed_case_b_fp16(d):
    _packed_vs_unpacked(LENS_A, 2, d, dtype=torch.float16, window_size=(-1, 0))


def test_packed_case_c_d256_triangular_exchange():
    _packed_vs_unpacked([129, 300], 2, 256, window_size=(-1, 0))


def test_packed_case_d_d256_square_exchange():
    _packed_vs_unpacked([129, 300], 2, 256, window_size=(-1, 0), num_contexts=_i32([3, 0]))


def test_packed_case_e_past_1024_rows():
    _packed_vs_unpacked([1056], 1, 256, window_size=(-1, 0))


@pytest.mark.parametrize("d", [64, 256])
def test_packed_case_f_window(d):
    _packed_vs_unpacked(LENS_A, 2, d, window_size=(8, 3))


def test_packed_case_g_rab_with_drab():
    _packed_vs_unpacked(LENS_A, 2, 64, rab=True, window_size=(-1, 0))


def test_packed_case_h_func():
    _packed_vs_unpacked(LENS_A, 2, 64, func=True, window_size=(-1, -1))


def test_packed_func_next_to_rab():
    _packed_vs_unpacked(LENS_A, 2, 64, rab=True, func=True, window_size=(-1, -1))


def _bwd_80(dout, q, k, v, cu, N, dq, dk, dv, alpha):
    return torch.ops.fbgemm.hstu_varlen_bwd_80(dout, q, k, v, cu, cu, None, None, N, N, float(N), dq, dk, dv, None, None, 1, -1, 0,
                                               alpha, None, False, None, False)


def _bwd_90(dout, q, k, v, cu, N, dq, dk, dv, alpha):
    return torch.ops.fbgemm.hstu_varlen_bwd_90(dout, None, q, None, k, None, v, cu, cu, None, None, N, N, float(N), dq, dk, dv, None,
                                               None, 1, -1, 0, alpha, -1, None, False, None, *([None] * 11), 0, False)


def _uvqk_views(buf, H, d):
    """the u / v / q / k slots of a (T, 4 H d) buffer as the fused layer splits its (d)uvqk, the last three viewed (T, H, d)"""
    u, v, q, k = buf.split([H * d] * 4, dim=-1)
    return u, q.view(-1, H, d), k.view(-1, H, d), v.view(-1, H, d)


@pytest.mark.parametrize("op", [_bwd_80, _bwd_90], ids=["80", "90"])
@pytest.mark.parametrize("strided_inputs", [False, True], ids=["contiguous_inputs", "inputs_in_uvqk"])
def test_fused_layer_layout_through_the_raw_op(op, strided_inputs):
    import hstu  # noqa: F401 (registers the ops)

    lens, H, d = [129, 300, 83], 2, 256
    cu, T, N, alpha = _cu(lens), sum(lens), max(lens), 1.0 / 16
    uvqk = _rand(4, T, 4 * H * d)
    _, q, k, v = _uvqk_views(uvqk, H, d)
    dout = _rand(5, T, H, d, lo=0.0)
    with torch.no_grad():
        want = op(dout, q.contiguous(), k.contiguous(), v.contiguous(), cu, N, None, None, None, alpha)
        assert all(w.is_contiguous() for w in want[:3])
        if not strided_inputs:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        buf = torch.full((T, 4 * H * d), SENTINEL, dtype=torch.bfloat16, device=DEV)
        du, dq, dk, dv = _uvqk_views(buf, H, d)
        assert dq.stride() == (4 * H * d, d, 1) and not dq.is_contiguous()
        got = op(dout, q, k, v, cu, N, dq, dk, dv, alpha)
    for g, given, w, name in zip(got[:3], (dq, dk, dv), want[:3], "qkv"):
        assert g.data_ptr() == given.data_ptr() and g.stride() == given.stride(), f"d{name} is not the given view"
        assert torch.equal(given, w), f"d{name} written through the view differs from the contiguous call"
    assert bool((du == SENTINEL).all()), "the u slot of the buffer was written: a store used a wrong stride"


def test_no_temporaries():
    """in place, the op allocates the exchange scratch and nothing else (it used to allocate three gradients and copy them)"""
    import hstu  # noqa: F401
    import mi355_native as N_
    from hstu import hstu_attn_interface as I

    B, L, H, d = 4, 512, 4, 256
    cu, T, alpha = _cu([L] * B), B * L, 1.0 / 16
    q, k, v = (_rand(6 + i, T, H, d) for i in range(3))
    dout = _rand(9, T, H, d, lo=0.0)
    buf = torch.full((T, 4 * H * d), SENTINEL, dtype=torch.bfloat16, device=DEV)
    du, dq, dk, dv = _uvqk_views(buf, H, d)
    ws = int(N_.lib().mi355_hstu_attn_bwd_ds_bytes(B, H, d, L))
    assert 0 < ws <= I._DS_MAX_BYTES            # (the dense layout: what _bwd_exchange_workspace allocates at this shape)
    one_gradient = T * H * d * 2
    assert one_gradient == 4 << 20
    with torch.no_grad():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        got = _bwd_80(dout, q, k, v, cu, L, dq, dk, dv, alpha)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    print(f"peak - base = {peak} bytes; exchange scratch = {ws}; one gradient = {one_gradient}")
    assert peak < ws + one_gradient
    assert got[0].data_ptr() == dq.data_ptr() and bool((du == SENTINEL).all()) and not bool((buf[:, H * d:] == SENTINEL).all())


@pytest.mark.parametrize("rab", [False, True], ids=["plain", "rab_drab"])
def test_delta_q_backward_into_strided_views(rab):
    from hstu import hstu_varlen_bwd_kv

    LQ, LK, H, d = [5, 0, 40], [37, 9, 130], 2, 64
    cuq, cuk, Tq, Tk, Nq, Nk = _cu(LQ), _cu(LK), sum(LQ), sum(LK), max(LQ), max(LK)
    q, dout = _rand(10, Tq, H, d), _rand(11, Tq, H, d, lo=0.0)
    k, v = _rand(12, Tk, H, d), _rand(13, Tk, H, d)
    bias = _rand(14, len(LK), H, Nk, Nk, lo=-2.0, hi=2.0) if rab else None
    args = (dout, q, k, v, cuq, cuk, Nq, Nk, float(Nk), None, None, 1, -1, 0, 1.0 / 8, bias, rab)
    want = hstu_varlen_bwd_kv(*args)
    qbuf = torch.full((Tq, 2 * H * d), SENTINEL, dtype=torch.bfloat16, device=DEV)
    kbuf = torch.full((Tk, 3 * H * d), SENTINEL, dtype=torch.bfloat16, device=DEV)
    dq = qbuf[:, H * d:].view(Tq, H, d)
    gk, dk, dv = (t.view(Tk, H, d) for t in kbuf.split([H * d] * 3, dim=-1))
    got = hstu_varlen_bwd_kv(*args, dq=dq, dk=dk, dv=dv)
    for g, given, w, name in zip(got[:3], (dq, dk, dv), want[:3], "qkv"):
        assert g.data_ptr() == given.data_ptr() and torch.equal(given, w), f"d{name}"
    # the sequence without queries: its keys receive zeros, at the strided address
    assert not bool(dk[LK[0]:LK[0] + LK[1]].any()) and not bool(dv[LK[0]:LK[0] + LK[1]].any())
    assert bool((qbuf[:, :H * d] == SENTINEL).all()) and bool((gk == SENTINEL).all())
    if rab:
        assert torch.equal(got[3], want[3])
    else:
        assert got[3] is None


def test_no_stale_strides_reach_the_next_backward():
    from hstu import hstu_attn_varlen_func, hstu_varlen_bwd

    # the ordinary call that follows, at another shape: its expected gradients first
    lens2, H2, d2 = [50, 20], 4, 32
    cu2, T2, N2 = _cu(lens2), sum(lens2), max(lens2)
    q2, k2, v2 = (_rand(20 + i, T2, H2, d2) for i in range(3))
    dout2 = _rand(23, T2, H2, d2, lo=0.0)

    def ordinary():
        qq, kk, vv = (t.clone().requires_grad_() for t in (q2, k2, v2))
        hstu_attn_varlen_func(qq, kk, vv, cu2, cu2, None, None, N2, N2, N2, None, None, 1, (-1, 0), 0.2).backward(dout2)
        return qq.grad, kk.grad, vv.grad

    want = ordinary()
    lens, H, d = LENS_A, 2, 64
    cu, T, N = _cu(lens), sum(lens), max(lens)
    q, k, v = (_rand(30 + i, T, H, d) for i in range(3))
    buf = torch.full((T, 4 * H * d), SENTINEL, dtype=torch.bfloat16, device=DEV)
    _, dq, dk, dv = _uvqk_views(buf, H, d)
    hstu_varlen_bwd(_rand(33, T, H, d, lo=0.0), q, k, v, cu, N, float(N), None, None, 1, True, 0.125, dq=dq, dk=dk, dv=dv)
    got = ordinary()
    for g, w in zip(got, want):
        assert g.is_contiguous() and torch.equal(g, w)


def test_a_view_the_kernels_cannot_address_is_filled_through_a_copy():
    from hstu import hstu_varlen_bwd

    lens, H, d = LENS_A, 2, 64
    cu, T, N = _cu(lens), sum(lens), max(lens)
    q, k, v = (_rand(40 + i, T, H, d) for i in range(3))
    dout = _rand(43, T, H, d, lo=0.0)
    args = (dout, q, k, v, cu, N, float(N), None, None, 1, True, 0.125)
    want = hstu_varlen_bwd(*args)
    buf = torch.full((T, H * d + 4), SENTINEL, dtype=torch.bfloat16, device=DEV)
    dq = buf[:, :H * d].view(T, H, d)
    assert dq.stride(0) == H * d + 4          # no multiple of 8 elements: not 16-byte rows
    got = hstu_varlen_bwd(*args, dq=dq)
    assert got[0] is dq and torch.equal(dq, want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert bool((buf[:, H * d:] == SENTINEL).all())
