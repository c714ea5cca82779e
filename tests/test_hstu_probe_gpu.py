"""The mask probes of tests/hstu_probe.py through the public entry points of the HSTU attention kernels: every case of hstu_probe.CASES
(tests/test_hstu_probe_cpu.py proves, without a device, that each has teeth: one wrong (query, key) pair is at least twice the standing
tolerance wherever it lands).  Each probe run compares all its tensors with the oracle under the unchanged standing rule
(_close_elementwise of tests/test_hstu_gpu.py; the bounds of the FP8 emulations for the FP8 kernels); on the probed tensor -- the
sparse one -- the result must also be exactly 0 wherever the reference is, and a failure names the worst (sequence, row, head, column)
and the number of pairs folded into it.  Every test prints `hstu_probe_use <case> <probe> <tensor> <rows> <ratio>`: the largest
|got / ref - 1| / rel_tolerance on the probed tensor (rows: sequences below / from 1 025 rows apart), an observation, not a threshold."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hstu_probe as hp
from test_hstu_gpu import _close_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHILD = bool(os.environ.get("MI355_HSTU_CHILD"))      # a forward-kernel variant run: the forward probes alone
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _t(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dt)


def _i32(x):
    return None if x is None else torch.from_numpy(np.asarray(x, np.int32)).to(DEV)


def _report(case, probe, tensor, got, ref):
    """the observation the summary of a change quotes per kernel family"""
    offq, offk, _, _ = hp.geometry(case)
    off = offq if tensor in ("out", "dq") else offk
    kind = ("fp8" if case.family == "fp8" else case.dtype) + ("_fwd" if tensor == "out" else "_bwd")
    rel = hp.rel_tolerance(kind)
    for rows, sel in (("short", lambda n: n < 1025), ("long", lambda n: n >= 1025)):
        worst = 0.0
        for b in range(len(off) - 1):
            if sel(case.lengths[b]) and off[b + 1] > off[b]:
                g, r = got[off[b]:off[b + 1]], ref[off[b]:off[b + 1]]
                nz = r != 0
                if nz.any():
                    worst = max(worst, float(np.abs(g[nz] / r[nz] - 1).max()))
        if worst or rows == "short":
            print(f"hstu_probe_use {case.name} {probe} {tensor} {rows} {worst / rel:.4f}")


def _check_probed(case, probe, tensor, got, ref, tol):
    """the probed tensor: exactly 0 (either sign) where the reference is, within the rule elsewhere; the message says which pair"""
    got = got.detach().to(torch.float64).cpu().numpy()
    ref, tol = np.asarray(ref, np.float64), np.asarray(tol, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), f"{case.name} {tensor}: shape {got.shape} or a NaN / Inf"
    _report(case, probe, tensor, got, ref)
    stray = (ref == 0) & (got != 0)
    bad = np.abs(got - ref) > tol
    if not (stray.any() or bad.any()):
        return
    score = np.where(stray, np.inf, np.abs(got - ref) / tol)
    idx = tuple(int(x) for x in np.unravel_index(int(np.argmax(score)), score.shape))
    b, row, h, c = hp.locate(case, tensor, idx)
    count = int(hp.folded(case, probe, tensor)[1][idx])
    side = "query" if tensor in ("out", "dq") else "key"
    raise AssertionError(f"{case.name} {probe} probe, {tensor}: {int(stray.sum())} elements non-zero where the mask leaves nothing, "
                         f"{int(bad.sum())} outside the rule; worst at sequence {b} (length {case.lengths[b]}), {side} row {row}, head {h}, "
                         f"column {c} (the other side's positions p with (p + {h} * (p // {case.d})) % {case.d} == {c}): got {got[idx]:.6g}, "
                         f"reference {ref[idx]:.6g} = {count} visible pairs, tolerance {tol[idx]:.3g}")


def _paged(case, t, dt):
    """(k, v of the call, kv_cache, page_offsets, page_ids, last_page_lens): the keys in front of the 3 candidates of every sequence
    written page by page into a shuffled cache, the call's k / v rows = the last lq keys (new history + candidates)"""
    offq, offk, _, _ = hp.geometry(case)
    P, B = case.page, len(case.lengths)
    cached = [case.lengths[b] - 3 for b in range(B)]
    npg = [-(-n // P) for n in cached]
    rng = np.random.default_rng(case.d)
    perm = rng.permutation(sum(npg) + 2)
    kf, vf = _t(t["k"], dt), _t(t["v"], dt)
    cache = torch.zeros(sum(npg) + 2, 2, P, hp.H, case.d, dtype=dt, device=DEV)
    page_ids, page_off, last, rows = [], [0], [], []
    for b in range(B):
        pages = perm[page_off[-1]:page_off[-1] + npg[b]]
        for j, pg in enumerate(pages):
            n = min(P, cached[b] - j * P)
            cache[pg, 0, :n] = kf[offk[b] + j * P:offk[b] + j * P + n]
            cache[pg, 1, :n] = vf[offk[b] + j * P:offk[b] + j * P + n]
        page_ids += pages.tolist()
        page_off.append(len(page_ids))
        last.append(cached[b] - (npg[b] - 1) * P)
        rows.append(np.arange(offk[b + 1] - (offq[b + 1] - offq[b]), offk[b + 1]))
    rows = torch.from_numpy(np.concatenate(rows)).to(DEV)
    return kf[rows].contiguous(), vf[rows].contiguous(), cache, _i32(page_off), _i32(page_ids), _i32(last)


def _run(case, probe, backward):
    """{'out', 'dq', 'dk', 'dv', 'drab'} of a bf16 / fp16 case through hstu_attn_varlen_func"""
    from hstu import hstu_attn_varlen_func

    t = hp.inputs(case, probe)
    dt = TDT[case.dtype]
    nc, nt = hp.mask_args(case)
    q, k, v = (_t(t[x], dt) for x in ("q", "k", "v"))
    kw = dict(target_group_size=case.grp, window_size=case.window, alpha=t["alpha"])
    if case.family == "paged":
        k, v, cache, po, pi, ll = _paged(case, t, dt)
        kw.update(kv_cache=cache, page_offsets=po, page_ids=pi, last_page_lens=ll)
    rab = None
    if t["rab"] is not None:
        rab = _t(t["rab"], dt).requires_grad_(backward)
        kw.update(rab=rab, has_drab=backward)
    if t["func"] is not None:
        kw.update(func=torch.from_numpy(t["func"]).to(DEV))
    if backward:
        q, k, v = (x.requires_grad_(True) for x in (q, k, v))
    cuq = _i32(t["offq"])
    cuk = cuq if case.lq is None else _i32(t["offk"])
    mq = max(case.lengths if case.lq is None else case.lq)
    with torch.set_grad_enabled(backward):
        out = hstu_attn_varlen_func(q, k, v, cuq, cuk, None, None, mq, max(case.lengths), t["scaling"], _i32(nc), _i32(nt), **kw)
    res = {"out": out.detach()}
    if backward:
        out.backward(_t(t["dout"], dt))
        res.update(dq=q.grad, dk=k.grad, dv=v.grad)
        if rab is not None:
            res["drab"] = rab.grad
    return res


def _check_run(case, probe, got, want):
    bits = hp.BITS[case.dtype]
    for tensor, (ref, mag) in want.items():
        if tensor == "drab":
            assert got["drab"].shape == ref.shape
        probed = tensor in hp.TESTED[probe] or (tensor == "drab" and probe != "pv")    # (drab of the dq / dk probes: the mask itself)
        if probed:   # (first: its message names the pair)
            _check_probed(case, probe, tensor, got[tensor], ref, hp.tolerance(ref, mag, hp.rule_k(tensor), bits))
        _close_elementwise(got[tensor], ref, mag, hp.rule_k(tensor), bits)          # the standing rule, unchanged, on every tensor


def _fp8(case, probe):
    import hstu

    G, E = hp.fp8_suites()
    t = hp.inputs(case, probe)
    mode, dt = case.quant, torch.bfloat16
    q, k, v, dout = (_t(t[x], dt) for x in ("q", "k", "v", "dout"))
    off = _i32(t["offk"])
    nc, nt, g, window = hp.fp8_mask_args(case, DEV)
    N = max(case.lengths)
    want = hp.expected(case, probe)
    out = hstu.hstu_attn_varlen_func(q, k, v, off, off, None, None, N, N, t["scaling"], nc, nt, g, window, t["alpha"], quant_mode=mode)
    emu, bound = G.emulate(hstu.hstu_fp8.quantize_qkv(q, k, v, off, mode), mode, off.cpu(), t["alpha"], t["scaling"],
                           None if nc is None else nc.cpu(), None if nt is None else nt.cpu(), g, window)
    got, refs = {"out": out}, {"out": (emu, bound)}
    kw = hstu.quantize_for_backward(q, k, v, dout, off, mode)
    grads = hstu.varlen_bwd(dq=None, dk=None, dv=None, cu_seqlens_q=off, cu_seqlens_k=off, max_seqlen_q=N, max_seqlen_k=N,
                            scaling_seqlen=t["scaling"], num_contexts=nc, num_targets=nt, target_group_size=g, window_size_left=window[0],
                            window_size_right=window[1], alpha=t["alpha"], quant_mode=mode, **kw)[:3]
    res = E.emulate_bwd(kw, mode, off.cpu(), t["alpha"], t["scaling"], nc, nt, g, window)
    got.update(zip(E.GRADS, grads))
    refs.update(res)
    for tensor in hp.TESTED[probe]:
        e, b = (x.cpu().numpy() for x in refs[tensor])
        # The emulation of the quantised operands is the oracle's tensor times one constant: modes 0 and 2 return the probe values
        # themselves, modes 1 (vt), 3, 4, 5 round amax / 448 to bf16 before use (hstu_fp8.hip), so each of the up to five operands behind
        # an element is off by one factor of at most 1 + 2^-8 -- the same factor on every pair, so the counts stay counts.
        o = want[tensor][0]
        assert ((e == 0) == (o == 0)).all(), f"{case.name} {tensor}: the emulation's mask is not the oracle's"
        np.testing.assert_allclose(e, o, rtol=5 * 2.0 ** -8, atol=0, err_msg=f"{case.name} {tensor}: a quantiser moved a probe value")
        _check_probed(case, probe, tensor, got[tensor], e, b)
    G.assert_within(out, emu, bound, f"{case.name} {probe} out")       # the FP8 suites' own assertions, on all four tensors
    E.assert_within(grads, res, f"{case.name} {probe}")


@pytest.mark.parametrize("name", list(hp.BY_NAME))
def test_probe(name, monkeypatch):
    case = hp.BY_NAME[name]
    if case.family == "fp8":
        for probe in hp.PROBES:
            _fp8(case, probe)
        return
    backward = case.family != "paged" and not CHILD
    for probe in hp.PROBES if backward else ("pv",):
        want = hp.expected(case, probe, backward)
        _check_run(case, probe, _run(case, probe, backward), want)
        if backward and case.d == 256 and case.dtype == "bf16" and case.family in ("varlen", "func"):
            # the backward again without the P / dS exchange: the three recomputing passes (test_backward_exchange_is_bit_identical... )
            import hstu.hstu_attn_interface as hi

            with monkeypatch.context() as mp:
                mp.setattr(hi, "_DS_MAX_BYTES", 0)
                again = _run(case, probe, True)
            print("hstu_probe_use (the recomputing passes:)")
            _check_run(case, probe, again, want)


@pytest.mark.parametrize("variant", ["1", "2", "3", "4", "5"])
def test_forward_kernel_variants_on_the_probes(variant):
    """MI355_HSTU_FWD = 1 .. 5 forces each d = 256 forward kernel onto every shape (test_forward_kernel_variants of tests/test_hstu_gpu.py:
    rows64, rows64_pairs, rows32, rows32_pairs, one_stream); the library reads the hook once, so the d = 256 forward probes of this file
    are re-run in a fresh child process per value."""
    if CHILD:
        pytest.skip("already a variant run")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_probe and d256 and not fp8 and not rab"],
                       env=dict(os.environ, MI355_HSTU_CHILD="1", MI355_HSTU_FWD=variant), capture_output=True, text=True, timeout=900)
    print("\n".join(ln.replace("hstu_probe_use ", f"hstu_probe_use fwd{variant}:") for ln in r.stdout.splitlines() if ln.startswith("hstu_probe_use")))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout, r.stdout[-500:]
