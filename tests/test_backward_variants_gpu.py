"""bwd_kernel (dynamicemb_extensions.backward_fused) and opt_rows_kernel (the *_update_for_flat_table /
*_for_padded_buffer ops) at small shapes, one case per instantiation of launch_bwd / launch_opt and per row class of
csrc/hot.h, against the element-wise brackets of tests/backward_cases.py (oracle/vec_twin.py's update_bracket, the weight
dtype's rounding on top).  tests/test_backward_variants_cpu.py shows on the same cases that the brackets can be met and
that they reject seeded mistakes.

The table under test is the interior of a larger allocation, one guard row on either side; `row_addr` entries past
`nu_dev` point at the guards, so nothing here needs an access outside the allocation even if a check in the kernel were
missing.  Everything the step does not own -- untouched rows, the pad between a row and its state, the spare elements of
the row-wise state, the guards -- is compared bit for bit."""
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import backward_cases as bc  # noqa: E402
from backward_cases import CASES, OPT_CASES  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
_EB = {"f32": 4, "bf16": 2, "f16": 2}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(_TD[dtype]) if dtype else t).to(DEV)


def _host(t):
    return t.float().cpu().numpy()


def _strided(a, cols, dtype):
    """[rows, stride] on the device, seen through its first `cols` columns (the row stride stays)"""
    return _dev(a, dtype)[:, :cols]


def _run_backward(e, case, inp, table, csr_state):
    """one backward_fused on `table` (the whole allocation, on the device) with the CSR / hot list in csr_state"""
    ptr_t, csr, hot, grads, offsets, doff, addr, nu_dev = csr_state
    combiner = {"sum": 0, "mean": 1, "seq": -1, "doff": 0}[case.mode]
    if case.opt == "store":      # the dense output is the allocation's interior: row u of it belongs to unique row u
        sink = dict(out=table[1:-1])
    else:
        sink = dict(iter_num=case.it, state_offset=case.state_offset, **case.hp)
    e.backward_fused(ptr_t, csr, inp["n"], inp["max_unique"], grads, inp["B"], case.D, combiner, offsets, doff, addr,
                     _TD[case.wdt], bc.KIND[case.opt], round_grad=case.round_grad, nu_dev=nu_dev, hot=hot, **sink)
    torch.cuda.synchronize()


def _report(kind, case, ref, use):
    worst = bc.worst_by_row_class(ref, use)
    print(f"backward_variants_use {kind} {case.klass:26s} {case.opt:16s} w={case.wdt:4s} g={case.gdt:4s} "
          + " ".join(f"{k}={v:.4f}" for k, v in worst.items()) + f"  ({case.name})")


def _assert_inside(case, ref, use, changed, what):
    bad = np.argwhere(use > 1)
    if bad.size:
        i, j = bad[0]
        raise AssertionError(
            f"{case.name} {what}: {len(bad)} elements outside the bracket; first: unique row {int(ref['u'][i])} "
            f"({int(ref['cnt'][i])} occurrences) column {int(j)}: bracket [{ref['lo'][i, j]!r}, {ref['hi'][i, j]!r}] slack "
            f"{ref['slack'][i, j]!r}, use {use[i, j]}; rows {sorted(set(ref['cnt'][bad[:, 0]].tolist()))[:12]} occurrences, "
            f"columns {sorted(set(bad[:, 1].tolist()))[:12]}")
    assert changed == 0, f"{case.name} {what}: {changed} rows the step does not own changed (guards, untouched rows, rows past nu_dev)"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_fused_backward_against_the_bracket(case):
    import dynamicemb_extensions as e
    t0 = time.perf_counter()
    inp = bc.make_inputs(case)
    ref = bc.reference(case, inp)
    eb, V = _EB[case.wdt], case.vdim
    table = _dev(inp["table"], case.wdt).contiguous()
    start = table.clone()
    nu, mu = inp["nu"], inp["max_unique"]
    # row addresses: 0 for a failed insert; past nu_dev the two guard rows in turn
    base = table.data_ptr() + V * eb
    addr = np.where(inp["slots"] >= 0, base + inp["slots"] * V * eb, 0).astype(np.int64)
    guards = np.where(np.arange(mu - nu) % 2 == 0, table.data_ptr(), table.data_ptr() + (inp["cap"] + 1) * V * eb)
    addr = _dev(np.concatenate([addr, guards.astype(np.int64)]))
    nu_dev = torch.tensor([nu], dtype=torch.int64, device=DEV) if case.nu_extra else None
    rev = _dev(inp["rev"])
    offsets = _dev(inp["offsets"]) if inp["offsets"] is not None else None
    doff = _dev(inp["D_offsets"]) if inp["D_offsets"] is not None else None
    grads = _strided(inp["grads"], case.total_D, case.gdt)
    assert grads.stride(0) == case.grad_stride and grads.data_ptr() % 16 == 0
    if case.hot:
        ptr_t, csr, hot = e.group_by_unique(rev, mu, offsets, nu_dev, dim=case.D)
    else:
        (ptr_t, csr), hot = e.group_by_unique(rev, mu, offsets, nu_dev), None
    # the CSR builder orders a row's entries with atomics, so the repeat below runs on the same CSR; the hot list (tickets
    # and accumulators of the multi-chunk rows) is put back to what the builder left
    hot0 = hot.clone() if hot is not None else None
    state = (ptr_t, csr, hot, grads, offsets, doff, addr if case.opt != "store" else None, nu_dev)
    _run_backward(e, case, inp, table, state)
    got = _host(table)
    use, changed = bc.judge(ref, got)
    _report("bwd", case, ref, use)
    _assert_inside(case, ref, use, changed, "backward_fused")
    # a second run from the same starting bytes: bit-identical on every row without atomics (<= 1024 occurrences)
    table.copy_(start)
    if hot is not None:
        hot.copy_(hot0)
    _run_backward(e, case, inp, table, state)
    again = _host(table)
    quiet = ref["rows"][ref["cnt"] <= 1024]
    same = bc.same_bits(again[quiet], got[quiet]).all(axis=1)
    assert same.all(), f"{case.name}: rows of {sorted(set(ref['cnt'][ref['cnt'] <= 1024][~same].tolist()))} occurrences differ between two runs"
    use2, changed2 = bc.judge(ref, again)
    _assert_inside(case, ref, use2, changed2, "backward_fused (second run)")
    print(f"backward_variants_time bwd {case.name} {time.perf_counter() - t0:.2f} s")


_FLAT = {"sgd": "sgd_update_for_flat_table", "adam": "adam_update_for_flat_table", "adagrad": "adagrad_update_for_flat_table",
         "rowwise_adagrad": "rowwise_adagrad_for_flat_table"}
_PADDED = {"sgd": "sgd_update_for_padded_buffer", "adam": "adam_update_for_padded_buffer",
           "adagrad": "adagrad_update_for_padded_buffer", "rowwise_adagrad": "rowwise_adagrad_for_padded_buffer"}


def _opt_args(case):
    hp = case.hp
    return {"sgd": (hp["lr"],), "adam": (hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], case.it),
            "adagrad": (hp["lr"], hp["eps"]), "rowwise_adagrad": (hp["lr"], hp["eps"])}[case.opt]


@pytest.mark.parametrize("case", OPT_CASES, ids=lambda c: c.name)
def test_optimizer_ops_against_the_bracket(case):
    import dynamicemb_extensions as e
    inp = bc.make_opt_inputs(case)
    D, V, eb = case.D, case.vdim, _EB[case.wdt]
    grads = _dev(inp["grads"], case.gdt)
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=DEV)   # noqa: E731
    # flat table: rows by (table pointer, index) inside a larger table
    table = _dev(inp["table"], case.wdt).contiguous()
    tptr = i64(table.data_ptr() + V * eb)
    tid = torch.zeros(bc.OPT_ROWS, dtype=torch.int64, device=DEV)
    a = _opt_args(case)
    # (the positional orders of the reference's bindings: SGD takes its learning rate after the two width arguments)
    tail = (D, case.vector) + a if case.opt == "sgd" else a + (D, case.vector)
    getattr(e, _FLAT[case.opt])(grads, _dev(inp["idx"]), tptr, tid, i64(V), i64(D), *tail, _TD[case.wdt])
    torch.cuda.synchronize()
    ref = bc.opt_reference(case, inp, "flat")
    use, changed = bc.judge(ref, _host(table))
    _report("opt_flat", case, ref, use)
    _assert_inside(case, ref, use, changed, "flat table")
    # padded buffer: rows of a dense buffer, each at its own table's width, the state behind the widest
    buf = _dev(inp["buffer"], case.wdt).contiguous()
    interior = buf[1:-1]
    tids = _dev(inp["table_ids"]) if case.widths else tid
    tdims = i64(*case.widths) if case.widths else i64(D)
    getattr(e, _PADDED[case.opt])(grads, interior, tids, tdims, D, V, case.vector, *a)
    torch.cuda.synchronize()
    ref = bc.opt_reference(case, inp, "padded")
    use, changed = bc.judge(ref, _host(buf))
    _report("opt_padded", case, ref, use)
    _assert_inside(case, ref, use, changed, "padded buffer")
