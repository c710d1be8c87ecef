"""
The argument checks of csrc/bindings.cpp, on host tensors: with ``_C.check_only(True)`` a binding runs every check and
launches nothing, so a missing check shows up here as a failed assertion, never as a kernel started on a host pointer.

For every row of tests/binding_args.py the good call returns; then each tensor argument in turn is put on another
device, given another dtype, strided, shortened, misaligned and flattened (whatever applies to it, see
binding_args.A) and the call must raise. The table covers every entry point with a tensor parameter, and
bindings.cpp itself takes no tensor's address: that is arg_check.h's.
"""

import os
import re

import pytest
import torch

from tests import binding_args as ba

try:
    from src import _C
except Exception:  # pragma: no cover - depends on build state
    _C = None

pytestmark = pytest.mark.skipif(_C is None, reason="src/_C is not built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.fixture
def check_only():
    _C.check_only(True)
    try:
        yield
    finally:
        _C.check_only(False)
        ba.stamps_off()


def test_table_covers_every_entry_point_with_a_tensor():
    ops = {n for n in dir(_C) if not n.startswith("_")}
    assert ba.TENSOR_FREE <= ops
    assert {r.op for r in ba.ROWS} == ops - ba.TENSOR_FREE
    # the tensor-free list is what it says: none of them has a Tensor in its signature
    for n in ba.TENSOR_FREE:
        assert "Tensor" not in getattr(_C, n).__doc__.split("->")[0], n


def test_bindings_take_no_address_themselves():
    src = open(os.path.join(ROOT, "csrc", "bindings.cpp")).read()
    assert src.count("data_ptr") == 0 and len(re.findall(r"\bbf\(", src)) == 0
    assert '#include "arg_check.h"' in src
    assert "data_ptr" in open(os.path.join(ROOT, "csrc", "arg_check.h")).read()


@pytest.mark.parametrize("r", ba.ROWS, ids=lambda r: r.name)
def test_good_call_returns_and_every_mutation_raises(r, check_only):
    args = r.build(CPU)
    ba.invoke(_C, r, args)
    checked = {k: v for k, v in args.items() if isinstance(v, ba.A)}
    n = 0
    for name, a in checked.items():
        for mut, detail, t in ba.mutations(a, "meta"):
            if (r.name, name, mut) in ba.LEAVE_OUT:
                continue
            if mut == "device" and len(checked) == 1:
                continue    # under check-only the first tensor defines the device: an only tensor has no other
            with pytest.raises(RuntimeError):
                ba.invoke(_C, r, args, (name, t))
                pytest.fail(f"{r.name}: {name} {mut} {detail} ({t.dtype} {tuple(t.shape)} {t.stride()}) was accepted")
            n += 1
    print(f"{r.name}: {n} mutated calls refused")
    ba.invoke(_C, r, args)      # and the good call is still one


def test_leave_out_list_is_short():
    names = {r.name for r in ba.ROWS}
    for (row, arg, mut), why in ba.LEAVE_OUT.items():
        assert row in names and mut in ba.MUTATIONS and mut not in ("device", "short") and why
        assert isinstance(ba.ROWS[[r.name for r in ba.ROWS].index(row)].build(CPU)[arg], ba.A)
    pairs = {(row, mut) for row, _, mut in ba.LEAVE_OUT}
    print(f"{len(pairs)} (row, mutation) pairs left out of {len(ba.ROWS) * len(ba.MUTATIONS)}")
    assert 10 * len(pairs) <= len(ba.ROWS) * len(ba.MUTATIONS)


def test_an_absent_optional_may_live_anywhere(check_only):
    meta = torch.empty(0, device="meta")
    for name, absent in (("silu_and_mul", {"row_scale": meta}), ("rms_row_scale", {"x": meta}),
                         ("attn_prefill", {"cos_sin": meta, "q_scale": meta}), ("attn_decode", {"counters": meta}),
                         ("sample", {k: None for k in ("temperature", "top_k", "top_p", "seeds", "steps", "part", "cnt",
                                                       "lm_part")}),
                         ("logit_process", {"count_ids": None, "lm_part": None}),
                         ("pool_embed", {"acc": None, "part": None, "tickets": None}),
                         ("gemm_decode_grouped", {"rows": meta})):
        r = next(r for r in ba.ROWS if r.name == name)
        args = r.build(CPU)
        args.update(absent)
        ba.invoke(_C, r, args)


def test_without_the_switch_a_host_tensor_is_refused():
    # the setters launch nothing: safe to call with the switch off
    for op in ("gd_set_timestamps", "attn_set_timestamps"):
        with pytest.raises(RuntimeError, match="must be a GPU tensor"):
            getattr(_C, op)(torch.zeros(6, dtype=torch.int64))
