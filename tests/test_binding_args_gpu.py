"""
The table of tests/binding_args.py on the GPU. Every good call that can run (the collectives' peers are made-up
addresses, the diagnostics setters would redirect later launches) is launched once for real and synchronises cleanly.
Then the mutations of test_binding_args_cpu.py run on ``cuda:0`` under ``_C.check_only(True)``, a host tensor being
the other device: each must raise, and nothing may have been launched: every floating-point tensor of the call is
filled with a sentinel first and is bit-identical afterwards (the index tensors keep their in-range contents). No
mutated call is ever made with the switch off.
"""

import pytest
import torch

from tests import binding_args as ba

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


@pytest.fixture
def _C(cuda):
    from src import _C
    yield _C
    _C.check_only(False)
    ba.stamps_off()


@pytest.mark.parametrize("r", [r for r in ba.ROWS if r.gpu], ids=lambda r: r.name)
def test_good_call_launches_and_synchronises(r, _C, cuda):
    args = r.build(cuda)
    ba.invoke(_C, r, args)
    torch.cuda.synchronize()


@pytest.mark.parametrize("r", ba.ROWS, ids=lambda r: r.name)
def test_mutations_raise_and_launch_nothing(r, _C, cuda):
    args = r.build(cuda)
    held = ba.tensors(args)
    for t in held.values():
        if t.is_floating_point():
            t.view(torch.uint8).fill_(SENTINEL)
    before = {k: t.clone() for k, t in held.items()}
    checked = {k: v for k, v in args.items() if isinstance(v, ba.A)}
    _C.check_only(True)
    for name, a in checked.items():
        for mut, detail, t in ba.mutations(a, "cpu"):
            if (r.name, name, mut) in ba.LEAVE_OUT or (mut == "device" and len(checked) == 1):
                continue
            with pytest.raises(RuntimeError):
                ba.invoke(_C, r, args, (name, t))
                pytest.fail(f"{r.name}: {name} {mut} {detail} was accepted")
    ba.invoke(_C, r, args)      # the good call under the switch: checked, not launched
    _C.check_only(False)
    torch.cuda.synchronize()
    for k, t in held.items():
        assert torch.equal(t.view(torch.uint8), before[k].view(torch.uint8)), (r.name, k)
