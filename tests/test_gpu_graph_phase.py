"""CapturedPhase (xagents_amd/graph_phase.py): eager once, captured on the second call,
replayed afterwards; reset() starts over; disabled stays eager."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _counted(device):
    x = torch.zeros(1, dtype=torch.float32, device=device)
    entered = []

    def fn():
        entered.append(1)
        x.add_(1)

    return x, entered, fn


def test_eager_then_captured_then_replayed(device):
    from xagents_amd.graph_phase import CapturedPhase
    x, entered, fn = _counted(device)
    phase = CapturedPhase()
    assert phase.graph is None
    for _ in range(4):
        phase.run(fn)
    assert x.item() == 4
    assert len(entered) == 2  # one eager call, one capture
    assert phase.graph is not None
    phase.reset()
    assert phase.graph is None
    phase.run(fn)  # eager again
    assert len(entered) == 3 and phase.graph is None
    assert x.item() == 5


def test_disabled_stays_eager(device):
    from xagents_amd.graph_phase import CapturedPhase
    x, entered, fn = _counted(device)
    phase = CapturedPhase()
    for _ in range(4):
        phase.run(fn, enabled=False)
    assert x.item() == 4
    assert len(entered) == 4
    assert phase.graph is None
