"""Run a launch sequence eagerly once, capture it on the second call, replay it afterwards."""
import torch


class CapturedPhase:
    """A phase of a train step whose launches have fixed arguments: the first run() calls
    fn() as it is (allocations and lazy setup happen there), the second captures it into a
    hipGraph and replays that, later ones only replay. Whatever a launch argument bakes in
    (a learning rate, a buffer address) changes: reset()."""

    def __init__(self):
        self.graph = None
        self._warm = False

    def run(self, fn, enabled=True):
        if not enabled:
            fn()
        elif self.graph is not None:
            self.graph.replay()
        elif self._warm:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            self.graph = g
            g.replay()
        else:
            fn()
            self._warm = True

    def reset(self):
        self.graph = None
        self._warm = False
