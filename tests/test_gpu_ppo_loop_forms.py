"""GPU tests of the persistent PPO update's step-loop forms (xa_ppo_update). The one-level
column-form kernels hold three copies of the step loop: a launch that requests no optional
output runs the copy specialised to its hand-off store mode (write-through or plain), a
launch that requests one (here loss_out) runs the general copy. Both must leave theta, the
Adam moments and the step count bit for bit equal at every placement, and the specialised
copies must match the per-minibatch chain over back-to-back launches and a replayed graph.

Which kernel a launch takes is the host's rule (launch_ts): 16-sample tiles whose every
block reduces its phase-B slice in the column form (col_b_everywhere, restated below) take
the one-level column-form kernels, the only ones with specialised copies; with P = 4675
parameters that needs G >= 19 blocks. Smaller grids take the generic kernel, which holds the
general copy alone."""
import ctypes

import numpy as np
import pytest
import torch
from test_gpu_agent import make_agent
from test_gpu_ppo_prologue import AUTO, LOCAL_WT, SPREAD, Launcher, _params
from test_gpu_ppo_update import _rollout_buffers, _theta0

pytestmark = pytest.mark.gpu

K_BF = 11  # granules per thread of one poll round (kBF)


def col_b_everywhere(G, P):
    """The host's test for the one-level column-form kernels (ppo_update_impl.hpp)."""
    NP2 = ((P + 3) & ~3) // 2
    CB = (NP2 + G - 1) // G
    for b in range(G):
        c0 = min(NP2, b * CB)
        nc = min(NP2, c0 + CB) - c0
        if nc <= 0:
            continue
        parts = min(4, 256 // nc) if nc <= 128 else 1
        if not (parts > 1 and (G + parts - 1) // parts <= K_BF):
            return False
    return True


# (batch, minibatch, epochs, blocks, takes a kernel with specialised copies)
#  * 16 envs x 8 steps: G = 2, the generic kernel (the general copy with and without
#    loss_out: the control)
#  * 680 = 2 x 320 + 40, one epoch: G = 20 (near the smallest column-form grid), K = 3, the
#    column-form kernel with run-time shape and workspace offsets; the last minibatch has 40
#    samples = 3 tiles, the third half filled, so 17 of the 20 blocks own no tile of it
#    (the zero row)
#  * 1064 = 2 x 512 + 40, two epochs: G = 32 like the headline, but K = 6 and a ragged last
#    minibatch, so not the fixed shape: the same kernel at the headline's grid, 29 blocks
#    with a zero row
#  * 16 envs x 128 steps, 4 epochs x 4 minibatches of 512: the fixed-shape kernel
SHAPES = [(128, 32, 2, 2, False), (680, 320, 1, 20, True), (1064, 512, 2, 32, True),
          (2048, 512, 4, 32, True)]
PLACES = [(AUTO, 1), (LOCAL_WT, 1), (SPREAD, 0)]


@pytest.mark.parametrize('place,want_local', PLACES)
@pytest.mark.parametrize('B,mb,E,G,column', SHAPES)
def test_specialised_and_general_loop_agree_bit_for_bit(device, B, mb, E, G, column, place,
                                                        want_local):
    """The same launch twice from the same inputs: without any optional output (the copy
    specialised to the placement's store mode: plain XCD-local, write-through when forced or
    spread) and with loss_out requested (the general copy). Theta, m, v and the step count
    are byte-identical; neither launch timed out."""
    bufs = _rollout_buffers(B, seed=B + E)
    theta0 = _theta0(7)
    assert col_b_everywhere(G, theta0.size) == column
    out = []
    for want_loss in (False, True):
        r = Launcher(theta0, bufs, mb, E, place)
        assert r.G == G and mb <= 512  # (<= 16 tiles of 32: 16-sample tiles)
        assert r.is_local() == want_local
        if not want_loss:
            r.u.loss_out = None
        r.launch()
        out.append(r.state())
        assert int(r.status.item()) == 0 and r.abort_word() == 0
        assert out[-1][3] == r.K
        # the general launch wrote its loss sums, the specialised one touched nothing
        assert bool(r.loss.abs().sum().item() > 0) == want_loss
    assert not np.array_equal(out[0][0], theta0)
    for got, ref in zip(out[0], out[1]):
        np.testing.assert_array_equal(got, ref)


def _agents128(monkeypatch, n):
    """(persistent, ..., chain) PPO agents on the same replay and seed at the headline shape:
    16 envs x 128 steps, 4 epochs x 4 minibatches of 512 on 32 blocks -- the fixed-shape
    column-form kernel, and no optional output: the specialised copies."""
    monkeypatch.setenv('XA_STATS_IN_UPDATE', '0')
    monkeypatch.setenv('XA_PPO_UPDATE', 'persistent')
    out = [make_agent(n_envs=16, n_steps=128, seed=5, use_graph=False, t_rec=512)
           for _ in range(n)]
    monkeypatch.setenv('XA_PPO_UPDATE', 'chain')
    out.append(make_agent(n_envs=16, n_steps=128, seed=5, use_graph=False, t_rec=512))
    assert all(a.update_mode == 'persistent' and a.update_blocks == 32 for a in out[:-1])
    assert out[-1].update_mode == 'chain'
    for a in out[:-1]:
        u = a._uargs
        assert (u.batch, u.mb_size, u.epochs) == (2048, 512, 4)
        assert not (u.loss_out or u.grad_out or u.theta_trace or u.grad_trace)
    for a in out:
        a.get_batch()  # the same rollout for every agent (same parameters, same replay)
    torch.cuda.synchronize()
    for a in out[1:]:
        np.testing.assert_array_equal(a.b_act.cpu().numpy(), out[0].b_act.cpu().numpy())
        np.testing.assert_array_equal(a.b_ret.cpu().numpy(), out[0].b_ret.cpu().numpy())
    return out


def test_specialised_launches_and_graph_replay_match_the_chain(device, monkeypatch):
    """Two launches in a row of the specialised form on one workspace (nothing re-zeroed):
    each parameter step equals the per-minibatch chain's from the same state at the chain
    test's tolerance (1e-4 of the step). The same two launches as one captured graph,
    replayed once, give the eager result bit for bit."""
    from xagents_amd import _lib
    a, c, b = _agents128(monkeypatch, 2)
    assert col_b_everywhere(32, a.model.theta.numel())
    assert _lib.load().xa_ppo_update_local(ctypes.byref(a._uargs)) == 1
    for i in range(2):
        prev = a.model.theta.cpu().numpy().astype(np.float64)
        for dst, src in zip(_params(b), _params(a)):
            dst.copy_(src)
        b.rng_counter.copy_(a.rng_counter)
        a._update_impl()
        b._update_impl()
        torch.cuda.synchronize()
        ta = a.model.theta.cpu().numpy().astype(np.float64)
        tb = b.model.theta.cpu().numpy().astype(np.float64)
        rel = np.linalg.norm(ta - tb) / np.linalg.norm(tb - prev)
        print(f'launch {i}: specialised persistent vs chain step, relative {rel:.3e}')
        assert rel < 1e-4, i
        assert int(a.model.optimizer.iterations.item()) == 16 * (i + 1)
        assert int(b.model.optimizer.iterations.item()) == 16 * (i + 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(2):
            c._update_impl()
    graph.replay()
    torch.cuda.synchronize()
    assert int(a.device_status.item()) == 0 and int(c.device_status.item()) == 0
    for got, ref in zip(_params(c), _params(a)):
        np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())
    assert int(c.rng_counter.item()) == int(a.rng_counter.item())
