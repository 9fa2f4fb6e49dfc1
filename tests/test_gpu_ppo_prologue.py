"""GPU tests of the persistent PPO update's launch prologue (xa_ppo_update): the XCD-local
launch picks its workgroups without an election and decides its hand-off stores from the
in-launch XCD census. The forced write-through fallback, the XCD-local and the spread
launches must agree bit for bit; back-to-back launches and graph replays on one workspace,
the first steps' loss sums and the workgroups that leave at once are pinned too."""
import ctypes

import numpy as np
import pytest
import torch
from test_gpu_ppo_update import A, B1, B2, CLIP_G, EPS, LR, OBS, _rollout_buffers, _theta0

pytestmark = pytest.mark.gpu

AUTO, SPREAD, LOCAL_WT = 0, 1, 3  # XA_PPO_PLACE_*


class Launcher:
    """xa_ppo_update arguments over one set of rollout buffers, parameters and ONE workspace
    (zeroed once): launch() may be called any number of times."""

    def __init__(self, theta0, bufs, mb_size, epochs, placement):
        from xagents_amd import kernels
        from xagents_amd._lib import XaPpoUpdateArgs, XaShuffle
        self.t = [torch.as_tensor(x, device='cuda') for x in bufs]
        obs, act, logp, val, ret = self.t
        B = obs.shape[0]
        self.K = epochs * ((B + mb_size - 1) // mb_size)
        self.G = G = kernels.ppo_update_blocks(OBS, A, mb_size)
        assert G > 0
        self.theta = torch.as_tensor(theta0, device='cuda').clone()
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.step = torch.zeros(1, dtype=torch.int32, device='cuda')
        nbytes = kernels.ppo_update_workspace_bytes(OBS, A, B, mb_size, epochs, G)
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
        self.loss = torch.zeros(self.K, G, 4, dtype=torch.float32, device='cuda')
        self.status = torch.zeros(1, dtype=torch.int32, device='cuda')
        sh = XaShuffle()
        sh.perm, sh.seed, sh.rng_counter = None, 12345, None
        u = XaPpoUpdateArgs()
        u.obs_dim, u.n_actions, u.batch, u.mb_size, u.epochs = OBS, A, B, mb_size, epochs
        u.shuffle = sh
        u.obs, u.actions, u.old_logp = obs.data_ptr(), act.data_ptr(), logp.data_ptr()
        u.old_values, u.returns = val.data_ptr(), ret.data_ptr()
        u.clip_norm, u.entropy_coef, u.value_coef, u.adv_eps = 0.1, 0.01, 0.5, 1e-8
        u.theta, u.adam_m, u.adam_v = self.theta.data_ptr(), self.m.data_ptr(), self.v.data_ptr()
        u.adam_step = self.step.data_ptr()
        u.adam = kernels.adam_struct(LR, B1, B2, EPS, clip_norm=CLIP_G)
        u.workspace, u.workspace_bytes = self.ws.data_ptr(), nbytes
        u.loss_out = self.loss.data_ptr()
        u.status = self.status.data_ptr()
        u.n_blocks = G
        u.placement = placement
        self.u = u

    def is_local(self):
        from xagents_amd import _lib
        return _lib.load().xa_ppo_update_local(ctypes.byref(self.u))

    def launch(self):
        from xagents_amd import kernels
        kernels.ppo_update(self.u)

    def state(self):
        torch.cuda.synchronize()
        return (self.theta.cpu().numpy(), self.m.cpu().numpy(), self.v.cpu().numpy(),
                int(self.step.item()))

    def abort_word(self):
        return int(self.ws[:8].view(torch.int32)[1].item())


# the smallest launches that still have a hop: G = 2 and G = 4 blocks of 16-sample tiles, a
# ragged last minibatch (232 = 3 x 64 + 40: a half-filled tile and a block with none), and
# the headline shape (the fixed-shape instantiation)
SHAPES = [(128, 32, 2), (256, 64, 1), (256, 64, 4), (232, 64, 2), (2048, 512, 4)]
BLOCKS = {32: 2, 64: 4, 512: 32}


@pytest.mark.parametrize('B,mb,E', SHAPES)
def test_local_forced_fallback_and_spread_agree_bit_for_bit(device, B, mb, E):
    """One launch three ways from the same inputs: XCD-local (plain hand-off stores when the
    census finds every block on one XCD), the same launch with the verdict forced to
    write-through, and the spread grid. Theta, m, v and the step count are byte-identical,
    and the launch that timed out nowhere left the abort word alone."""
    bufs = _rollout_buffers(B, seed=B + E)
    theta0 = _theta0(7)
    out = {}
    for place, want_local in ((AUTO, 1), (LOCAL_WT, 1), (SPREAD, 0)):
        r = Launcher(theta0, bufs, mb, E, place)
        assert r.G == BLOCKS[mb]
        assert r.is_local() == want_local, place
        r.launch()
        out[place] = r.state()
        assert int(r.status.item()) == 0 and r.abort_word() == 0, place
        assert out[place][3] == r.K
    assert not np.array_equal(out[AUTO][0], theta0)
    for place in (LOCAL_WT, SPREAD):
        for got, ref in zip(out[place], out[AUTO]):
            np.testing.assert_array_equal(got, ref)


def _agents(monkeypatch, n, use_graph=False):
    """(persistent, ..., chain) PPO agents on the same replay and seed: 16 envs x 16 steps,
    4 epochs x 4 minibatches of 64 (4 blocks of 16-sample tiles)."""
    from test_gpu_agent import make_agent
    monkeypatch.setenv('XA_STATS_IN_UPDATE', '0')
    monkeypatch.setenv('XA_PPO_UPDATE', 'persistent')
    out = [make_agent(n_envs=16, n_steps=16, seed=5, use_graph=use_graph) for _ in range(n)]
    monkeypatch.setenv('XA_PPO_UPDATE', 'chain')
    out.append(make_agent(n_envs=16, n_steps=16, seed=5, use_graph=False))
    assert all(a.update_mode == 'persistent' and a.update_blocks == 4 for a in out[:-1])
    assert out[-1].update_mode == 'chain'
    for a in out:
        a.get_batch()  # the same rollout for every agent (same parameters, same replay)
    torch.cuda.synchronize()
    for a in out[1:]:
        np.testing.assert_array_equal(a.b_act.cpu().numpy(), out[0].b_act.cpu().numpy())
        np.testing.assert_array_equal(a.b_ret.cpu().numpy(), out[0].b_ret.cpu().numpy())
    return out


def _params(a):
    opt = a.model.optimizer
    return a.model.theta, opt.m, opt.v, opt.iterations


def test_back_to_back_launches_and_graph_replays_match_the_chain(device, monkeypatch):
    """Six launches in a row on one workspace with nothing re-zeroed (launch generation and
    tag parity alone keep them apart): each launch's parameter step equals the
    per-minibatch chain's from the same state at the chain test's tolerance (1e-4 of the
    step; the chain is re-seated on the persistent state before every launch, so each
    comparison is that test's). The same six launches as a captured graph of three,
    replayed twice, give the eager result bit for bit."""
    from xagents_amd import _lib
    a, c, b = _agents(monkeypatch, 2)
    assert _lib.load().xa_ppo_update_local(ctypes.byref(a._uargs)) == 1
    for i in range(6):
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
        print(f'launch {i}: persistent vs chain step, relative {rel:.3e}')
        assert rel < 1e-4, i
        assert int(a.model.optimizer.iterations.item()) == 16 * (i + 1)
        assert int(b.model.optimizer.iterations.item()) == 16 * (i + 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(3):
            c._update_impl()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert int(a.device_status.item()) == 0 and int(c.device_status.item()) == 0
    for got, ref in zip(_params(c), _params(a)):
        np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())
    assert int(c.rng_counter.item()) == int(a.rng_counter.item())


def test_first_steps_loss_sums_match_the_chain(device, monkeypatch):
    """The pg / value / entropy sums of optimizer steps 0 and 1 (loss_out) against the
    per-minibatch chain's loss partials, at the teacher-forced test's 1e-5: step 0's loss
    phase must see the minibatch statistics the prologue forms, step 1's the parameters
    after one Adam step."""
    from xagents_amd import kernels
    a, b = _agents(monkeypatch, 1)
    K, G, mb = 16, 4, 64
    loss = torch.zeros(K, G, 4, dtype=torch.float32, device='cuda')
    a._uargs.loss_out = loss.data_ptr()
    a._update_impl()
    kernels.minibatches(b._mbargs)
    ref = []
    for i in (0, 1):
        kernels.ac_grad(b._gargs_list[i])
        ref.append(b.loss_partials.cpu().numpy().astype(np.float64).sum(axis=0))
        b._reduce_gradients(b.partials)
    torch.cuda.synchronize()
    assert int(a.device_status.item()) == 0
    got = loss.cpu().numpy().astype(np.float64).sum(axis=1)
    for i in (0, 1):
        err = (abs(got[i][0] - ref[i][0]) / max(abs(ref[i][0]), mb),
               abs(got[i][1] - ref[i][1]) / abs(ref[i][1]),
               abs(got[i][2] - ref[i][2]) / abs(ref[i][2]))
        print(f'step {i}: pg / value / entropy sums vs the chain, relative {err}')
        assert got[i][3] == ref[i][3] == mb
        assert max(err) < 1e-5, (i, err)
    assert not np.allclose(got[0][:3], got[1][:3], rtol=1e-6)  # two different steps
