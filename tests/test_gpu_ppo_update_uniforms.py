"""GPU tests of the launch-uniform values in the persistent PPO update's step loop
(xa_ppo_update) at the headline shape: 16 envs x 128 steps, 4 epochs x 4 minibatches of 512
on 32 blocks, the fixed-shape column-form kernel. The loss coefficients, the clip range, the
gradient-norm clip and the Adam constants are the same in every lane and every step; how the
step loop holds them (and the lane predicates around them) is the kernel's business, so each
is moved off its default here, the gradient clip both switched off and made to bind on every
step.

In every case the launch without optional outputs (the step loop's specialised copy) must
equal the launch with loss_out requested (the general copy) byte for byte in theta, m, v and
the step count, and the per-minibatch chain at the chain test's tolerance (1e-4 of the
parameter step), under both XCD-local placements (plain hand-off stores, forced
write-through); no launch may report a poll time-out."""
import ctypes

import numpy as np
import pytest
import torch
from test_gpu_agent import make_agent
from test_gpu_ppo_prologue import AUTO, LOCAL_WT, _params

pytestmark = pytest.mark.gpu

K, G = 16, 32

# agent keywords (loss) and optimizer attributes (Adam) moved off their defaults
CASES = {
    'grad_clip_off': (dict(grad_norm=0.0), {}),
    # five hundred times below the default clip norm, far below a PPO step's gradient norm
    # here (the last test sees that this case lands elsewhere than the default and than 0)
    'grad_clip_binds': (dict(grad_norm=1e-3), {}),
    'loss_coefficients': (dict(entropy_coef=0.05, value_loss_coef=0.25, clip_norm=0.3), {}),
    'adam_constants': ({}, dict(beta_1=0.8, beta_2=0.99, epsilon=1e-5)),
}


def _agent(monkeypatch, mode, kw, opt_kw):
    """A PPO agent on _agents128's seeded replay (test_gpu_ppo_loop_forms.py) with the
    case's loss keywords and Adam constants."""
    monkeypatch.setenv('XA_STATS_IN_UPDATE', '0')
    monkeypatch.setenv('XA_PPO_UPDATE', mode)
    a = make_agent(n_envs=16, n_steps=128, seed=5, use_graph=False, t_rec=512, **kw)
    if opt_kw:
        for name, value in opt_kw.items():
            assert hasattr(a.model.optimizer, name)
            setattr(a.model.optimizer, name, value)
        a._setup_update()  # the update's arguments again, from the optimizer as it is now
    assert a.update_mode == mode
    return a


def _abort_word(a):
    return int(a.update_ws[:8].view(torch.int32)[1].item())


@pytest.mark.parametrize('place', [AUTO, LOCAL_WT], ids=['plain', 'write_through'])
@pytest.mark.parametrize('case', list(CASES))
def test_specialised_general_and_chain_agree(device, monkeypatch, case, place):
    from xagents_amd import _lib
    kw, opt_kw = CASES[case]
    spec, gen = (_agent(monkeypatch, 'persistent', kw, opt_kw) for _ in range(2))
    chain = _agent(monkeypatch, 'chain', kw, opt_kw)
    loss = torch.zeros(K, G, 4, dtype=torch.float32, device='cuda')
    for a in (spec, gen):
        u = a._uargs
        assert a.update_blocks == G and (u.batch, u.mb_size, u.epochs) == (2048, 512, 4)
        u.placement = place
        assert _lib.load().xa_ppo_update_local(ctypes.byref(u)) == 1
        assert not (u.loss_out or u.grad_out or u.theta_trace or u.grad_trace)
        # the case reached the launch arguments
        opt = a.model.optimizer
        want = (a.clip_norm, a.entropy_coef, a.value_loss_coef, a.grad_norm, opt.beta_1,
                opt.beta_2, opt.epsilon)
        got = (u.clip_norm, u.entropy_coef, u.value_coef, u.adam.clip_norm, u.adam.beta1,
               u.adam.beta2, u.adam.eps)
        np.testing.assert_allclose(got, want, rtol=1e-6)
    gen._uargs.loss_out = loss.data_ptr()  # an optional output: the general copy
    agents = (spec, gen, chain)
    for a in agents:
        a.get_batch()  # the same rollout for every agent (same parameters, same replay)
    torch.cuda.synchronize()
    for a in agents[1:]:
        np.testing.assert_array_equal(a.b_act.cpu().numpy(), spec.b_act.cpu().numpy())
        np.testing.assert_array_equal(a.b_ret.cpu().numpy(), spec.b_ret.cpu().numpy())
    theta0 = spec.model.theta.cpu().numpy().astype(np.float64)
    for a in agents:
        a._update_impl()
    torch.cuda.synchronize()
    for a in (spec, gen):
        assert int(a.device_status.item()) == 0 and _abort_word(a) == 0  # no poll time-out
    assert bool(loss.abs().sum().item() > 0)  # the general copy ran and wrote its sums
    for got, ref in zip(_params(spec), _params(gen)):
        np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())
    for a in agents:
        assert int(a.model.optimizer.iterations.item()) == K
    ts = spec.model.theta.cpu().numpy().astype(np.float64)
    tc = chain.model.theta.cpu().numpy().astype(np.float64)
    assert np.isfinite(ts).all() and not np.array_equal(ts, theta0)
    rel = np.linalg.norm(ts - tc) / np.linalg.norm(tc - theta0)
    print(f'{case}: specialised persistent vs chain step, relative {rel:.3e}')
    assert rel < 1e-4


def test_the_cases_differ_from_the_defaults(device, monkeypatch):
    """Each case's update lands somewhere else than the default arguments' (so a value the
    kernel ignored or froze would be seen): theta after one launch, case by case."""
    thetas = []
    for kw, opt_kw in [({}, {})] + list(CASES.values()):
        a = _agent(monkeypatch, 'persistent', kw, opt_kw)
        a.get_batch()
        a._update_impl()
        torch.cuda.synchronize()
        assert int(a.device_status.item()) == 0
        thetas.append(a.model.theta.cpu().numpy())
    for i in range(len(thetas)):
        for j in range(i):
            assert not np.array_equal(thetas[i], thetas[j]), (i, j)
