"""GPU tests of the 16-sample PPO tile's two in-wave hand-offs (ppo_tile.hpp, through
xa_ppo_update): the head partial sums leave each wave by one transposing row sum, every lane
storing one (sample, head) total, and dL/dz reaches the lanes of the MFMA layout lane to lane.
A total stored to the wrong (sample, head) cell, or a dz taken from the wrong lane, changes
the loss sums or rows of the gradient, so every optimizer step's reduced gradient and loss
sums are compared with the float64 restatement at the device's own parameters, at
test_gpu_ppo_update.py's tolerances -- at the smallest grids that run 16-sample tiles, with
3, 4 and 5 heads per sample (12, 16 and 20 totals for a row of 16 lanes), and with a last
tile that holds one valid sample and fifteen padding rows. The specialised and the general
copy of the step loop must then leave the same bits."""
import numpy as np
import oracle
import pytest
import torch
from test_gpu_ppo_phase_b import col_b_everywhere, n_params
from test_gpu_ppo_update import B1, B2, CLIP_G, EPS, LR, _rel

pytestmark = pytest.mark.gpu

# (obs, actions, minibatch): two minibatches per launch (K = 2 optimizer steps).
#  * 33 samples: 3 blocks with one 16-sample tile each (the generic kernel: the general copy
#    of the step loop alone); the third block's tile holds a single valid sample
#  * 305 samples: 20 blocks, the one-level column-form kernel with its specialised copies;
#    the twentieth block's tile holds a single valid sample
CASES = [(4, 2, 33), (4, 2, 305), (6, 3, 33), (6, 3, 305), (8, 4, 33), (8, 4, 305), (2, 3, 33)]


def _buffers(obs_dim, A, B, seed):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((B, obs_dim)).astype(np.float32)
    act = rng.integers(0, A, B).astype(np.int32)
    val = (rng.standard_normal(B) * 0.5).astype(np.float32)
    ret = (val + rng.standard_normal(B)).astype(np.float32)
    logp = np.log(rng.uniform(0.2, 0.8, B)).astype(np.float32)
    return obs, act, logp, val, ret


def _run(obs_dim, A, theta0, bufs, mb, outputs):
    """One xa_ppo_update launch of one epoch; outputs: loss_out, grad_out and the per-step
    traces requested (the general copy of the step loop) or none (the specialised copy,
    where the kernel has one)."""
    from xagents_amd import kernels
    from xagents_amd._lib import XaPpoUpdateArgs, XaShuffle
    obs, act, logp, val, ret = (torch.as_tensor(x, device='cuda') for x in bufs)
    B = obs.shape[0]
    K = (B + mb - 1) // mb
    G = kernels.ppo_update_blocks(obs_dim, A, mb)
    assert G == (mb + 15) // 16  # one 16-sample tile per block
    theta = torch.as_tensor(theta0, device='cuda').clone()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    step = torch.zeros(1, dtype=torch.int32, device='cuda')
    nbytes = kernels.ppo_update_workspace_bytes(obs_dim, A, B, mb, 1, G)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    loss = torch.zeros(K, G, 4, dtype=torch.float32, device='cuda')
    grad = torch.zeros_like(theta)
    th_tr = torch.zeros(K, theta.numel(), dtype=torch.float32, device='cuda')
    g_tr = torch.zeros_like(th_tr)
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    sh = XaShuffle()
    sh.perm, sh.seed, sh.rng_counter = None, 12345, None
    u = XaPpoUpdateArgs()
    u.obs_dim, u.n_actions, u.batch, u.mb_size, u.epochs = obs_dim, A, B, mb, 1
    u.shuffle = sh
    u.obs, u.actions, u.old_logp = obs.data_ptr(), act.data_ptr(), logp.data_ptr()
    u.old_values, u.returns = val.data_ptr(), ret.data_ptr()
    u.clip_norm, u.entropy_coef, u.value_coef, u.adv_eps = 0.1, 0.01, 0.5, 1e-8
    u.theta, u.adam_m, u.adam_v, u.adam_step = (theta.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                step.data_ptr())
    u.adam = kernels.adam_struct(LR, B1, B2, EPS, clip_norm=CLIP_G)
    u.workspace, u.workspace_bytes = ws.data_ptr(), nbytes
    u.loss_out = loss.data_ptr() if outputs else None
    u.grad_out = grad.data_ptr() if outputs else None
    if outputs:
        u.theta_trace, u.grad_trace = th_tr.data_ptr(), g_tr.data_ptr()
    u.status = status.data_ptr()
    u.n_blocks = G
    u.placement = 0
    kernels.ppo_update(u)
    torch.cuda.synchronize()
    return dict(theta=theta.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy(),
                step=int(step.item()), status=int(status.item()), loss=loss.cpu().numpy(),
                theta_trace=th_tr.cpu().numpy(), grad_trace=g_tr.cpu().numpy(), G=G, K=K)


@pytest.mark.parametrize('obs_dim,A,mb', CASES)
def test_head_sums_and_dz_hand_off_vs_f64(device, obs_dim, A, mb):
    B = 2 * mb
    P = n_params(obs_dim, A)
    bufs = _buffers(obs_dim, A, B, seed=B + A)
    obs, act, logp, val, ret = bufs
    theta0 = (np.random.default_rng(obs_dim + 100).standard_normal(P) * 0.2).astype(np.float32)
    out = _run(obs_dim, A, theta0, bufs, mb, outputs=True)
    G, K = out['G'], out['K']
    assert out['status'] == 0 and out['step'] == K == 2
    assert mb % 16 == 1  # the last block's tile: one valid sample, fifteen padding rows
    assert col_b_everywhere(G, P) == (mb == 305)
    np.testing.assert_array_equal(out['theta_trace'][0], theta0)
    perm = oracle.shuffle_perm(B, 0, 12345, 0)
    for k in range(K):
        idx = perm[k * mb:(k + 1) * mb]
        adv = oracle.normalize_advantages(ret[idx], val[idx])
        tm, g = oracle.ac_loss_grad_f64(out['theta_trace'][k].astype(np.float64), obs[idx],
                                        act[idx], ret[idx], val[idx], A, 'ppo', logp[idx], adv)
        rel = _rel(out['grad_trace'][k], g)
        per_block = out['loss'][k].astype(np.float64)
        ls = per_block.sum(axis=0)
        err = (abs(ls[0] - tm['pg_sum']) / max(abs(tm['pg_sum']), mb),
               abs(ls[1] - tm['vl_sum']) / abs(tm['vl_sum']),
               abs(ls[2] - tm['ent_sum']) / abs(tm['ent_sum']))
        print(f'step {k}: reduced gradient rel {rel:.3e}, loss sums pg / value / entropy '
              f'{err[0]:.3e} / {err[1]:.3e} / {err[2]:.3e}')
        # every block one tile: 16 samples each, the last block one
        np.testing.assert_array_equal(per_block[:, 3], [16.0] * (G - 1) + [1.0])
        assert rel < 1e-5
        assert max(err) < 1e-5
    # the launch with no optional output (the specialised copy where the kernel holds one)
    bare = _run(obs_dim, A, theta0, bufs, mb, outputs=False)
    assert bare['status'] == 0 and bare['step'] == K
    assert not np.array_equal(bare['theta'], theta0)
    for key in ('theta', 'm', 'v'):
        np.testing.assert_array_equal(bare[key], out[key])
