"""Tests of phase B of the persistent PPO update's column-form kernels (xa_ppo_update): every
part of a pair column is polled and summed on one wave and combined there lane to lane, the
step's polls share one vote on the block's abort word, and a poll round after the first
reloads only what is missing. None of it may move a bit: the specialised and the general
step-loop copies agree byte for byte at the shapes that reach these kernels, every step's
reduced gradient matches the float64 sum over the minibatch at both slice widths, and the
lane layout is restated on the host for every grid the host's rule admits.

(No test makes a poll time out: the abort path is argued in the kernel's comments.)"""
import numpy as np
import oracle
import pytest

K_BF = 11  # granules per thread of one poll round (kBF)
H = 64     # hidden width of the two dense layers
SHAPES_OA = [(4, 2), (2, 3), (6, 3), (8, 4)]  # the compiled (obs, actions) shapes


def n_params(obs, actions):
    return obs * H + H + H * H + H + H * (actions + 1) + (actions + 1)


def slices(G, P):
    """(c0, nc, parts) of every block's phase-B slice of pair columns (ppo_update_impl.hpp)."""
    NP2 = ((P + 3) & ~3) // 2
    CB = (NP2 + G - 1) // G
    out = []
    for b in range(G):
        c0 = min(NP2, b * CB)
        nc = min(NP2, c0 + CB) - c0
        parts = (min(4, 256 // nc) if nc <= 128 else 1) if nc > 0 else 0
        out.append((c0, nc, parts))
    return out


def col_b_everywhere(G, P):
    """The host's rule for the one-level column-form kernels: every block's slice in the
    column form, with every part of a column on one of the block's four waves."""
    for _, nc, parts in slices(G, P):
        if nc <= 0:
            continue
        if not (parts > 1 and (G + parts - 1) // parts <= K_BF):
            return False
        if nc > 4 * (64 // parts):
            return False
    return True


def test_every_part_of_a_column_sits_on_one_lane_of_one_wave():
    """The kernel's lane layout, restated: wave v owns columns [v cpw, (v + 1) cpw) of the
    slice (cpw = 64 / parts) and lane part * cpw + j holds part `part` of column v cpw + j.
    For every grid the host's rule admits: each (part, column) of each block lands on exactly
    one lane of one of the four waves, no lane index passes 63, the parts of a column share
    the wave, and the kernel's decode of (wave, lane) gives the pair back."""
    assert n_params(4, 2) == 4675
    admitted = 0
    for obs, act in SHAPES_OA:
        P = n_params(obs, act)
        for G in range(19, 33):
            if not col_b_everywhere(G, P):
                continue
            admitted += 1
            for _, nc, parts in slices(G, P):
                if nc <= 0:
                    continue
                cpw = 64 // parts
                assert parts in (2, 3, 4) and cpw == {2: 32, 3: 21, 4: 16}[parts]
                seen = {}
                for part in range(parts):
                    for c in range(nc):
                        wave, lane = c // cpw, part * cpw + c % cpw
                        assert 0 <= wave < 4 and 0 <= lane <= 63, (G, P, part, c)
                        assert (wave, lane) not in seen
                        seen[(wave, lane)] = (part, c)
                        # part 0's lane fetches part q from lane j + q cpw of its own wave
                        assert lane == (c % cpw) + part * cpw
                # the kernel's decode of every (wave, lane) of the block
                for wave in range(4):
                    for lane in range(64):
                        part = (lane >= cpw) + (lane >= 2 * cpw) + (lane >= 3 * cpw)
                        c = wave * cpw + lane - part * cpw
                        active = wave * cpw < nc and part < parts and c < nc
                        assert active == ((wave, lane) in seen)
                        if active:
                            assert seen[(wave, lane)] == (part, c)
                assert len(seen) == parts * nc
    assert admitted > 0
    # the headline grid: 31 slices of 74 columns in 3 parts, the last of 44 in 4
    assert col_b_everywhere(32, 4675)
    assert sorted(set(s[1:] for s in slices(32, 4675))) == [(44, 4), (74, 3)]
    # 85 columns in 3 parts would need a 22nd column on a wave: the rule sends that grid to
    # the generic kernel
    assert (85, 3) in [s[1:] for s in slices(30, n_params(8, 4))]
    assert not col_b_everywhere(30, n_params(8, 4))


# (batch, minibatch, epochs, blocks): the smallest shapes that reach the column-form kernels
# (test_gpu_ppo_loop_forms.py): 20 blocks with slices of 117 / 115 columns in 2 parts and
# blocks without a tile; the headline's grid at a run-time shape; the fixed-shape kernel
# (slices of 74 columns in 3 parts, the last block's 44 in 4)
SHAPES = [(680, 320, 1, 20), (1064, 512, 2, 32), (2048, 512, 4, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize('place', ['auto', 'local_wt', 'spread'])
@pytest.mark.parametrize('B,mb,E,G', SHAPES)
def test_specialised_and_general_copies_agree_byte_for_byte(device, B, mb, E, G, place):
    """The same launch from the same inputs through the specialised copy (no optional output)
    and the general copy (loss_out requested), at each placement: theta, m, v and the step
    count byte-identical, status 0, the abort word untouched."""
    from test_gpu_ppo_prologue import AUTO, LOCAL_WT, SPREAD, Launcher
    from test_gpu_ppo_update import _rollout_buffers, _theta0
    placement = {'auto': AUTO, 'local_wt': LOCAL_WT, 'spread': SPREAD}[place]
    bufs = _rollout_buffers(B, seed=B + E)
    theta0 = _theta0(7)
    assert col_b_everywhere(G, theta0.size)
    out = []
    for want_loss in (False, True):
        r = Launcher(theta0, bufs, mb, E, placement)
        assert r.G == G
        if not want_loss:
            r.u.loss_out = None
        r.launch()
        out.append(r.state())
        assert int(r.status.item()) == 0 and r.abort_word() == 0
        assert out[-1][3] == r.K
    assert not np.array_equal(out[0][0], theta0)
    for got, ref in zip(out[0], out[1]):
        np.testing.assert_array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('B,mb,E,G', [SHAPES[0], SHAPES[2]])
def test_every_steps_reduced_gradient_vs_f64(device, B, mb, E, G):
    """grad_trace (the general copy): every optimizer step's reduced gradient against the
    float64 gradient of the step's minibatch at the device's own theta_k -- the f64 sum of
    the blocks' rows -- at the teacher-forced test's 1e-5. A slice boundary or a part mapped
    to the wrong lane would drop or double rows of some columns."""
    from test_gpu_ppo_update import A, _rel, _rollout_buffers, _theta0, run_update
    bufs = _rollout_buffers(B, seed=B + 17)
    obs, act, logp, val, ret = bufs
    theta0 = _theta0(6)
    out = run_update(theta0, bufs, mb, E, trace=True)
    assert out['status'] == 0 and out['G'] == G and out['step'] == out['K']
    th_tr, g_tr = out['theta_trace'].astype(np.float64), out['grad_trace'].astype(np.float64)
    perms = [oracle.shuffle_perm(B, e, 12345, 0) for e in range(E)]
    n_mb = (B + mb - 1) // mb
    worst = 0.0
    for k in range(out['K']):
        e, mi = divmod(k, n_mb)
        idx = perms[e][mi * mb:(mi + 1) * mb]
        adv = oracle.normalize_advantages(ret[idx], val[idx])
        _, g = oracle.ac_loss_grad_f64(th_tr[k], obs[idx], act[idx], ret[idx], val[idx], A,
                                       'ppo', logp[idx], adv)
        worst = max(worst, _rel(g_tr[k], g))
    print(f'worst relative error of a reduced gradient over {out["K"]} steps: {worst:.3e}')
    assert worst < 1e-5
