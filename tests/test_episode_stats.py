"""CPU tests of the episode-statistics fold and the packed-buffer layout
(xagents_amd/episode_stats.py): numpy arrays and a stand-in sink, no device."""
import numpy as np
import oracle
import pytest

from xagents_amd.base import BaseAgent
from xagents_amd.episode_stats import StatsLayout, finished_returns, fold_rollout


class Sink:
    """What BaseAgent._record_finished touches."""
    record = BaseAgent._record_finished

    def __init__(self, history_checkpoint=None):
        self.history_checkpoint = history_checkpoint
        self.total_rewards, self.history = [], []
        self.games = self.done_envs = 0

    def update_history(self, episode_reward):
        self.history.append(float(episode_reward))


def test_fold_matches_reference_step_envs(golden):
    """The oracle rollout over the reference's recorded step_envs run (set up as
    test_host.py::test_replay_rollout_env_semantics_match_reference_step_envs): the fold
    gives the reference's total_rewards in order, the last-column rule its
    episode_rewards."""
    g = golden('step_envs.npz')
    n, T = g['s0'].shape[0], g['new_states'].shape[0]
    rng = np.random.default_rng(0)
    theta = (rng.standard_normal(4675) * 0.1).astype(np.float32)
    env = dict(kind=0, state=g['s0'].copy(), done=np.zeros(n, np.float32),
               cursor=np.zeros(n, np.int32), ep_return=np.zeros(n, np.float32),
               rep_obs=g['rep_obs'], rep_state=g['rep_state'], rep_rew=g['rep_rew'],
               rep_done=g['rep_done'])
    out = oracle.mlp_rollout(theta, 2, env, T, uniforms=rng.random((n, T), dtype=np.float32))
    finished, episode_rewards, dones = fold_rollout(out['done'], out['epret'])
    assert len(g['total_rewards']) > 0
    np.testing.assert_array_equal(finished, g['total_rewards'])
    np.testing.assert_array_equal(episode_rewards, g['episode_rewards'])
    assert dones == (g['dones'][-1] != 0).tolist()
    sink = Sink()
    sink.record(finished)
    assert sink.total_rewards == g['total_rewards'].astype(np.float64).tolist()
    assert sink.games == sink.done_envs == len(g['total_rewards'])


def _episodes():
    """3 envs x 4 steps: env 1 finishes at step 1 (return 7); envs 0 and 2 both finish at
    step 2 (returns 3 and 5); env 0 again at step 3 (return 1). Row form [K, n]."""
    done = np.zeros((4, 3), np.float32)
    epret = np.arange(12, dtype=np.float32).reshape(4, 3) + 100  # running returns elsewhere
    for t, i, r in ((1, 1, 7.0), (2, 0, 3.0), (2, 2, 5.0), (3, 0, 1.0)):
        done[t, i], epret[t, i] = 1.0, r
    return done, epret


def test_fold_is_step_major_then_env_minor():
    done, epret = _episodes()
    finished = finished_returns(done, epret)
    assert finished.dtype == np.float32
    assert finished.tolist() == [7.0, 3.0, 5.0, 1.0]


def test_rollout_form_equals_row_form():
    """[N, T+1] / [N, T] (on-policy, column 0 of done carried in and not folded) and
    [K, n] rows (off-policy) of the same episodes give the same sequence."""
    done, epret = _episodes()
    carried = np.ones((3, 1), np.float32)  # a set carried-in flag is not an episode end
    finished, episode_rewards, dones = fold_rollout(
        np.ascontiguousarray(np.hstack([carried, done.T])), np.ascontiguousarray(epret.T))
    assert finished.tolist() == finished_returns(done, epret).tolist() == [7.0, 3.0, 5.0, 1.0]
    # after the last step: env 0 just finished (its return restarts), envs 1 and 2 run on
    assert dones == [True, False, False]
    assert episode_rewards.tolist() == [0.0, epret[3, 1], epret[3, 2]]


def test_single_row_block():
    """A [1, n] block (one env step, DDPG's stage) folds like a row of a larger block."""
    done, epret = _episodes()
    rows = [finished_returns(done[t:t + 1], epret[t:t + 1]).tolist() for t in range(4)]
    assert rows == [[], [7.0], [3.0, 5.0], [1.0]]
    assert sum(rows, []) == finished_returns(done, epret).tolist()


@pytest.mark.parametrize('history', [None, 'history.parquet'])
def test_record_finished_side_effects(history):
    done, epret = _episodes()
    sink = Sink(history)
    sink.record(finished_returns(done[:1], epret[:1]))  # no finished episode: no change
    assert (sink.total_rewards, sink.history, sink.games, sink.done_envs) == ([], [], 0, 0)
    sink.done_envs = 2  # (check_episodes resets done_envs, games keeps counting)
    sink.games = 10
    sink.record(finished_returns(done, epret))
    assert sink.total_rewards == [7.0, 3.0, 5.0, 1.0]
    assert all(type(r) is float for r in sink.total_rewards)
    assert sink.history == ([7.0, 3.0, 5.0, 1.0] if history else [])
    assert (sink.games, sink.done_envs) == (14, 6)


@pytest.mark.parametrize('n_envs, n_steps, words, packed', [(16, 128, 4224, False),
                                                            (256, 128, 65856, True)])
def test_layout(n_envs, n_steps, words, packed):
    """16 x 128: 16 * 129 = 2064 -> 2112, + 2048 -> status word at 4160, 4224 floats in all;
    256 x 128: 33024 + 32768 -> status word at 65792, 65856 floats, the smallest standard
    shape that reaches the packed-copy threshold."""
    lay = StatsLayout.of(n_envs, n_steps)
    assert lay.o_epret % 64 == 0 and lay.o_status % 64 == 0
    assert lay.o_epret >= n_envs * (n_steps + 1)
    assert lay.o_status >= lay.o_epret + n_envs * n_steps
    assert lay.words == lay.o_status + 64 == words
    assert (lay.words >= StatsLayout.PACKED_COPY_MIN) == packed
    buf = np.zeros(lay.words, np.float32)
    done, epret, status = lay.views(buf)
    assert done.shape == (n_envs, n_steps + 1) and epret.shape == (n_envs, n_steps)
    assert status.shape == (1,) and status.dtype == np.int32
    # views of the buffer at the layout's offsets, disjoint, the status word after both
    done[:], epret[:], status[:] = 1.0, 2.0, 3
    assert buf[:lay.o_epret].sum() == done.size
    assert buf[lay.o_epret:lay.o_status].sum() == 2.0 * epret.size
    assert buf[lay.o_status:].view(np.int32).tolist() == [3] + [0] * 63
    # the same views over a host slot that ends after the status word and one more word
    slot = np.zeros(lay.o_status + 2, np.float32)
    assert [v.shape for v in lay.views(slot)] == [done.shape, epret.shape, status.shape]
