"""Episode statistics, from the device into BaseAgent._record_finished without stalling it: one
fold, one packed layout, one object per on-policy agent (three transports), one per off-policy."""
import ctypes
import os
from collections import namedtuple

import numpy as np
import torch


def finished_returns(done, epret):
    """done[K, n], epret[K, n] (K steps, n envs) -> the returns of the episodes that ended,
    steps outer and envs inner as BaseAgent.step_envs meets them (xagents/base.py:388-426)."""
    return epret[np.nonzero(done)]


def fold_rollout(done, epret):
    """done[N, T+1] (column 0 carried in), epret[N, T] -> (finished, running returns, dones)."""
    d = done[:, 1:]
    return (finished_returns(d.T, epret.T), epret[:, -1] * (1.0 - d[:, -1]),
            (d[:, -1] != 0).tolist())


class StatsLayout(namedtuple('StatsLayout', 'n_envs n_steps o_epret o_status words')):
    """done [N, T+1], epret [N, T] and the status word in one f32 buffer of `words` floats, each
    on a 64-float (256-B) boundary, the status word last: they leave the device in one copy."""
    PACKED_COPY_MIN = 65536  # floats from which the copy / side transports send the pack whole

    @classmethod
    def of(cls, n_envs, n_steps):
        al = lambda x: (x + 63) // 64 * 64  # noqa: E731
        o_epret = al(n_envs * (n_steps + 1))
        o_status = o_epret + al(n_envs * n_steps)
        return cls(n_envs, n_steps, o_epret, o_status, o_status + 64)

    def views(self, buf):
        N, T = self.n_envs, self.n_steps
        return (buf[:N * (T + 1)].reshape(N, T + 1),
                buf[self.o_epret:self.o_epret + N * T].reshape(N, T),
                buf[self.o_status:self.o_status + 1].view(
                    torch.int32 if isinstance(buf, torch.Tensor) else np.int32))


class _OneInFlight:
    """push(item) folds the item pushed before: one rollout (group, block) stays in flight."""
    in_flight = None

    def push(self, item):
        prev, self.in_flight = self.in_flight, item
        if prev is not None:
            self.fold(*prev)

    close = staticmethod(lambda: None)  # (whatever is still open goes in flight)

    def drain(self):
        self.close()
        self.push(None)


class _Copy(_OneInFlight):
    """`copy`: one xa_copy_to_host launch per rollout on the launch stream into one of two mapped
    host slots, each with a reused event: the pack whole from PACKED_COPY_MIN floats (C2 0.419
    -> 0.401 ms per step), else done, epret, status as segments (16 envs 0.2859 -> 0.2814 ms).
    `side` (XA_STATS_SIDE_STREAM=1): the copy on a side stream behind the rollout's event, over
    the update (the pack whole as a D2H DMA copy); the next rollout waits for `guard`."""

    def __init__(self, st, side=False):
        self.st = st
        pin = lambda t: torch.zeros(t.shape, dtype=t.dtype).pin_memory()  # noqa: E731
        self.packed = st.pack is not None and st.pack.numel() >= StatsLayout.PACKED_COPY_MIN
        if self.packed:
            self.host = [pin(st.pack) for _ in range(2)]
            self.views = [st.layout.views(h) for h in self.host]
        else:
            self.views = [(pin(st.done), pin(st.epret), pin(torch.zeros(1, dtype=torch.int32)))
                          for _ in range(2)]
        self.arrays = [tuple(v.numpy() for v in hv) for hv in self.views]
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        self.args = {}  # launch arguments per (slot, segment count)
        self.slot = 0
        self.stream = torch.cuda.Stream(device=st.done.device) if side else None
        self.guard, self.warm = None, not self.packed

    def launch(self, slot):
        from xagents_amd._lib import XaHostCopyArgs, call, mapped_address, stream
        st, h = self.st, self.views[slot]
        segs = [(st.pack, self.host[slot])] if self.packed else \
            [(st.done, h[0]), (st.epret, h[1]), (st.agent.device_status, h[2])]
        if segs[-1][0] is None:
            segs.pop()
        a = self.args.get((slot, len(segs)))
        if a is None:
            a = self.args[slot, len(segs)] = XaHostCopyArgs()
            a.n_segments = len(segs)
            for i, (d, h) in enumerate(segs):
                assert d.is_contiguous() and h.is_contiguous() and h.is_pinned()
                a.src[i], a.dst[i] = d.data_ptr(), mapped_address(h)
                a.bytes[i] = d.numel() * d.element_size()
        call('xa_copy_to_host', ctypes.byref(a), stream())

    def queue(self, after, group_end):
        slot, pack = self.slot, self.st.pack
        if self.stream is None:
            self.launch(slot)
            self.events[slot].record()
        else:
            self.stream.wait_event(after)
            with torch.cuda.stream(self.stream):
                if not self.warm:
                    # a side stream's first D2H copies block the host ~7 ms each: pay them once
                    for h in self.host * 4:
                        h.copy_(pack, non_blocking=True)
                    self.stream.synchronize()
                    self.warm = True
                if self.packed:
                    self.host[slot].copy_(pack, non_blocking=True)
                else:
                    self.launch(slot)
                self.guard = self.events[slot]
                self.guard.record()
        self.slot ^= 1
        self.push((slot,))

    def fold(self, slot):
        self.events[slot].synchronize()
        self.st.fold(*self.arrays[slot])


class _Fused(_OneInFlight):
    """`fused`: the persistent update stores the pack, then its launch number, into the mapped
    slot launch number % XA_PPO_STATS_SLOTS: no statistics launch. Steps are folded in groups
    behind one of four reused events (`group_end` closes one; XA_STATS_EVERY), at most
    FUSED_GROUP_MAX = half the slots each, so a slot is folded before a launch reuses it."""

    def __init__(self, st):
        from xagents_amd._lib import XA_PPO_STATS_SLOTS, mapped_pinned
        self.st = st
        self.words = nw = st.layout.o_status + 1  # through the status word
        self.host, self.dev = zip(*(mapped_pinned(nw + 1, torch.float32)
                                    for _ in range(XA_PPO_STATS_SLOTS)))
        self.arrays = [tuple(v.numpy() for v in st.layout.views(h)) for h in self.host]
        self.gen = [h[nw:].view(torch.int32).numpy() for h in self.host]
        self.events = [torch.cuda.Event() for _ in range(4)]
        self.ev_i = 0
        self.pending = []

    def queue(self, after, group_end):
        agent = self.st.agent
        self.pending.append(agent._upd_launches - 1)
        every = min(int(os.environ.get('XA_STATS_EVERY', '1')), agent.FUSED_GROUP_MAX)
        if group_end and len(self.pending) >= every or \
                len(self.pending) >= agent.FUSED_GROUP_MAX:
            self.close()

    def close(self):
        if self.pending:  # one event behind them: their slots are complete once it is
            ev = self.events[self.ev_i % len(self.events)]
            self.ev_i += 1
            ev.record()
            gens, self.pending = self.pending, []
            self.push((ev, gens))

    def fold(self, ev, gens):
        ev.synchronize()
        for gen in gens:
            slot = gen % len(self.gen)
            got = int(self.gen[slot][0])
            if got != gen:  # an uncounted launch, or one that aborted before its store
                self.st.check_status()
                raise RuntimeError(f'{type(self.st.agent).__name__}: episode statistics slot '
                                   f'{slot} holds update launch {got}, expected {gen}')
            self.st.fold(*self.arrays[slot])


class EpisodeStats:
    """An agent's on-policy statistics, built with the buffers: the given done / epret, or
    (layout) a pack it allocates. queue() picks `side` behind an `after` event, `fused` while
    the update stores them (setup_fused), else `copy`; switching drains the old transport."""

    def __init__(self, agent, done=None, epret=None, layout=None):
        self.agent, self.layout = agent, layout
        self.pack = self.status = None
        if layout is not None:
            self.pack = torch.zeros(layout.words, dtype=torch.float32, device=agent.device)
            done, epret, self.status = layout.views(self.pack)
        self.done, self.epret = done, epret
        self.copy = self.side = self.fused = self.active = None
        self.fused_on = False

    def setup_fused(self, u):
        # the update's statistics arguments; off with XA_STATS_IN_UPDATE=0 or the side stream
        u.stats_words = 0
        self.fused_on = os.environ.get('XA_STATS_IN_UPDATE', '1') != '0' and \
            not self.agent.stats_side_stream
        if self.fused_on:
            f = self.fused = self.fused or _Fused(self)
            u.stats_src, u.stats_words = self.pack.data_ptr(), f.words
            for i, dp in enumerate(f.dev):
                u.stats_dst[i] = dp

    def queue(self, after=None, group_end=True):
        if after is not None:
            t = self.side = self.side or _Copy(self, side=True)
        elif self.fused_on:
            t = self.fused
        else:
            t = self.copy = self.copy or _Copy(self)
        if t is not self.active:
            self.drain()
            self.active = t
        t.queue(after, group_end)

    def sync_copy(self):
        side = self.side  # before a rollout: wait for a copy still reading its buffers
        if side is not None and side.guard is not None:
            torch.cuda.current_stream().wait_event(side.guard)
            side.guard = None

    def fold(self, done, epret, status):
        agent = self.agent
        self.check_status(status[0])
        finished, agent.episode_rewards, agent.dones = fold_rollout(done, epret)
        agent._record_finished(finished)

    def drain(self):
        if self.active is not None:
            self.active.drain()
        if self.side is not None or self.fused_on:
            self.check_status()

    def check_status(self, word=None):
        status = self.agent.device_status  # (word: a host copy; None: read the device's)
        if status is not None and int(status.max().item() if word is None else word):
            raise RuntimeError(
                f'{type(self.agent).__name__}: an in-launch exchange of the persistent update '
                f'timed out (device status word set); the parameters are invalid')


class StepStats(_OneInFlight):
    """The off-policy env steps: a device block of `rows` x [done row | return row] (one launch
    fills a step's two), sent to the host every `rows` steps behind _device_checks()."""

    def __init__(self, agent, rows):
        self.agent, self.rows, n = agent, rows, agent.n_envs
        self.block = torch.zeros(rows, 2, n, dtype=torch.float32, device=agent.device)
        p = self.block.data_ptr()  # each row's (done, return) device addresses
        self.ptrs = [(p + 8 * n * r, p + 8 * n * r + 4 * n) for r in range(rows)]
        self.row = 0

    def advance(self):
        self.row += 1
        if self.row == self.rows:
            self.close()

    def close(self):
        self.agent._device_checks()
        if self.row:
            h = torch.empty(self.row, 2, self.agent.n_envs).pin_memory()
            h.copy_(self.block[:self.row], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.row = 0
            self.push((h.numpy(), ev))

    def fold(self, rows, ev=None):
        """[K, 2, n] host rows into the agent (f64: off-policy histories hold Python floats)."""
        if ev is not None:
            ev.synchronize()
        self.agent._record_finished(finished_returns(rows[:, 0], rows[:, 1]).astype(np.float64))
