"""CPU: the host logic of launch-policy tuning (gym-lmaze_amd/_tuning.py: the online tuner and the autotune engine both
env classes drive), with stand-in events and steps -- no GPU.  Importing the package loads liblmaze_hip.so
(cross-compiled here), which needs no device."""
import contextlib
import importlib

import pytest
import torch

PKG = importlib.import_module("gym-lmaze_amd")
tuning = importlib.import_module("gym-lmaze_amd._tuning")
base = importlib.import_module("gym-lmaze_amd._base")


class FakeEvent:
    """An event pair 'completes' only once the test says so; elapsed_time returns what the test planted."""

    def __init__(self, ms=None):
        self.ms, self.done = ms, False

    def query(self):
        return self.done

    def elapsed_time(self, other):
        return other.ms


def test_round_robin_warm_up_and_lowest_median_wins():
    cands = ((3, 1), (3, 2), (8, 1))
    cost = {(3, 1): 0.090, (3, 2): 0.083, (8, 1): 0.100}
    t = tuning.OnlineTuner(cands, warm=5, samples=3)
    pending, best, seen = [], None, []
    for i in range(200):
        c = t.next_candidate()
        seen.append(c)
        e0, e1 = FakeEvent(), FakeEvent(cost[c] * (3.0 if i % 7 == 0 else 1.0))   # an outlier now and then
        pending.append(e1)
        if len(pending) > 4:                 # the device runs a few launches behind the host
            pending.pop(0).done = True
        best = t.add(c, e0, e1)
        if best is not None:
            break
    assert seen[:6] == [cands[0], cands[1], cands[2]] * 2           # strict round robin
    assert best == (3, 2)                                            # medians shrug the outliers off
    assert all(len(v) >= 3 for v in t.timings.values())
    assert i >= 5 + 3 * len(cands) - 1                               # never before every candidate has its samples


def test_nothing_is_decided_while_the_device_lags():
    t = tuning.OnlineTuner(((3, 1), (8, 1)), warm=0, samples=2)
    evs = []
    for i in range(50):                      # no event ever completes
        c = t.next_candidate()
        e0, e1 = FakeEvent(), FakeEvent(0.1)
        evs.append(e1)
        assert t.add(c, e0, e1) is None
    for e in evs:
        e.done = True
    c = t.next_candidate()
    assert t.add(c, FakeEvent(), FakeEvent(0.1)) in ((3, 1), (8, 1))


def test_launch_hint_encoding():
    V = PKG.LmazeVecEnv
    assert V.launch_hint_of(3, 2) == 0x23 and V.launch_hint_of(8) == 0x18 and V.launch_hint_of(0, 0) == 0
    # (0, 0) = launch_hint 0, the library's per-shape default: always a candidate, and the one kept unless beaten by 1.5 %
    assert V.CANDIDATES[0] == V.DEFAULT_POLICY == (0, 0) and (3, 1) in V.CANDIDATES and (3, 2) in V.CANDIDATES
    assert all(1 <= c[0] <= 8 and 1 <= c[1] <= 15 and (len(c) == 2 or c[2] in (1, 2, 3)) for c in V.CANDIDATES[1:])
    assert V.launch_hint_of(8, 1, 2) == 0x818 and V.launch_hint_of(4, 1, 1) == 0x414


class Clock:
    """Stand-in for the device: every launch appends its cost (ms); an event pair measures the launches enqueued
    between its two records."""

    def __init__(self):
        self.costs = []

    def pair(self):
        return Mark(self), Mark(self)


class Mark:
    def __init__(self, clock):
        self.clock, self.at = clock, None

    def record(self):
        self.at = len(self.clock.costs)

    def synchronize(self):
        pass

    def elapsed_time(self, other):
        return sum(self.clock.costs[self.at:other.at])


class FakeEnv(base.VecEnvBase):
    """What VecEnvBase._tune needs of an env, on the CPU: each step logs (action row, policy, observation buffer k,
    numbered in order of first use), costs cost(policy, k) ms and changes state, epoch and observations, so that the
    test sees whether they come back."""

    def __init__(self, cost, rows=5):
        self.num_envs, self.device, self._epoch, self._captured = 4, torch.device("cpu"), 7, 0
        self.placement, self.tuned_policy, self._expanded = None, None, "stale"
        self._state = torch.arange(32, dtype=torch.uint8)
        self._persistent = [self._state]
        self.obs = torch.arange(12, dtype=torch.float32).reshape(4, 3)
        self.policy, self.buf = "initial", self.obs.data_ptr()
        self.cost, self.rows = cost, rows
        self.clock, self.log, self.seen = Clock(), [], []

    def _guard(self):
        return contextlib.nullcontext()

    def _set_policy(self, policy):
        self.policy = policy

    def _set_obs(self, ptr):
        self.buf = ptr

    def step_row(self, r):
        if self.buf not in self.seen:
            self.seen.append(self.buf)
        k = self.seen.index(self.buf)
        self.log.append((r, self.policy, k))
        self.clock.costs.append(self.cost(self.policy, k))
        self._state.add_(1)
        self._epoch += 1
        self.obs.add_(1)

    def tune(self, **kw):
        return self._tune(self.rows, self.step_row, [self.obs], events=self.clock.pair, **kw)


def test_autotune_engine_launch_sequence_and_restore():
    D, A, B, TRIAL = (0, 0), (3, 1), (8, 2), (5, 2)
    ms, factor = {D: 0.100, A: 0.097, B: 0.120, TRIAL: 0.200}, (1.10, 1.05, 1.00)     # the third buffer is fastest
    env = FakeEnv(lambda p, k: ms.get(p, 1.0) * factor[k])
    state, obs, warm, steps, rounds = env._state.clone(), env.obs.clone(), 4, 6, 2
    t = env.tune(candidates=[D, A, B], default=D, trial_policy=TRIAL, steps=steps, warm=warm, rounds=rounds,
                 placement_trials=3)
    want = [("initial", 0)] * warm                                       # untimed warm-up, first buffer
    for k in range(3):                                                   # per buffer: 3 untimed + 12 timed, trial policy
        want += [(TRIAL, k)] * 15
    for _ in range(rounds):                                              # per round and candidate: 1 untimed + steps timed
        for c in (D, A, B):
            want += [(c, 2)] * (1 + steps)
    want += [(A, 2)] * (3 + steps) + [(A, 0)] * (3 + steps) + [(D, 0)] * (3 + steps)   # kept / first tuned, first default
    assert [(p, k) for _, p, k in env.log] == want
    assert [r for r, _, _ in env.log] == [i % env.rows for i in range(len(want))]        # action rows cycled in order
    assert t == pytest.approx({D: 0.100, A: 0.097, B: 0.120})
    assert env.tuned_policy == A and env.policy == A                     # 3 % ahead of the default: chosen
    assert env.placement["kept"] == 2 and env.placement["trials_ms"] == [0.22, 0.21, 0.2]
    assert (env.placement["kept_ms_tuned"], env.placement["first_ms_tuned"], env.placement["first_ms_default"]) == (
        0.097, round(0.097 * 1.1, 5), 0.11)
    assert env.buf == env.obs.data_ptr() == env.seen[2] and env._expanded is None     # obs re-homed, same tensor
    assert (env._state == state).all() and env._epoch == 7 and (env.obs == obs).all()  # state, epoch, frame restored


def test_autotune_engine_keeps_the_default_within_1_5_percent_and_times_each_launch_with_between():
    D, A = (0, 0), (3, 1)
    env = FakeEnv(lambda p, k: {D: 0.100, A: 0.099}.get(p, 1.0))
    t = env.tune(candidates=[A, D], default=D, trial_policy=None, steps=5, warm=2, rounds=3)
    assert env.tuned_policy == D and env.policy == D and min(t, key=t.get) == A     # 1 % ahead is not enough
    assert len(env.log) == 2 + 3 * 2 * 6 and env.placement is None
    assert tuning.prefer_default({D: 1.0, A: 0.984}, D) == A and tuning.prefer_default({D: 1.0, A: 0.986}, D) == D
    assert tuning.prefer_default({A: 1.0, (8, 1): 0.5}, D) == (8, 1)    # no default among the candidates

    spikes = iter([0.5, 0.1, 0.1, 0.1, 0.5] * 100)                     # an outlier now and then: the median shrugs it off
    env, between = FakeEnv(lambda p, k: next(spikes) * (0.9 if p == A else 1.0)), []
    t = env.tune(candidates=[D, A], default=D, trial_policy=None, steps=5, warm=1, rounds=1,
                 between=lambda: between.append(len(env.log)))
    assert between == [2 + i for i in range(5)] + [8 + i for i in range(5)]   # before each timed launch, not the untimed one
    assert t == pytest.approx({D: 0.1, A: 0.09}) and env.tuned_policy == A


def test_autotune_refuses_to_move_a_captured_observation_buffer():
    env = FakeEnv(lambda p, k: 1.0)
    env._captured = 1
    with pytest.raises(RuntimeError):
        env.tune(candidates=[(0, 0)], default=(0, 0), trial_policy=(5, 2), placement_trials=2)
    assert env.log == [] and env.tuned_policy is None
