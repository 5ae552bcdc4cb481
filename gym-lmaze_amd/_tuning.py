"""Launch-policy tuning shared by LmazeVecEnv and LmazeFovealVecEnv: the explicit autotune() and the online tuner.

Nothing here knows which env it tunes.  The env hands over callables -- run n steps, set a policy, point the step
at another observation buffer -- and the engine times them with HIP event pairs (`events`, replaceable by stand-ins
on a machine without a GPU).  Results never depend on the policy, only the pace of the launches."""
import torch


def event_pair():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def median(v):
    return sorted(v)[len(v) // 2]


def prefer_default(ms, default):
    """The fastest entry of {policy: ms}, except that the library default stays unless another policy beats it by more
    than 1.5 %: with the minimum of two short passes a pair that is fast in a burst and slower sustained could win --
    (4, 1) measured 82.6 us while tuning and 88.6 us over the 300 timed steps that followed, next to 83.4 for the
    default."""
    best = min(ms, key=ms.get)
    if default in ms and ms[best] > 0.985 * ms[default]:
        best = default
    return best


def autotune(run, set_policy, set_obs, obs, candidates, default, trial_policy, steps=24, warm=150, rounds=3,
             placement_trials=0, between=None, events=event_pair):
    """Time `candidates` on real steps; returns ({policy: median ms per step}, chosen policy, placement dict or None).

    run(n) enqueues n steps on the current observation buffer, set_policy(p) selects a launch policy, set_obs(ptr)
    points the steps at another observation buffer.  `warm` untimed launches come first: a cold device (the first
    ~100 launches of a process) ranks the candidates differently from the steady state.

    placement_trials=K (K > 1): K - 1 further buffers like `obs` are allocated and the step is timed on each under
    `trial_policy` (3 untimed, 12 timed launches); the fastest becomes the storage of `obs` -- the SAME tensor object,
    so references the caller holds stay valid; the others are freed.  After the policies are timed, the
    first allocation and the kept one are timed under the chosen policy, and the first under the default: what a
    caller who never tries placements gets (bench.py prints both roofline fractions).

    Then `rounds` interleaved passes over the candidates (1 untimed launch -- the first of a new shape -- then
    `steps` timed); the MEDIAN of a candidate's passes counts, and prefer_default() decides.  `between`: a callable
    that enqueues what runs between two steps in the real loop; each step is then timed on its own with an event
    pair and the per-launch median counts."""
    def timed(n, untimed):
        run(untimed)
        e0, e1 = events()
        e0.record()
        run(n)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    run(int(warm))
    placement = first = None
    if int(placement_trials) > 1:
        bufs = [obs] + [torch.empty_like(obs) for _ in range(int(placement_trials) - 1)]
        set_policy(trial_policy)                 # the policy that tells the placements apart
        ms_of = []
        for b in bufs:
            set_obs(b.data_ptr())
            ms_of.append(timed(12, 3))
        keep = min(range(len(bufs)), key=lambda i: ms_of[i])
        placement = {"trials_ms": [round(m, 5) for m in ms_of], "kept": keep}
        first = obs.view_as(obs) if keep != 0 else None      # keeps the first allocation alive (timed below)
        if keep != 0:
            obs.set_(bufs[keep])
        set_obs(obs.data_ptr())
        del bufs
    timings = {}
    for _round in range(int(rounds)):            # interleaved passes; the median of a candidate's passes counts
        for c in candidates:
            set_policy(c)
            if between is None:
                ms = timed(steps, 1)
            else:
                run(1)
                pairs = []
                for _ in range(steps):
                    between()
                    e0, e1 = events()
                    e0.record()
                    run(1)
                    e1.record()
                    pairs.append((e0, e1))
                pairs[-1][1].synchronize()
                ms = median([a.elapsed_time(b) for a, b in pairs])
            timings.setdefault(c, []).append(ms)
    timings = {c: median(v) for c, v in timings.items()}
    best = prefer_default(timings, default)
    if placement is not None:
        kept = obs.data_ptr()
        first_ptr = first.data_ptr() if first is not None else kept
        set_policy(best)
        for name, ptr in (("kept_ms_tuned", kept), ("first_ms_tuned", first_ptr)):
            set_obs(ptr)
            placement[name] = round(timed(steps, 3), 5)
        set_policy(default)                      # ... and under the library default: what an untuned env runs
        set_obs(first_ptr)
        placement["first_ms_default"] = round(timed(steps, 3), 5)
        set_obs(kept)
    return timings, best, placement


class OnlineTuner:
    """Launch-policy selection on the caller's own steps (LmazeVecEnv, streaming regime).  The best (workgroups
    per CU, chunks per workgroup) pair depends on the device and on what else runs between two steps -- with
    the per-env state still cached, 3 per CU wins; after half a gigabyte of other traffic, 8 per CU does
     -- so instead of guessing, the first launches of a run cycle through the candidates, each
    timed on its own with an event pair (no synchronisation: finished pairs are collected as they complete),
    and once every candidate has `samples` timings the lowest median is kept.  `warm` launches are ignored first
    (a cold device ranks differently).  Results never depend on the policy, only the pace of those launches."""

    def __init__(self, candidates, warm=100, samples=12):
        self.candidates = [tuple(c) for c in candidates]
        self.warm, self.samples = int(warm), int(samples)
        self.timings = {c: [] for c in self.candidates}
        self._pending, self._count = [], 0

    def next_candidate(self):
        return self.candidates[self._count % len(self.candidates)]

    def time(self, cand, launch, *args):
        """launch(*args) under an event pair; returns what add() returns."""
        e0, e1 = event_pair()
        e0.record()
        launch(*args)
        e1.record()
        return self.add(cand, e0, e1)

    def add(self, cand, e0, e1):
        """Register one timed launch; returns the winner once every candidate has enough samples."""
        self._count += 1
        if self._count > self.warm:
            self._pending.append((cand, e0, e1))
        while self._pending and self._pending[0][2].query():
            c, a, b = self._pending.pop(0)
            self.timings[c].append(a.elapsed_time(b))
        if all(len(v) >= self.samples for v in self.timings.values()):
            return prefer_default({c: median(v) for c, v in self.timings.items()}, (0, 0))
        return None
