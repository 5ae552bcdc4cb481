"""Loaded state and near-empty mazes: the case table of test_gpu_loaded_state.py, its generators, and its reference.

Two kinds of input the v0/v3 grid kernels carry explicit code for: state no reset produced (set_state() takes any int32
coordinates; the kernels clamp, include/lmaze.h "Loaded state") and mazes with 0, 1 or 2 spawn cells (the placement
rule's "leave unchanged" results, in every one of its implementations).

The reference does not restate the transition: on a layout with a full 'W' border the contract equals the UNMODIFIED C
oracle run on the maze padded with one more ring of 'W', (G+2) x (G+2) -- balls enter as clip(ball, 0, G-1) + 1, goals as
goal + 1, planes are cropped [1:-1, 1:-1], coordinates come back minus 1.  Resets agree under padding (the old border is
'W': the accepted cells and their row-major ranking are unchanged); a reset takes the ball as it is, so a reset that
places nothing hands back whatever the env had.  The oracle refuses G > 64: at G = 63 and 64 it runs unpadded and the
loaded balls stay on rows and columns 1..G-2 (any cell type there; goals anywhere).

The action decode and the cell lookups in Reference._cover_* are coverage bookkeeping only -- they count which envs met
which situation, for test_loaded_state_cpu.py -- and feed no expected value."""
import zlib
from collections import OrderedDict

import numpy as np

import launch_matrix as M
import oracle_lib as O
from closed_loop_ref import explore_draw, sample_action

Row = M.Row
hint = M.hint
kernel_key = M.kernel_key
PER_ENV = M.PER_ENV
SEED, ENV_BASE, STEP_LIMIT = 21, 4099, 12
T_STEPS, K_REC = 6, 3
EPSILON = 0.25
W, B, S, X = (ord(c) for c in "WBSX")

# entry points
RESET, RESET_MASKED = "reset", "reset_masked"
STEP, STEP_RESET = M.STEP, M.STEP_RESET
STEP_U8, STEP_U8_RESET = "step_u8", "step_u8_reset"
OBSERVE, OBSERVE_U8, OBSERVE_U8_MASKED = "observe", "observe_u8", "observe_u8_masked"
ROLLOUT, ROLLOUT_OBS, ROLLOUT_U8, ROLLOUT_OBS_U8 = M.ROLLOUT, M.ROLLOUT_OBS, M.ROLLOUT_U8, M.ROLLOUT_OBS_U8
POLICY_BALL, POLICY_GOAL, SAMPLE_BALL, SAMPLE_GOAL = "policy_ball", "policy_goal", "sample_ball", "sample_goal"
RESETS_ONLY = (RESET, RESET_MASKED)
OBSERVES = (OBSERVE, OBSERVE_U8, OBSERVE_U8_MASKED)
STEPS = (STEP, STEP_RESET, STEP_U8, STEP_U8_RESET)
ROLLOUTS = (ROLLOUT, ROLLOUT_OBS, ROLLOUT_U8, ROLLOUT_OBS_U8)
CLOSED = (POLICY_BALL, POLICY_GOAL, SAMPLE_BALL, SAMPLE_GOAL)
U8 = (STEP_U8, STEP_U8_RESET, OBSERVE_U8, OBSERVE_U8_MASKED, ROLLOUT_U8, ROLLOUT_OBS_U8)
FIRES_RESETS = RESETS_ONLY + (STEP_RESET, STEP_U8_RESET) + ROLLOUTS + CLOSED
TAKES_STEPS = STEPS + ROLLOUTS + CLOSED

# the v0 reward patterns a sticky 'S' target hands back: -0.0, a denormal, +inf, a quiet and a signalling NaN ...
SPECIAL_REWARDS = (0x80000000, 0x00000001, 0x7F800000, 0x7FC00001, 0x7F800001)
# ... and the three reward constants
REWARD_BITS = np.array(SPECIAL_REWARDS + tuple(int(np.float32(r).view(np.uint32)) for r in (-1.0, -0.01, 100.0)), np.uint32)
N_FIXED = 8


def shared(maze):
    """the layout field of a shared-layout row: one of the N_FIXED fixed mazes"""
    return "%s%d" % (M.SHARED, maze)


def maze_of(layout):
    return None if layout == PER_ENV else int(layout[len(M.SHARED):])


def interior_only(G):
    """the oracle cannot take the padded maze: it runs unpadded, on balls that need no clamp"""
    return G + 2 > 64


# ---------------------------------------------------------------- mazes
def _force_goal_marker(lay, used):
    """v0 wants an 'X' (layouts.validate): on the first interior wall cell from the middle on, row-major; where the
    interior has no wall cell left, on the last cell of `used`"""
    G = lay.shape[0]
    if (lay == X).any():
        return
    cells = [(x, y) for x in range(1, G - 1) for y in range(1, G - 1)]
    mid = len(cells) // 2
    for x, y in cells[mid:] + cells[:mid]:
        if lay[x, y] == W:
            lay[x, y] = X
            return
    lay[used[-1]] = X


def fixed_maze(k, G, variant, seed=0):
    """uint8[G,G], the k-th fixed maze (k = 0..7): interior all wall; only the first interior cell; only the last; first
    and last; only an 'X'; one free cell in each 64-cell stretch of the row-major order (the last interior cell of the
    stretch: the top bit of every ballot that has one); two adjacent cells at the end of the last interior row; an
    ordinary p_wall = 0.2 maze.  'S' cells among them, for v0's sticky pairs; v0 gets an 'X' where none is."""
    lay = np.full((G, G), W, np.uint8)
    first, last = (1, 1), (G - 2, G - 2)
    used = []

    def put(cell, c):
        lay[cell] = c
        used.append(cell)
    if k == 1:
        put(first, S)
    elif k == 2:
        put(last, S)
    elif k == 3:
        put(first, B)
        put(last, S)
    elif k == 4:
        put((max(1, (G - 1) // 2),) * 2, X)
    elif k == 5:
        for j, base in enumerate(range(0, G * G, 64)):
            inside = [c for c in range(base, min(base + 64, G * G)) if 1 <= c // G <= G - 2 and 1 <= c % G <= G - 2]
            if inside:
                put((inside[-1] // G, inside[-1] % G), S if j % 2 else B)
    elif k == 6:
        put((G - 2, max(1, G - 3)), B)
        put(last, S)
    elif k == 7:
        if G >= 5:
            lay = M.layouts(1, G, seed)[0]
        else:
            lay[1:-1, 1:-1] = B
            put(first, S)
            put(last, X)
    if variant == "v0":
        _force_goal_marker(lay, used or [first])
    return lay


def sparse_layouts(n, G, variant, seed):
    """uint8[n,G,G]: full 'W' border, every interior cell free with probability 1.5 / (G-2)^2 (0 / 1 / 2 free cells in
    about 22 / 33 / 25 % of the envs), a free cell 'B', 'S' or 'X' with weights 6:2:2; v0 gets an 'X' where none was drawn;
    the first eight envs are the fixed mazes."""
    rs = np.random.RandomState(seed)
    I = G - 2
    free = rs.rand(n, I, I) < min(1.5 / (I * I), 0.5)              # G = 3: one interior cell, free in half the envs
    kind = rs.choice(np.array([B, S, X], np.uint8), size=(n, I, I), p=[0.6, 0.2, 0.2])
    lay = np.full((n, G, G), W, np.uint8)
    lay[:, 1:-1, 1:-1] = np.where(free, kind, W)
    for i in range(n):
        if i < N_FIXED:
            lay[i] = fixed_maze(i, G, variant, seed)
        elif variant == "v0":
            _force_goal_marker(lay[i], [(1, 1)])
    return lay


def spawn_counts(lay, variant):
    """the cells the placement accepts, per maze: interior, not 'W', for v0 not 'X' either"""
    inner = lay[..., 1:-1, 1:-1]
    ok = (inner != W) & ((inner != X) if variant == "v0" else True)
    return ok.reshape(ok.shape[:-2] + (-1,)).sum(-1)


def case_seed(key):
    return zlib.crc32(repr(tuple(key)).encode())


def case_layouts(key):
    entry, variant, layout, G, N, T, k = key
    if layout == PER_ENV:
        return sparse_layouts(N, G, variant, case_seed(key))
    return fixed_maze(maze_of(layout), G, variant, case_seed(key))


# ---------------------------------------------------------------- closed-loop tables
def policy_table(G, key, seed):
    """uint8: the ball-keyed table walks down from even rows and up from odd ones, so that either the cell above or the
    cell below any 'S' steps onto it; every seventh cell holds another id, 'no move' ids (4, 7) among them.  The
    goal-conditioned table is random in 0..5."""
    rs = np.random.RandomState(seed)
    if key == "goal":
        return rs.randint(0, 6, G ** 4).astype(np.uint8)
    c = np.arange(G * G)
    t = np.where((c // G) % 2 == 0, 1, 0).astype(np.uint8)
    odd = c % 7 == 3
    t[odd] = rs.choice(np.array([2, 3, 4, 7], np.uint8), int(odd.sum()))
    return t


def sample_thresholds(G, key, seed):
    """uint32[S,4]: 0.85 on the policy_table action (uniform where that is no move); random rows, zeros among them, for the
    goal-conditioned table.  The conversion is include/lmaze.h's."""
    rs = np.random.RandomState(seed + 1)
    if key == "goal":
        p = rs.rand(G ** 4, 4) * (rs.rand(G ** 4, 4) < 0.8)
        p[p.sum(1) == 0] = 1.0
    else:
        t = policy_table(G, key, seed)
        p = np.full((G * G, 4), 0.05)
        p[t < 4, t[t < 4]] = 0.85
        p[t >= 4] = 0.25
    a = np.cumsum(p.astype(np.float64), axis=1)
    c = np.minimum(np.floor(a[:, :3] / a[:, 3:4] * 4294967296.0 + 0.5), 4294967295.0).astype(np.uint64).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate([c, np.zeros((len(c), 1), np.uint32)], axis=1))


def closed_loop_key(key):
    return "goal" if key[0] in (POLICY_GOAL, SAMPLE_GOAL) else "ball"


def closed_loop_table(key):
    entry, variant, layout, G, N, T, k = key
    make = policy_table if entry in (POLICY_BALL, POLICY_GOAL) else sample_thresholds
    return make(G, closed_loop_key(key), case_seed(key))


def closed_loop_actions(key, table):
    """the action rule of include/lmaze.h on the host, for the coverage run: act(t, state after the fused reset) -> int32[N]"""
    entry, variant, layout, G, N, T, k = key
    goal_keyed = closed_loop_key(key) == "goal"
    eps = min(int(EPSILON * 4294967296.0), 4294967295)

    def act(t, st, epoch):
        b = np.clip(st["ball_xy"], 0, G - 1).astype(np.int64)
        kk = b[:, 0] * G + b[:, 1]
        if goal_keyed:
            g = np.clip(st["goal_xy"], 0, G - 1).astype(np.int64)
            kk = kk + (g[:, 0] * G + g[:, 1]) * G * G
        r = explore_draw(SEED, epoch + t, ENV_BASE + np.arange(N, dtype=np.uint64))
        if entry in (SAMPLE_BALL, SAMPLE_GOAL):
            return sample_action(table[kk], r[0])
        a = table[kk].astype(np.int32)
        return np.where(r[0] < np.uint64(eps), (r[1] >> np.uint64(30)).astype(np.int32), a).astype(np.int32)
    return act


# ---------------------------------------------------------------- loaded state
OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1))                      # of action ids 0..3 (bookkeeping: where to aim from)


def _preferred_action(key):
    """the action a closed-loop case's table most likely takes at (ball cell, clamped goal cell); None for open loops"""
    entry, variant, layout, G, N, T, k = key
    if entry not in CLOSED:
        return None
    table = closed_loop_table(key)
    if entry in (SAMPLE_BALL, SAMPLE_GOAL):
        c = np.concatenate([np.zeros((len(table), 1)), table[:, :3].astype(np.float64), np.full((len(table), 1), 2.0 ** 32)], axis=1)
        table = np.diff(c, axis=1).argmax(1)
    goal_keyed = closed_loop_key(key) == "goal"

    def want(bx, by, goal):
        g = np.clip(goal, 0, G - 1)
        return int(table[(g[0] * G + g[1]) * G * G * goal_keyed + bx * G + by])
    return want


def loaded_state(key, lay):
    """(state dict for set_state(), actions int32[T,N], mask uint8[N]): ball_xy and goal_xy uniform in -3..G+2, about half
    the balls forced onto the grid (wall, border and free cells all occur); done from {0, 1, 2, 255}; step_count from
    {-5, 0, limit-2, limit-1, limit, limit+3}; reward from REWARD_BITS; actions in -1..5.  Where the entry point steps,
    some envs are AIMED, done clear: v0 envs whose maze has an 'S' stand beside it with step 0's action onto it and one of
    SPECIAL_REWARDS in turn -- the sticky pair that hands the pattern back; others stand on a wall cell beside a cell they
    can enter, with the action into it; the env behind the fixed mazes stands off the grid's corner and walks further out.
    The fixed mazes (the first envs of a per-env batch, every third env of a shared one) enter done, or pass the step
    limit at step 0, so that their resets fire inside the run."""
    entry, variant, layout, G, N, T, k = key
    rs = np.random.RandomState(case_seed(key) ^ 0x5EED)
    lim = STEP_LIMIT
    inner = interior_only(G)
    ball = rs.randint(-3, G + 3, (N, 2))
    on = rs.rand(N) < 0.5
    ball[on] = rs.randint(0, G, (int(on.sum()), 2))
    if inner:
        ball = rs.randint(1, G - 1, (N, 2))
    goal = rs.randint(-3, G + 3, (N, 2))
    done = np.where(rs.rand(N) < 0.55, 0, rs.choice(np.array([1, 2, 255]), N)).astype(np.uint8)
    sc = rs.choice(np.array([-5, 0, lim - 2, lim - 1, lim, lim + 3]), N).astype(np.int32)
    reward = REWARD_BITS[rs.randint(0, len(REWARD_BITS), N)].copy()
    acts = rs.randint(-1, 6, (max(T, 1), N)).astype(np.int32)
    mask = (rs.rand(N) < 0.5).astype(np.uint8)
    per_env = layout == PER_ENV
    fixed = np.arange(N) < N_FIXED if per_env else np.arange(N) % 3 == 0      # shared: every third env of the one maze
    mask[fixed] = 1
    done[fixed] = np.array([1, 2, 255], np.uint8)[np.arange(N)[fixed] % 3]
    want = _preferred_action(key)
    past_limit = lim if variant == "v3" else lim - 1                            # done at step 0: the reset fires at step 1
    aimed = 0

    def aim(i, targets, from_wall):
        """the ball of env i beside one of `targets`, step 0's action onto it"""
        li = lay[i] if per_env else lay
        tx, ty = targets[rs.randint(len(targets))]
        for d in np.roll(np.arange(4), -int(rs.randint(4))):
            bx, by = tx - OFFSETS[d][0], ty - OFFSETS[d][1]
            if (inner and not (1 <= bx <= G - 2 and 1 <= by <= G - 2)) or (from_wall and li[bx, by] != W):
                continue
            if want is not None and want(bx, by, goal[i]) != d:
                continue
            ball[i], acts[0, i], done[i] = (bx, by), d, 0
            if fixed[i]:
                sc[i] = past_limit
            return True
        return False
    for i in range(N if entry in TAKES_STEPS else 0):
        li = lay[i] if per_env else lay
        if per_env and i == N_FIXED and not inner:
            ball[i], acts[0, i], done[i] = (-3, G + 2), 0, 0
            continue
        sticky = np.argwhere(li == S) if variant == "v0" else ()
        enter = np.argwhere((li == B) | (li == X) | ((li == S) & (variant == "v3")))
        u = rs.rand()
        if per_env and i == 3 and len(enter):                     # first and last: off the wall into the first cell
            aim(i, enter, True)
        elif len(sticky) and (i < N_FIXED or u < (0.9 if per_env else 0.2)):
            if aim(i, sticky, False):
                reward[i] = SPECIAL_REWARDS[aimed % len(SPECIAL_REWARDS)]
                aimed += 1
        elif len(enter) and ((per_env and i < N_FIXED and i % 2) or (not fixed[i] and u < 0.25)):
            aim(i, enter, True)
    st = dict(ball_xy=ball.astype(np.int32), step_count=sc, done=done, reward=reward.view(np.float32),
              goal_count=rs.randint(0, 5, N).astype(np.int32))
    if variant == "v3":
        st["goal_xy"] = goal.astype(np.int32)
    return st, acts[:T] if T else acts[:0], mask


def host_state_of(key, lay, st):
    """the per-env arrays an env of the case holds after set_state(**st), as host_state() names them: v0's goal_xy is the
    layout's first 'X', row-major (the env looks it up once)"""
    entry, variant, layout, G, N, T, k = key
    out = {n: np.array(v, copy=True) for n, v in st.items()}
    if variant == "v0":
        first = (np.broadcast_to(lay, (N, G, G)).reshape(N, -1) == X).argmax(1)
        out["goal_xy"] = np.stack([first // G, first % G], 1).astype(np.int32)
    return out


# ---------------------------------------------------------------- the reference
COVERAGE = ("spawn0", "spawn1", "spawn2", "spawn3+", "reset_keeps_ball", "ball_clamped", "target_clamped", "off_wall",
            "goal_off_grid", "goal_only") + tuple("sticky_%08x" % b for b in SPECIAL_REWARDS)


class Reference(object):
    """The C oracle on the padded maze (unpadded where interior_only(G))."""

    def __init__(self, variant, layout, G, N, lay, step_limit=STEP_LIMIT, rewards=(-1.0, -0.01, 100.0)):
        self.v3, self.variant, self.G, self.N = variant == "v3", variant, G, N
        self.per_env = layout == PER_ENV
        self.lay = np.ascontiguousarray(lay)
        self.off = 0 if interior_only(G) else 1
        Gp = G + 2 * self.off
        if self.off:
            pad = ((0, 0),) * (self.lay.ndim - 2) + ((1, 1), (1, 1))
            self.layp = np.ascontiguousarray(np.pad(self.lay, pad, constant_values=W))
        else:
            self.layp = self.lay
        self.p = O.params(O.VARIANT_V3 if self.v3 else O.VARIANT_V0, Gp, O.LAYOUT_PER_ENV if self.per_env else O.LAYOUT_SHARED,
                          step_limit, *rewards)
        self.Gp = Gp
        self.counts = np.broadcast_to(spawn_counts(self.lay, variant), (N,))
        self.cov = OrderedDict((name, np.zeros(N, bool)) for name in COVERAGE)

    def _enter(self, st, clip):
        b = st["ball_xy"]
        if clip and self.off:
            b = np.clip(b, 0, self.G - 1)
        return (np.ascontiguousarray(b + self.off, dtype=np.int32),
                np.ascontiguousarray(st["goal_xy"] + self.off, dtype=np.int32) if self.v3 else None)

    def _crop(self, planes):
        return np.ascontiguousarray(planes[:, 1:-1, 1:-1]) if self.off else planes

    def _cell(self, xy):
        return self.lay[np.arange(self.N), xy[:, 0], xy[:, 1]] if self.per_env else self.lay[xy[:, 0], xy[:, 1]]

    def reset(self, st, mask, epoch):
        """lmaze_reset(mask) on st, in place; mask None = every env.  The ball enters as it is."""
        fired = np.ones(self.N, bool) if mask is None else np.asarray(mask) != 0
        c = self.counts
        for name, sel in (("spawn0", c == 0), ("spawn1", c == 1), ("spawn2", c == 2), ("spawn3+", c >= 3),
                          ("reset_keeps_ball", c <= (1 if self.v3 else 0)), ("goal_only", (c == 1) & self.v3)):
            self.cov[name] |= fired & sel
        b, g = self._enter(st, clip=False)
        O.reset(self.p, self.layp, None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8), SEED, epoch, b, g,
                st["step_count"], st["reward"], st["done"], None, env_base=ENV_BASE)
        st["ball_xy"][:] = b - self.off
        if self.v3:
            st["goal_xy"][:] = g - self.off

    def _cover_step(self, st, acts):
        G = self.G
        b = st["ball_xy"]
        cb = np.clip(b, 0, G - 1)
        off = np.array(OFFSETS + ((0, 0),))[np.where((acts >= 0) & (acts <= 3), acts, 4)]
        t = cb + off
        self.cov["ball_clamped"] |= (b != cb).any(1)
        self.cov["target_clamped"] |= ((t < 0) | (t > G - 1)).any(1)
        if self.v3:
            g = st["goal_xy"]
            self.cov["goal_off_grid"] |= ((g < 0) | (g > G - 1)).any(1)
        tc = np.clip(t, 0, G - 1)
        return cb, (self._cell(tc) == S) & (t == tc).all(1) & off.any(1), st["reward"].view(np.uint32).copy()

    def step(self, st, acts, planes=True):
        """one step of every env on st, in place: the ball clamped first.  Returns the cropped planes."""
        cb, onto_s, bits = self._cover_step(st, acts)
        b, g = self._enter(st, clip=True)
        obs = np.zeros((self.N, self.Gp, self.Gp), np.int32) if planes else None
        a = np.ascontiguousarray(acts, dtype=np.int32)
        if self.v3:
            O.step_v3(self.p, self.layp, a, b, g, st["step_count"], st["reward"], st["done"], obs)
        else:
            O.step_v0(self.p, self.layp, a, b, st["step_count"], st["reward"], st["done"], st["goal_count"], obs)
        st["ball_xy"][:] = b - self.off
        self.cov["off_wall"] |= (self._cell(cb) == W) & (st["ball_xy"] != cb).any(1)
        if not self.v3:
            kept = st["reward"].view(np.uint32) == bits
            for pat in SPECIAL_REWARDS:
                self.cov["sticky_%08x" % pat] |= onto_s & kept & (bits == pat)
        return self._crop(obs) if planes else None

    def observe(self, st):
        b, g = self._enter(st, clip=True)
        obs = np.zeros((self.N, self.Gp, self.Gp), np.int32)
        O.observe(self.p, self.layp, b, g, obs)
        return self._crop(obs)

    def coverage(self):
        return OrderedDict((name, int(v.sum())) for name, v in self.cov.items())


def run_reference(key, lay, state, acts, mask, epoch, act=None):
    """What the row's entry point must leave: dict(state, planes, rows of reward / done, slots, epoch, touched, coverage).
    state: host arrays as host_state() gives them (copied).  act(t, st, epoch): the closed loop's actions, asked after the
    fused reset of step t.  touched: the envs whose planes the call rewrites (None = all)."""
    entry, variant, layout, G, N, T, k = key
    st = {n: np.array(v, copy=True) for n, v in state.items()}
    ref = Reference(variant, layout, G, N, lay)
    out = dict(state=st, rows=(None, None), slots=[], touched=None, epoch=epoch)
    if entry in RESETS_ONLY:
        m = mask if entry == RESET_MASKED else None
        ref.reset(st, m, epoch)
        # masked: the planes were current on entry, and an env outside the mask keeps them -- untouched, or rewritten from
        # its unchanged state by a 16-byte store it shares with a reset env (include/lmaze.h lmaze_reset)
        out.update(planes=ref.observe(st), epoch=epoch + 1)
    elif entry in OBSERVES:
        ref._cover_step(st, np.full(N, -1, np.int32))
        out.update(planes=ref.observe(st), touched=mask != 0 if entry == OBSERVE_U8_MASKED else None)
    else:
        resets = entry not in (STEP, STEP_U8)
        rew, done, planes = [], [], None
        for t in range(T):
            if resets:
                ref.reset(st, st["done"].copy(), epoch + t)
            a = acts[t] if act is None else act(t, st, epoch)
            planes = ref.step(st, a)
            rew.append(st["reward"].copy())
            done.append(st["done"].copy())
            if k and (t + 1) % k == 0:
                out["slots"].append(planes)
        out.update(planes=planes, rows=(np.stack(rew), np.stack(done)), epoch=epoch + (T if resets else 0))
    out["coverage"] = ref.coverage()
    return out


def required_coverage(key):
    """the coverage names a per-env case must reach, by what its entry point does and what its grid admits"""
    entry, variant, layout, G, N, T, k = key
    need = []
    if entry in FIRES_RESETS:
        cells = (G - 2) ** 2 - (variant == "v0")                  # v0 gives one interior cell to its 'X'
        need += ["spawn0"] + ["spawn%s" % c for c, least in (("1", 1), ("2", 2), ("3+", 3)) if cells >= least]
        need += ["reset_keeps_ball"] + (["goal_only"] if variant == "v3" else [])
    if not interior_only(G):
        if entry in TAKES_STEPS + OBSERVES:
            need.append("ball_clamped")
        if entry in TAKES_STEPS:
            need.append("target_clamped")
    if entry in TAKES_STEPS:
        need.append("off_wall")
        if variant == "v0":
            need += ["sticky_%08x" % b for b in SPECIAL_REWARDS]
    if variant == "v3" and entry not in RESETS_ONLY:
        need.append("goal_off_grid")
    return need


# ---------------------------------------------------------------- the table
# odd N, ragged against every envs-per-workgroup size.  N_REG: the register-tiled (G*G a multiple of 256) and G >= 48 cases;
# at 131 envs a per-env batch has about 25 mazes with three or more spawn cells and 34 with an 'S', too few for 8 envs in
# every situation test_loaded_state_cpu.py asks for (5-7 were met), so it is 259
N_LDS, N_REG, N_SMALL, N_TINY = 515, 259, 13, 3
RESET_SHARED_G = (3, 4, 9, 12, 21, 62)
RESET_MAZES = (0, 3, 5, 7)                  # the shared mazes of the fused reset: count 0, 2 (v0: 1), one per ballot, ordinary
STEP_MAZES = (6, 7)
WAVE8_POLICIES = ((1, 1), (2, 2), (4, 3), (0, 0))


def _n(G):
    return N_REG if G * G % 256 == 0 or G >= 48 else N_LDS


def _rows():
    rows = []
    for v in ("v0", "v3"):
        # lmaze_reset, plain and masked, and its render
        for entry in RESETS_ONLY:
            rows += [Row(entry, v, shared(m), G, N_LDS, 1, None, 0) for G in RESET_SHARED_G for m in range(N_FIXED)]
            rows += [Row(entry, v, PER_ENV, G, _n(G), 1, None, 0) for G in (3, 5, 9, 11, 16, 32, 48, 64)]
        rows += [Row(RESET_MASKED, v, PER_ENV, 11, N_SMALL, 1, None, 0), Row(RESET, v, shared(3), 9, N_TINY, 1, None, 0)]
        # the step, with and without the fused reset
        for entry in (STEP, STEP_RESET):
            mazes = RESET_MAZES if entry == STEP_RESET else STEP_MAZES
            for m in mazes:
                for G in M.SPECIALISED + (5, 21, 62):
                    rows += [Row(entry, v, shared(m), G, N_LDS, T_STEPS, None, hint(sel=s, bit8=G == 8)) for s in M.SELS.get(G, range(4))]
                rows += [Row(entry, v, shared(m), 8, N_LDS, T_STEPS, None, hint(w, e)) for w, e in WAVE8_POLICIES]
            for G in (8, 9, 11, 16, 32, 48, 64):
                rows += [Row(entry, v, PER_ENV, G, _n(G), T_STEPS, None, h) for h in (0, hint(3, 2))]
        for entry in (STEP_U8, STEP_U8_RESET):
            mazes = RESET_MAZES if entry == STEP_U8_RESET else STEP_MAZES
            # 8: G*G = 64, a 16-byte store never straddles two envs, and the smallest grid at which a neighbour's
            # "no goal" value, added to G*G - c, lands inside a store (step_shared_u8_kernel's render)
            rows += [Row(entry, v, shared(m), G, N_LDS, T_STEPS, None, 0) for m in mazes for G in (4, 8, 11, 62)]
        rows += [Row(STEP_RESET, v, PER_ENV, 11, N_SMALL, T_STEPS, None, 0), Row(STEP_RESET, v, shared(3), 11, N_TINY, T_STEPS, None, 0)]
        # lmaze_observe of loaded state
        rows += [Row(OBSERVE, v, shared(7), G, N_LDS, 0, None, hint(bit8=b8)) for G in (5, 8, 11, 62) for b8 in ((False, True) if G == 8 else (False,))]
        rows += [Row(OBSERVE, v, PER_ENV, G, _n(G), 0, None, 0) for G in (9, 11, 16)]
        rows += [Row(e, v, shared(7), G, N_LDS, 0, None, 0) for e in (OBSERVE_U8, OBSERVE_U8_MASKED) for G in (4, 11, 62)]
        rows += [Row(OBSERVE, v, PER_ENV, 11, N_SMALL, 0, None, 0), Row(OBSERVE, v, shared(7), 11, N_TINY, 0, None, 0)]
        # the one-launch rollouts, plain and recording (k = 3), u8 forms included
        for entry, k in ((ROLLOUT, None), (ROLLOUT_OBS, K_REC)):
            for m in RESET_MAZES:
                rows += [Row(entry, v, shared(m), G, N_LDS, T_STEPS, k, hint(ro_epb=e)) for G in (11, 32) for e in (0, 3, 7)]
                rows.append(Row(entry, v, shared(m), 8, N_LDS, T_STEPS, k, 0))
            rows += [Row(entry, v, PER_ENV, G, _n(G), T_STEPS, k, hint(ro_epb=e)) for G in (11, 32) for e in (0, 5)]
        for entry, k in ((ROLLOUT_U8, None), (ROLLOUT_OBS_U8, K_REC)):
            rows += [Row(entry, v, shared(m), 11, N_LDS, T_STEPS, k, hint(ro_epb=e)) for m in RESET_MAZES for e in (0, 3, 7)]
            # the same body at the other shared sizes: 8 (stores never straddle two envs) and 32
            rows += [Row(entry, v, shared(m), G, N_LDS, T_STEPS, k, 0) for m in (3, 7) for G in (8, 32)]
        rows += [Row(ROLLOUT_OBS, v, PER_ENV, 11, N_SMALL, T_STEPS, K_REC, 0), Row(ROLLOUT_OBS, v, shared(3), 11, N_TINY, T_STEPS, K_REC, 0)]
        # the closed-loop rollouts: the transition inside their bodies
        for entry in CLOSED:
            if v == "v0" and entry in (POLICY_GOAL, SAMPLE_GOAL):
                continue
            rows += [Row(entry, v, lay, 11, N_LDS, T_STEPS, K_REC, 0) for lay in (shared(3), shared(7), PER_ENV)]
        rows += [Row(POLICY_BALL, v, PER_ENV, 11, N_SMALL, T_STEPS, K_REC, 0), Row(SAMPLE_BALL, v, shared(7), 11, N_TINY, T_STEPS, K_REC, 0)]
    return rows


ROWS = _rows()


def groups():
    """rows that differ in launch_hint only: one env, one reference run"""
    out = OrderedDict()
    for r in ROWS:
        out.setdefault(tuple(r[:-1]), []).append(r.hint)
    return out


def case_id(key):
    entry, variant, layout, G, N, T, k = key
    return "%s-%s-%s-G%d-N%d" % (entry, variant, layout, G, N)


def describe(abi, entry, variant, layout, G, N, T, obs_every, launch_hint):
    """what the launcher would queue for the row's step or rollout; '' for the entry points that have no describe call"""
    kind = PER_ENV if layout == PER_ENV else M.SHARED
    if entry in (STEP, STEP_RESET) + ROLLOUTS:
        return M.describe(abi, entry, variant, kind, G, N, T, obs_every, launch_hint)
    p = M.params(abi, variant, G, kind, launch_hint, STEP_LIMIT)
    if entry in (STEP_U8, STEP_U8_RESET):
        return abi.describe_step(p, N, auto_reset=entry == STEP_U8_RESET, with_obs="u8")
    if entry in CLOSED:
        f = abi.describe_rollout_policy if entry in (POLICY_BALL, POLICY_GOAL) else abi.describe_rollout_sample
        return f(p, N, T, True, True, obs_every, "goal" if entry in (POLICY_GOAL, SAMPLE_GOAL) else "ball")
    return ""
