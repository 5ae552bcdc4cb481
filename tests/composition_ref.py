"""What test_gpu_planning_compositions.py and its CPU twin share: the two compositions README.md prints under evaluate() and
occupancy() -- policy iteration as repeated evaluate(q=ev.q), and the softmax policy gradient d_sa (q - v) / tau -- with their
inputs, a float64 reference of the gradient and the bound it is held to.  Importing it needs no GPU."""
import functools

import numpy as np

import evaluate_ref as E
import helpers as H
import maze_ref as MZ
import occupancy_ref as OR
import solve_ref as SR

REWARDS = (-1.0, -0.01, 100.0)
SWEEPS = 4096
ROUND_LIMIT = 64                 # the loop gives up here; the twin asserts the reference ends well below it
U = 2.0 ** -24
V_ROUNDINGS = 8                  # test_evaluate_cpu.py's: || V32 - V ||_inf <= 8 u M / (1 - gamma)
D_ROUNDINGS = 11                 # test_occupancy_cpu.py's: || d32 - d ||_1 <= rel(11) || d ||_1 / (1 - gamma)
ETA = 2.0 ** -29                 # sum_a | p_a - pi_a | of a converted row, see gradient_bound()

# (variant, G, problems): the wave form with 1 and 2 cells per lane, six problems ragged against its four per workgroup, and the
# first workgroup form, a problem per workgroup
ITERATION_CASES = tuple((v, G, P) for v in ("v0", "v3") for G, P in ((5, 6), (11, 6), (18, 3)))
ITERATION_GAMMAS = (0.9, 0.99)
GRADIENT_CASES = tuple((v, G, P, tau) for v in ("v3", "v0") for G, P in ((11, 6), (18, 3)) for tau in (1.0, 0.5))
GRADIENT_GAMMA = 0.9


def rel(n):
    return n * U / (1 - n * U)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------- policy iteration
@functools.lru_cache(maxsize=None)
def iteration_problem(variant, G, P):
    """(layouts uint8[P,G,G], goals int32[P,2] or None, models, the start policy uint8[P, G*G]): random bordered mazes with an
    'X' and an 'S' each, v3 with a random free goal, and random bytes 0..3 to start from.  Read only."""
    lays = H.bordered_random_layouts(P, G, 7)
    goals = H.random_free_cells(lays, 5) if variant == "v3" else None
    pol = np.random.RandomState(G).randint(0, 4, (P, G * G)).astype(np.uint8)
    return lays, goals, SR.models_of(variant, lays, goals, REWARDS), pol


def iterate(evaluate, pol0, limit=ROUND_LIMIT):
    """README.md's loop: ev = evaluate(policy=pi), then ev = evaluate(q=ev.q) until the first maxima of ev.q stop changing.
    evaluate(policy= | q=) returns numpy (q float32[P,S,4], v float32[P,S], sweeps_run int32[P]).  Returns every round's tuple;
    the last two have the same first maxima.  A batch runs until no problem's maxima change: a problem that is through repeats
    its last round bit for bit, since its q= is read to the same policy."""
    rounds = [evaluate(policy=pol0)]
    while True:
        rounds.append(evaluate(q=rounds[-1][0]))
        if (E.first_max(rounds[-1][0]) == E.first_max(rounds[-2][0])).all():
            return rounds
        assert len(rounds) < limit, "policy iteration did not end in %d rounds" % limit


def reference_rounds(variant, lays, goals, models, pol0, gamma):
    def evaluate(**table):
        got = E.evaluate_many(variant, lays, goals, gamma, SWEEPS, rewards=REWARDS, models=models, epsilon_u32=0, **table)
        return got.q, got.v, got.sweeps_run
    return iterate(evaluate, pol0)


def same_rounds(got, ref, what):
    """Every round's q, v and sweeps_run bit for bit, as many rounds, every evaluation at its exact stop"""
    for k, (a, b) in enumerate(zip(got, ref)):
        for name, x, y in zip(("q", "v", "sweeps_run"), a, b):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and x.dtype == y.dtype, (what, k, name, x.shape, y.shape)
            bad = (bits(x) != bits(y)) if x.dtype == np.float32 else (x != y)
            assert not bad.any(), (what, "round", k, name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
        assert (np.asarray(a[2]) < SWEEPS).all(), (what, "round", k, "not at the exact stop")
    assert len(got) == len(ref), (what, len(got), len(ref))


def ends_at_the_solution(models, last, solved_v, solved_policy, summary, what):
    """The final v is solve()'s in every bit; the first maxima of the final q are solve()'s policy on every state that is not a
    wall and has a usable pair; the walk of those maxima is a shortest one from every cell that can reach done (summary:
    reachable, arrived, shortest, excess)"""
    q, v, _ = last
    bad = bits(v) != bits(solved_v)
    assert not bad.any(), (what, "v is not solve()'s", int(bad.sum()), np.argwhere(bad)[:5].tolist())
    live = np.stack([~m.wall & ~m.sticky.all(1) for m in models]).reshape(np.asarray(solved_policy).shape)
    assert live.any() and (E.first_max(q).reshape(live.shape)[live] == np.asarray(solved_policy)[live]).all(), what
    summary = np.asarray(summary).reshape(-1, 4)
    assert (summary[:, 0] > 0).any() and (summary[:, 1] == summary[:, 0]).all() and (summary[:, 2] == summary[:, 0]).all(), (what, summary)


# ------------------------------------------------------------- the softmax policy gradient
@functools.lru_cache(maxsize=None)
def gradient_problem(variant, G, P):
    """(layouts, goals or None, models, logits float32[P,S,4], start float32[P,S]): v3 on iteration_problem()'s mazes, v0 on
    generated mazes, which have no 'S' -- no pair of any state is excluded, which is where README.md claims the formula;
    logits O(1); start random on the cells that are not walls, summing to 1.  Read only."""
    if variant == "v3":
        lays, goals, models, _ = iteration_problem("v3", G, P)
    else:
        lays, goals = MZ.generate(G, P, 7)[0], None
        models = SR.models_of("v0", lays, None, REWARDS)
    assert not any(m.sticky.any() for m in models)
    rs = np.random.RandomState(100 + G)
    logits = rs.randn(P, G * G, 4).astype(np.float32)
    free = np.stack([~m.wall for m in models])
    start = np.where(free, rs.rand(P, G * G), 0.0)
    return lays, goals, models, logits, (start / start.sum(1, keepdims=True)).astype(np.float32)


def softmax64(logits, tau):
    z = np.asarray(logits).astype(np.float64) / float(tau)
    z = np.exp(z - z.max(-1, keepdims=True))
    return z / z.sum(-1, keepdims=True)


def expected_return(model, gamma, logits, tau, start):
    """J = <start, V> in float64 with the exact softmax probabilities"""
    pi = np.where(model.wall[:, None], 0.0, softmax64(logits, tau))
    return float(np.asarray(start, np.float64) @ E.exact_values_of(model, gamma, pi))


def exact_gradient(model, gamma, logits, tau, start):
    """(dJ / dlogits float64[S,4], dict of its parts): d pi (Q - V) / tau from float64 linear solves for V, Q and d with the
    exact softmax probabilities, not the thresholds"""
    pi = np.where(model.wall[:, None], 0.0, softmax64(logits, tau))
    V = E.exact_values_of(model, gamma, pi)
    Q = E.exact_action_values(model, gamma, V)
    d = OR.exact_occupancy_of(model, gamma, pi, start)
    return d[:, None] * pi * (Q - V[:, None]) / float(tau), dict(pi=pi, V=V, Q=Q, d=d)


def float32_gradient(d_sa, q, v, tau):
    """README.md's line, in float64 from the float32 outputs"""
    return np.asarray(d_sa, np.float64) * (np.asarray(q, np.float64) - np.asarray(v, np.float64)[..., None]) / float(tau)


def gradient_bound(gamma, tau, q32, d32, parts, g32):
    """|| g32 - g64 ||_1 of one maze where no pair is excluded.  With A = Q - V and d_sa = d pi,
        tau (g32 - g64) = (d_sa32 - d_sa) A32 + d_sa (A32 - A),
    so tau || g32 - g64 ||_1 <= max|A32| || d_sa32 - d_sa ||_1 + || d ||_1 max|A32 - A| <= 2 M E_dsa + 2 m E_v, with M >= |Q|, |V|
    on both sides and m >= || d ||_1 on both sides.  Each error has two parts.  Rounding, against the exact solve with the
    probabilities p the kernels weigh: the suite's bounds E_v = 8 u M / (1 - gamma) (test_evaluate_cpu.py; on v, hence on q =
    r + gamma v) and E_d = rel(11) m / (1 - gamma) (test_occupancy_cpu.py), and || d_sa32 - d_sa ||_1 <= (1 + rel(4)) E_d +
    rel(4) m as in test_duality_on_the_gpus_own_outputs.  Quantisation, p against the softmax pi: a threshold is a cumulative
    probability rounded to a multiple of 2^-32 (one off at most where it is clamped), so |p_a - pi_a| <= 2^-31 and
    sum_a |p_a - pi_a| <= ETA = 2^-29 per state; then V_p - V_pi = (I - gamma P_p)^-1 (sum_a (p_a - pi_a) Q_pi(., a)) is at most
    ETA M / (1 - gamma) in every state, d_p - d_pi = gamma (I - gamma P_p^T)^-1 (P_p - P_pi)^T d_pi at most ETA m / (1 - gamma) in
    L1, and d_p p - d_pi pi at most that plus ETA m.  Last, the products of float32_gradient() are float64: three roundings on
    every entry of g32.  M and m are taken from both sides with a factor that covers the exact middle one."""
    g = float(np.float32(gamma))
    M = max(float(np.abs(q32).max()), float(np.abs(parts["Q"]).max())) * (1 + 2.0 ** -16)
    m = max(float(np.asarray(d32, np.float64).sum()), float(parts["d"].sum())) * (1 + 2 * rel(D_ROUNDINGS) / (1 - g) + 2 * ETA / (1 - g))
    e_v = (V_ROUNDINGS * U + ETA) * M / (1 - g)
    e_dsa = (1 + rel(4)) * rel(D_ROUNDINGS) * m / (1 - g) + rel(4) * m + ETA * m / (1 - g) + ETA * m
    return (2 * M * e_dsa + 2 * m * e_v) / float(tau) + 4 * 2.0 ** -53 * float(np.abs(g32).sum())
