"""GPU: the off-policy kernels against their numpy restatements (offpolicy_ref.py) -- lmaze_action_probs bit for bit on all
three table forms, lmaze_vtrace / lmaze_vtrace_table bit for bit against the float32 loop, on fabricated rows that hold every
special case and on the rows real closed-loop rollouts write; on-policy against gae(); the table form against the composition
it replaces; outputs that alias inputs; what the Python surface refuses."""
import importlib
import itertools

import numpy as np
import pytest
import torch

import offpolicy_ref as R
import tabular_ref as TR

pytestmark = pytest.mark.gpu

PKG = importlib.import_module("gym-lmaze_amd")
DEV = torch.device("cuda", 0)
INF = float("inf")
F = np.float32
# T below, at and across the block depths (4 and 8 rows), N off 64 and 256, more than one workgroup
SHAPES = [(1, 1), (9, 257), (13, 777), (64, 4099)]
DISCOUNTS = [(0.0, 0.0), (0.99, 0.95), (1.0, 1.0)]
CLIPS = [(1.0, 1.0), (INF, INF), (2.0, 0.5)]
KINDS = ("thresholds", "policy", "q")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def _bits(x):
    return np.ascontiguousarray(_np(x) if isinstance(x, torch.Tensor) else x, dtype=F).view(np.uint32)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _record(kind, table, eps32=0):
    """(the table_policy() record of a numpy table on the GPU, eps32 as the epsilon that converts to it)"""
    eps = {0: 0.0, R.EPSILONS[1]: 0.1, R.EPSILONS[2]: 1.0}[eps32]
    rec = PKG.table_policy(**{kind: _dev(table)}, **({} if kind == "thresholds" else {"epsilon": eps}))
    assert rec.epsilon_u32 == (0 if kind == "thresholds" else eps32) and rec.keys == len(table)
    return rec


# ------------------------------------------------------------- action_probs
@pytest.mark.parametrize("keys", [1, 121, 14641])
def test_action_probs_bit_exact(keys):
    tables = R.special_tables(keys, keys)
    for (T, N), kind in itertools.product(SHAPES, KINDS):
        key, act = R.special_samples(keys, T * N, T + N)
        k, a = _dev(key.reshape(T, N)), _dev(act.reshape(T, N))
        for e in (R.EPSILONS if kind != "thresholds" else (0,)):
            p = PKG.action_probs(k, a, _record(kind, tables[kind], e))
            assert p.dtype == torch.float32 and tuple(p.shape) == (T, N)
            want = R.probs(R.weights(kind, tables[kind], key, act, e))
            assert (_bits(p).reshape(-1) == _bits(want)).all(), (T, N, kind, e)
    assert ((want > 0) & (want < 1)).any()


@pytest.mark.parametrize("kind", KINDS)
def test_action_probs_on_rows_sliced_off_a_16_byte_boundary(kind):
    keys, m = 121, 13 * 777
    table = R.special_tables(keys, 3)[kind]
    key, act = R.special_samples(keys, m, 4)
    kb, ab = torch.zeros(m + 3, dtype=torch.int32, device=DEV), torch.zeros(m + 3, dtype=torch.int32, device=DEV)
    k, a = kb[1:m + 1], ab[3:m + 3]
    k.copy_(_dev(key))
    a.copy_(_dev(act))
    assert k.data_ptr() % 16 == 4 and a.data_ptr() % 16 == 12 and k.is_contiguous()
    out = torch.full((m + 2,), -7.0, device=DEV)
    p = PKG.action_probs(k, a, _record(kind, table, R.EPSILONS[1] if kind != "thresholds" else 0), out=out[2:])
    assert p.data_ptr() == out[2:].data_ptr()
    want = R.probs(R.weights(kind, table, key, act, R.EPSILONS[1]))
    assert (_bits(p) == _bits(want)).all() and _np(out[:2]).tolist() == [-7.0, -7.0]


# ------------------------------------------------------------- vtrace, rows form
@pytest.mark.parametrize("gamma,lam", DISCOUNTS)
@pytest.mark.parametrize("T,N", SHAPES)
def test_vtrace_rows_bit_exact(T, N, gamma, lam):
    reward, done, value, tail, ratio = R.special_rows(T, N, 0.1, 7 * T + N)
    r, d, v, x, tl = _dev(reward), _dev(done), _dev(value), _dev(ratio), _dev(tail)
    for rho_bar, c_bar in CLIPS:
        for with_tail in (False, True):
            want_vs, want_pg = R.vtrace_numpy(reward, done, value, tail if with_tail else None, ratio, gamma, lam, rho_bar, c_bar)
            vs, pg, none = PKG.vtrace(r, d, gamma, lam, value_t=v, tail=tl if with_tail else None, rho_t=x, rho_bar=rho_bar, c_bar=c_bar)
            assert none is None and vs.dtype == pg.dtype == torch.float32 and tuple(vs.shape) == tuple(pg.shape) == (T, N)
            assert (_bits(vs) == _bits(want_vs)).all(), (rho_bar, c_bar, with_tail)
            assert (_bits(pg) == _bits(want_pg)).all(), (rho_bar, c_bar, with_tail)
        vs2, none, _ = PKG.vtrace(r, d.view(torch.bool), gamma, lam, value_t=v, tail=tl, rho_t=x, rho_bar=rho_bar, c_bar=c_bar, pg=False)
        assert none is None and (_bits(vs2) == _bits(want_vs)).all()
    # the done row with r = -0.0 and v = 0: pg = 1 * (-0.0 - 0.0) keeps its sign
    assert _bits(pg).flat[0] == 0x80000000 and _bits(vs).flat[0] == 0
    assert (_bits(r) == _bits(reward)).all() and (_bits(v) == _bits(value)).all() and (_bits(x) == _bits(ratio)).all()


# ------------------------------------------------------------- on-policy is gae()
@pytest.mark.parametrize("gamma,lam", DISCOUNTS)
@pytest.mark.parametrize("T,N", SHAPES)
def test_on_policy_vtrace_is_gae_in_every_bit(T, N, gamma, lam):
    """rho_t=None in the rows form; the same record as behaviour and target in the table form, on rows that table can have
    produced (keys inside it, actions 0 .. 3 that carry weight in every row): every ratio is exactly 1"""
    keys = 121
    rs = np.random.RandomState(N)
    reward, done, value, tail, _ = R.special_rows(T, N, 0.1, T + 3 * N)
    key, act = rs.randint(0, keys, (T, N)).astype(np.int32), rs.randint(0, 4, (T, N)).astype(np.int32)
    key_tail = np.resize(np.array([5, -1, keys, 17, 120], np.int32), N)
    values = (rs.randn(keys) * 20).astype(F)
    r, d, v, tl = _dev(reward), _dev(done), _dev(value), _dev(tail)
    k, a, kt, vals = _dev(key), _dev(act), _dev(key_tail), _dev(values)
    adv, tgt = PKG.gae(r, d, gamma, lam, value_t=v, tail=tl)
    adv_k, tgt_k = PKG.gae(r, d, gamma, lam, values=vals, key_t=k, key_tail=kt)
    tables = dict(R.special_tables(keys, 9), thresholds=R.min_law_table(keys, 9))
    for rho_bar, c_bar in CLIPS[:2]:
        vs, _, _ = PKG.vtrace(r, d, gamma, lam, value_t=v, tail=tl, rho_bar=rho_bar, c_bar=c_bar)
        assert _same(vs, tgt) and _same(vs, adv + v)
        for kind in KINDS:
            rec = _record(kind, tables[kind], R.EPSILONS[1] if kind != "thresholds" else 0)
            vs, _, rho = PKG.vtrace(r, d, gamma, lam, values=vals, key_t=k, key_tail=kt, actions_t=a, behaviour=rec, target=rec,
                                    rho_bar=rho_bar, c_bar=c_bar, ratios=True)
            assert bool((rho == 1).all()), kind
            assert _same(vs, tgt_k) and _same(vs, adv_k + _dev(TR.table_values(values, key))), (kind, rho_bar)


# ------------------------------------------------------------- the table form is the composition it replaces
@pytest.mark.parametrize("b_kind,t_kind", list(itertools.product(KINDS, KINDS)))
def test_vtrace_table_form_is_the_composition(b_kind, t_kind):
    keys = 121
    for T, N in SHAPES[1:]:
        reward, done, _, _, _ = R.special_rows(T, N, 0.1, T + N)
        key, act = R.special_samples(keys, T * N, T)
        key, act = key.reshape(T, N), act.reshape(T, N)
        key_tail = np.resize(np.array([5, -1, keys, 17, 120], np.int32), N)
        values = (np.random.RandomState(T).randn(keys) * 20).astype(F)
        tb, tt = R.special_tables(keys, 1)[b_kind], R.special_tables(keys, 2)[t_kind]
        eb, et = (0 if b_kind == "thresholds" else R.EPSILONS[1]), (0 if t_kind == "thresholds" else R.EPSILONS[2])
        behaviour, target = _record(b_kind, tb, eb), _record(t_kind, tt, et)
        r, d, k, a, kt, vals = _dev(reward), _dev(done), _dev(key), _dev(act), _dev(key_tail), _dev(values)
        vs, pg, rho = PKG.vtrace(r, d, 0.99, 0.95, values=vals, key_t=k, key_tail=kt, actions_t=a, behaviour=behaviour, target=target,
                                 rho_bar=2.0, c_bar=0.5, ratios=True)
        # the composition: two action_probs, a division, a gather, the rows form
        pt, pb = PKG.action_probs(k, a, target), PKG.action_probs(k, a, behaviour)
        ratio = torch.where(pb == 0, torch.zeros_like(pb), pt / pb)
        inside = (k >= 0) & (k < keys)
        v_rows = torch.where(inside, vals[torch.where(inside, k, torch.zeros_like(k)).long()], torch.zeros_like(r))
        kti = (kt >= 0) & (kt < keys)
        v_tail = torch.where(kti, vals[torch.where(kti, kt, torch.zeros_like(kt)).long()], torch.zeros(N, device=DEV))
        vs_c, pg_c, _ = PKG.vtrace(r, d, 0.99, 0.95, value_t=v_rows, tail=v_tail, rho_t=ratio, rho_bar=2.0, c_bar=0.5)
        assert _same(rho, ratio) and _same(vs, vs_c) and _same(pg, pg_c), (T, N)
        # ... and the restatement
        want_rho = R.ratios(R.weights(t_kind, tt, key, act, et), R.weights(b_kind, tb, key, act, eb))
        assert (_bits(rho) == _bits(want_rho)).all() and (want_rho == 0).any() and (want_rho > 1).any()
        want_vs, want_pg = R.vtrace_numpy(reward, done, TR.table_values(values, key), TR.table_values(values, key_tail), want_rho,
                                          0.99, 0.95, 2.0, 0.5)
        assert (_bits(vs) == _bits(want_vs)).all() and (_bits(pg) == _bits(want_pg)).all()
        # only one output; no key_tail
        none_vs = PKG.vtrace(r, d, 0.99, 0.95, values=vals, key_t=k, actions_t=a, behaviour=behaviour, target=target, pg=False)
        assert none_vs[1] is None and none_vs[2] is None


# ------------------------------------------------------------- aliasing
@pytest.mark.parametrize("T,N", SHAPES[1:])
def test_vtrace_outputs_may_alias_inputs(T, N):
    """vs_t is value_t and pg_adv_t is reward_t in the rows form: the unaliased results"""
    reward, done, value, tail, ratio = R.special_rows(T, N, 0.1, 3)
    want_vs, want_pg, _ = PKG.vtrace(_dev(reward), _dev(done), 0.99, 0.95, value_t=_dev(value), tail=_dev(tail), rho_t=_dev(ratio),
                                     rho_bar=2.0, c_bar=0.5)
    r, v = _dev(reward), _dev(value)
    vs, pg, _ = PKG.vtrace(r, _dev(done), 0.99, 0.95, value_t=v, tail=_dev(tail), rho_t=_dev(ratio), rho_bar=2.0, c_bar=0.5, out=v, pg=r)
    assert vs is v and pg is r and _same(v, want_vs) and _same(r, want_pg)
    # the table form: the advantages over the rewards, the ratios kept
    keys = 121
    key, act = R.special_samples(keys, T * N, 5)
    tables = R.special_tables(keys, 6)
    b, t = _record("policy", tables["policy"], R.EPSILONS[1]), _record("q", tables["q"], 0)
    args = dict(values=_dev((np.random.RandomState(2).randn(keys) * 9).astype(F)), key_t=_dev(key.reshape(T, N)),
                actions_t=_dev(act.reshape(T, N)), behaviour=b, target=t, rho_bar=INF, c_bar=1.0)
    want = PKG.vtrace(_dev(reward), _dev(done), 0.99, 0.95, ratios=True, **args)
    r = _dev(reward)
    got = PKG.vtrace(r, _dev(done), 0.99, 0.95, pg=r, ratios=True, **args)
    assert got[1] is r and all(_same(x, y) for x, y in zip(got, want))


# ------------------------------------------------------------- the rows of a real rollout
@pytest.mark.parametrize("variant,key", [("v0", "ball"), ("v3", "goal")])
def test_vtrace_on_the_rows_of_a_real_rollout(variant, key):
    """rollout_sample(logits=a) on 4 096 x 11x11 for T = 32; the target is table_policy(logits=b), the critic evaluate(logits=b).v"""
    N, G, T, gamma, lam = 4096, 11, 32, 0.9, 0.95
    lay = PKG.layouts.to_codes(PKG.layouts.open_room(G, (G // 2, G // 2)))
    env = PKG.LmazeVecEnv(N, variant=variant, layout=lay, device=DEV, seed=23, step_limit=20)
    env.reset()
    S = G ** 4 if key == "goal" else G * G
    gen = torch.Generator(device=DEV).manual_seed(5)
    la, lb = torch.randn((S, 4), device=DEV, generator=gen), torch.randn((S, 4), device=DEV, generator=gen)
    _, _, _, rew_t, done_t, act_t, key_t = env.rollout_sample(T, logits=la, key=key, trajectory=True)
    key_tail = env.state_keys(key)
    old, new = PKG.table_policy(logits=la), PKG.table_policy(logits=lb, keys=S)
    values = env.evaluate(logits=lb, key=key, gamma=gamma).v.reshape(-1).contiguous()
    assert tuple(values.shape) == (S,)
    vs, pg, rho = PKG.vtrace(rew_t, done_t, gamma, lam, values=values, key_t=key_t, key_tail=key_tail, actions_t=act_t, behaviour=old,
                             target=new, ratios=True)
    k, a, kt, vals = _np(key_t), _np(act_t), _np(key_tail), _np(values)
    assert k.min() >= 0 and k.max() < S and a.min() >= 0 and a.max() <= 3 and _np(done_t).any() and not _np(done_t).all()
    tha, thb = _np(old.table.view(torch.int32)).view(np.uint32), _np(new.table.view(torch.int32)).view(np.uint32)
    wb = R.weights("thresholds", tha, k, a)
    assert (wb > 0).all()                                              # the rollout drew every action from the table it ran
    want_rho = R.ratios(R.weights("thresholds", thb, k, a), wb)
    assert (_bits(rho) == _bits(want_rho)).all() and len(np.unique(want_rho)) > 100
    want_vs, want_pg = R.vtrace_numpy(_np(rew_t), _np(done_t), TR.table_values(vals, k), TR.table_values(vals, kt), want_rho, gamma, lam,
                                      1.0, 1.0)
    assert (_bits(vs) == _bits(want_vs)).all() and (_bits(pg) == _bits(want_pg)).all()
    # the log-prob row, and the composition the README names: the advantages per (key, action)
    logp = torch.log(PKG.action_probs(key_t, act_t, old))
    assert bool(torch.isfinite(logp).all()) and (_bits(PKG.action_probs(key_t, act_t, old)) == _bits(R.probs(wb))).all()
    count, total = PKG.table_stats(key_t, act_t, pg, keys=S)
    assert int(count.sum()) == T * N and total is not None
    # b = a: on-policy, gae() in every bit
    adv, tgt = PKG.gae(rew_t, done_t, gamma, lam, values=values, key_t=key_t, key_tail=key_tail)
    vs_on, _, rho_on = PKG.vtrace(rew_t, done_t, gamma, lam, values=values, key_t=key_t, key_tail=key_tail, actions_t=act_t,
                                  behaviour=old, target=PKG.table_policy(logits=la), ratios=True)
    assert bool((rho_on == 1).all()) and _same(vs_on, tgt)


# ------------------------------------------------------------- refusals and no-ops
def test_python_refusals_and_nothing_to_do():
    T, N, keys = 5, 7, 121
    r, d = torch.zeros((T, N), device=DEV), torch.zeros((T, N), dtype=torch.uint8, device=DEV)
    v, x = torch.zeros((T, N), device=DEV), torch.ones((T, N), device=DEV)
    k, a = torch.zeros((T, N), dtype=torch.int32, device=DEV), torch.zeros((T, N), dtype=torch.int32, device=DEV)
    vals = torch.zeros(keys, device=DEV)
    rec = PKG.table_policy(policy=torch.zeros(keys, dtype=torch.uint8, device=DEV), epsilon=0.1)
    cpu = PKG.table_policy(policy=torch.zeros(keys, dtype=torch.uint8), epsilon=0.1)
    short = PKG.table_policy(policy=torch.zeros(keys - 1, dtype=torch.uint8, device=DEV))
    table = dict(values=vals, key_t=k, actions_t=a, behaviour=rec, target=rec)
    bad = [dict(value_t=v, **table),                                                  # two value sources
           dict(),                                                                   # none
           dict(table, target=None), dict(table, behaviour=None),                    # one record without the other
           dict(table, rho_t=x),                                                     # rho_t= with the table form
           dict(value_t=v, behaviour=rec, target=rec), dict(value_t=v, actions_t=a), dict(value_t=v, ratios=True),
           dict(value_t=v, key_tail=torch.zeros(N, dtype=torch.int32, device=DEV)), dict(table, tail=torch.zeros(N, device=DEV)),
           dict(value_t=v.double()), dict(value_t=v[:, :3]), dict(value_t=v.cpu()), dict(value_t=v, rho_t=x.double()),
           dict(value_t=v, rho_t=x[:4]), dict(value_t=v, rho_t=x.cpu()), dict(value_t=v, tail=torch.zeros(N + 1, device=DEV)),
           dict(table, actions_t=a.long()), dict(table, actions_t=None), dict(table, key_t=k.long()), dict(table, values=vals.double()),
           dict(table, behaviour=cpu), dict(table, target=short), dict(table, target="greedy"),
           dict(value_t=v, out=v.double()), dict(value_t=v, pg=x[:4]), dict(value_t=v, out=x, pg=x),
           dict(table, ratios=x.cpu())]
    for kw in bad:
        with pytest.raises(ValueError):
            PKG.vtrace(r, d, 0.99, 0.95, **kw)
    for args in ((r.cpu(), d), (r, d.float()), (r.double(), d), (r[:, :3], d)):
        with pytest.raises(ValueError):
            PKG.vtrace(*args, 0.99, 0.95, value_t=v)
    for args in ((k.cpu(), a, rec), (k, a.long(), rec), (k, a[:4], rec), (k.long(), a, rec), (k, a, cpu), (k, a, "table"), (k[:, :3], a, rec)):
        with pytest.raises(ValueError):
            PKG.action_probs(*args)
    with pytest.raises(ValueError):
        PKG.action_probs(k, a, rec, out=x.double())
    # nothing to do: T == 0 and N == 0 return shaped outputs without a call (an empty tensor has no address to pass)
    for shape in ((0, N), (T, 0), (0, 0)):
        e, eb, ei = torch.zeros(shape, device=DEV), torch.zeros(shape, dtype=torch.bool, device=DEV), torch.zeros(shape, dtype=torch.int32, device=DEV)
        vs, pg, rho = PKG.vtrace(e, eb, 0.99, 0.95, value_t=e)
        assert tuple(vs.shape) == tuple(pg.shape) == shape and rho is None
        vs, pg, rho = PKG.vtrace(e, eb, 0.99, 0.95, values=vals, key_t=ei, actions_t=ei, behaviour=rec, target=rec, pg=False, ratios=True)
        assert tuple(vs.shape) == tuple(rho.shape) == shape and pg is None
        assert tuple(PKG.action_probs(ei, ei, rec).shape) == shape
    # defaults: lam = 1, both bars 1
    vs, pg, _ = PKG.vtrace(r, d, 0.99, value_t=v)
    assert _same(vs, PKG.vtrace(r, d, 0.99, 1.0, value_t=v, rho_bar=1.0, c_bar=1.0)[0])
