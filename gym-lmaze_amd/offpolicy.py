"""Off-policy learning from rollout rows: the probability with which a table rule records an action (action_probs) and
V-trace over rows whose table is no longer the one being learnt (vtrace) -- include/lmaze.h lmaze_action_probs, lmaze_vtrace,
lmaze_vtrace_table.  A table is named once, as a table_policy() record, and converted by the rules the rollouts and
evaluate_tables() convert theirs by (_tables, _abi): nothing is restated here."""
import collections

import torch

from . import _abi
from . import _tables
from .vec_env import _rows_like, _value_source


class TablePolicy(collections.namedtuple("TablePolicy", "kind table epsilon_u32 keys")):
    """One checked table of `keys` rows in the form the kernels read: kind "policy" (uint8[keys]), "q" (float32[keys, 4]) or
    "thresholds" (uint32[keys, 4]); epsilon_u32 goes with the first two.  Made by table_policy()."""
    __slots__ = ()

    @property
    def device(self):
        return self.table.device

    def _law(self):
        """(policy, q, epsilon_u32, thresholds): the four arguments one table takes in the C entries"""
        at = self.table.data_ptr()
        return (at if self.kind == "policy" else None, at if self.kind == "q" else None, self.epsilon_u32,
                at if self.kind == "thresholds" else None)


def table_policy(policy=None, q=None, probs=None, logits=None, thresholds=None, epsilon=0.0, temperature=1.0, keys=None):
    """The record action_probs() and vtrace() take for one table, of exactly one of
    policy      uint8[S] with epsilon: the epsilon-greedy rule rollout_policy(policy=, epsilon=) runs, kept as bytes -- an id
                above 3, which the rollout records as it stands, carries its greedy share;
    q           float32[S, 4], contiguous and 16-byte aligned, with epsilon: kept as q, the greedy action being the FIRST
                maximum (rollout_qlearn()'s and evaluate_tables(q=)'s rule; rollout_policy(q=) reads a row with a NaN as "no
                move", so name what it ran as policy=greedy_table(q));
    probs       float[S, 4] of non-negative weights, converted by _abi.sampling_thresholds() as rollout_sample() does;
    logits      float[S, 4]: sampling_thresholds(softmax(logits.double() / temperature)), temperature > 0;
    thresholds  the table itself, uint32 (or int32, the same bits) [S, 4], contiguous and 16-byte aligned: the caller's
                memory, never a copy.
    epsilon != 0 with a categorical input is refused.  keys: the number of rows S the table must have (default: what it has).
    What the record stands for is the law of the action a rollout RECORDS, with no exclusion and no renormalisation -- not
    evaluate_tables()' law, which is conditioned on the usable pairs.  Host side only; nothing launches."""
    given = {"policy": policy, "q": q, "probs": probs, "logits": logits, "thresholds": thresholds}
    kind = _tables.exactly_one("table_policy()", **given)
    src = given[kind]
    if not (isinstance(src, torch.Tensor) and src.dim() >= 1 and src.shape[0] >= 1):
        raise ValueError("%s must be a tensor of at least one row" % kind)
    S = int(src.shape[0])
    if keys is not None and int(keys) != S:
        raise ValueError("%s has %d rows, keys=%d" % (kind, S, int(keys)))
    eps = _abi.epsilon_u32(epsilon)
    what = "keys=%d" % S
    if kind == "policy":
        return TablePolicy("policy", _tables.greedy_policy(src, None, S, src.device, what), eps, S)
    if kind == "q":
        if not (src.dtype == torch.float32 and tuple(src.shape) == (S, 4) and src.is_contiguous() and src.data_ptr() % 16 == 0):
            raise ValueError("q must be a contiguous, 16-byte aligned float32 tensor [%d, 4] (%s)" % (S, what))
        return TablePolicy("q", src, eps, S)
    if eps != 0:
        raise ValueError("epsilon belongs to policy= and q=: a categorical table already says how it explores")
    return TablePolicy("thresholds", _tables.threshold_table(probs, logits, thresholds, temperature, S, 4, src.device, what), 0, S)


def _check_table(name, table, dev, keys=None):
    if not isinstance(table, TablePolicy):
        raise ValueError("%s must be a table_policy() record" % name)
    if table.device != dev:
        raise ValueError("%s's table must be on the rows' device" % name)
    if keys is not None and table.keys != keys:
        raise ValueError("%s has %d rows, values %d" % (name, table.keys, keys))


def action_probs(key_t, actions_t, table, out=None):
    """The probability with which `table` records actions_t at key_t, float32 shaped like key_t, in ONE launch (include/lmaze.h
    lmaze_action_probs); torch.log of it is the log-prob row the rollouts do not write.  key_t, actions_t: contiguous int32
    tensors of one shape on one GPU, the [T, N] rows of rollout_policy() / rollout_sample() or any slice that stays
    contiguous; table: a table_policy() record on that GPU.  p = fl(w) * 2**-34 with w the integer weight of the (key, action)
    pair under the rule the rollout runs: a key outside the table or an action the rule cannot record gives 0.  out: float32 of
    key_t's shape to fill; default a new tensor.  Returns it."""
    if not (isinstance(key_t, torch.Tensor) and key_t.dtype == torch.int32 and key_t.is_cuda and key_t.is_contiguous()):
        raise ValueError("key_t must be a contiguous int32 tensor on a GPU")
    dev = key_t.device

    def like(t, dtype):
        return (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.is_contiguous()
                and tuple(t.shape) == tuple(key_t.shape))
    if not like(actions_t, torch.int32):
        raise ValueError("actions_t must be a contiguous int32 tensor of key_t's shape, on its device")
    _check_table("table", table, dev)
    if out is None:
        out = torch.empty(key_t.shape, dtype=torch.float32, device=dev)
    elif not like(out, torch.float32):
        raise ValueError("out must be a contiguous float32 tensor of key_t's shape, on its device")
    m = key_t.numel()
    if m == 0:
        return out
    with torch.cuda.device(dev):
        rc = _abi.lib.lmaze_action_probs(key_t.data_ptr(), actions_t.data_ptr(), m, *table._law(), table.keys, out.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream)
    _abi.check("lmaze_action_probs", rc)
    return out


def vtrace(reward_t, done_t, gamma, lam=1.0, *, value_t=None, tail=None, rho_t=None, values=None, key_t=None, key_tail=None,
           actions_t=None, behaviour=None, target=None, rho_bar=1.0, c_bar=1.0, out=None, pg=True, ratios=False):
    """V-trace (Espeholt et al. 2018) over trajectory rows that another table produced, in ONE launch (include/lmaze.h
    lmaze_vtrace / lmaze_vtrace_table): walking t = T-1 .. 0 with v the value of the row, ratio its unclipped importance ratio,
    rho = min(ratio, rho_bar) and c = lam * min(ratio, c_bar),
        acc = rho * (r - v)                                                where done_t[t]
        acc = rho * ((r + gamma * v_next) - v) + (gamma * c) * acc_next    otherwise
        vs = acc + v;   pg_adv = rho * ((r, or r + gamma * vs_next) - v)
    in float32, every operation rounded on its own, so a float32 loop on the host gives the same bits; with ratio 1 and both
    bars >= 1 vs - v is gae()'s advantage and vs its target in every bit.  Exactly one value source, as gae():
    value_t         rows form: float32[T,N], tail float32[N] (default 0), and rho_t float32[T,N], the unclipped ratios the
                    caller computed (default: 1) -- also the way in for the 25-action foveal and hierarchical rows;
    values + key_t  table form: values float32[S], key_t and actions_t int32[T,N], key_tail int32[N] as gae()'s, and
                    behaviour= / target=, two table_policy() records of S rows each (the table the rollout ran and the one
                    being learnt; their forms need not match).  ratio = fl(fl(wt) / fl(wb)) of the pair's integer weights,
                    0 where the behaviour table cannot have produced the row; equal tables give exactly 1.
    out: float32[T,N] for vs_t (rows form: it may be value_t); default a new tensor.  pg: True allocates the policy-gradient
    advantages, a float32[T,N] tensor fills it (it may be reward_t), False skips them.  ratios (table form): the same for the
    unclipped ratio.  gamma, lam and the bars are not validated.  Returns (vs_t, pg_adv_t or None, rho_t or None)."""
    T, N, dev, table = _value_source("vtrace()", reward_t, done_t, value_t, tail, values, key_t, key_tail)
    if table:
        if rho_t is not None:
            raise ValueError("rho_t= belongs to the rows form; the table form takes behaviour= and target=")
        if not _rows_like(reward_t, actions_t, (torch.int32,)):
            raise ValueError("actions_t must be a contiguous int32 tensor of reward_t's shape, on its device")
        if behaviour is None or target is None:
            raise ValueError("the table form wants behaviour= and target=, two table_policy() records")
        _check_table("behaviour", behaviour, dev, values.numel())
        _check_table("target", target, dev, values.numel())
    else:
        if behaviour is not None or target is not None or actions_t is not None:
            raise ValueError("behaviour=, target= and actions_t= belong to the table form; the rows form takes rho_t=")
        if ratios is not False and ratios is not None:
            raise ValueError("ratios= belongs to the table form: the rows form is given its ratios")
        if rho_t is not None and not _rows_like(reward_t, rho_t, (torch.float32,)):
            raise ValueError("rho_t must be a contiguous float32 tensor of reward_t's shape, on its device")

    def rows(name, t, default):
        if t is True or (t is None and default):
            return torch.empty_like(reward_t)
        if t is False or t is None:
            return None
        if not _rows_like(reward_t, t, (torch.float32,)):
            raise ValueError("%s must be a contiguous float32 tensor of reward_t's shape, on its device" % name)
        return t
    out, pg, ratios = rows("out", out, True), rows("pg", pg, False), rows("ratios", ratios, False)
    given = [t for t in (out, pg, ratios) if t is not None]
    if len({t.data_ptr() for t in given}) != len(given) and T * N:
        raise ValueError("out, pg and ratios must be distinct tensors")
    if T == 0 or N == 0:          # nothing to do; an empty tensor has no address to pass
        return out, pg, ratios

    def ptr(t):
        return None if t is None else t.data_ptr()
    scalars = (float(gamma), float(lam), float(rho_bar), float(c_bar))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if table:
            name = "lmaze_vtrace_table"
            rc = _abi.lib.lmaze_vtrace_table(reward_t.data_ptr(), done_t.data_ptr(), key_t.data_ptr(), actions_t.data_ptr(),
                                             ptr(key_tail), values.data_ptr(), values.numel(), *behaviour._law(), *target._law(),
                                             *scalars, out.data_ptr(), ptr(pg), ptr(ratios), T, N, stream)
        else:
            name = "lmaze_vtrace"
            rc = _abi.lib.lmaze_vtrace(reward_t.data_ptr(), done_t.data_ptr(), value_t.data_ptr(), ptr(tail), ptr(rho_t), *scalars,
                                       out.data_ptr(), ptr(pg), T, N, stream)
    _abi.check(name, rc)
    return out, pg, ratios
