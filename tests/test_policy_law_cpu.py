"""CPU: what lmaze_evaluate weighs a table by (evaluate_ref.weights, the header's rule) against the exact action law of the
rules the rollouts run (policy_law.py: the draws counted through closed_loop_ref.sample_action and
env_table_ref.epsilon_greedy, the functions the GPU replays are held to bit for bit), and the two readings of a q row
(lmaze_q_first_max for evaluate(q=) / score(q=) / rollout_qlearn, greedy_table() for rollout_policy(q=)) against each other."""
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import evaluate_ref as E
import policy_law as L
import qlearn_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lm():
    lib = os.path.join(ROOT, "gym-lmaze_amd", "liblmaze_hip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gym-lmaze_amd", "csrc"), "-s"])
    return importlib.import_module("gym-lmaze_amd")


def non_monotone(rows):
    c = rows[:, :3].astype(np.int64)
    return (c[:, 1] < c[:, 0]) | (c[:, 2] < c[:, 1])


def mixed_table(abi):
    """uint32[n, 4] with a kind per row, and the kinds"""
    rs = np.random.RandomState(17)
    probs = rs.rand(600, 4)
    probs[200:400] *= rs.rand(200, 4) < 0.6                                   # zero entries
    probs[200:400, 1] += (probs[200:400].sum(1) == 0)                         # but no all-zero row: the converter refuses it
    assert (probs[200:400] == 0).any(1).sum() > 100
    probs[400:600] = np.eye(4)[rs.randint(0, 4, 200)]                         # one-hot
    conv = abi.sampling_thresholds(torch.from_numpy(probs)).view(torch.int32).numpy().view(np.uint32)
    raw = rs.randint(0, 1 << 32, (3000, 4), dtype=np.uint64).astype(np.uint32)
    ordered = raw[:1000].copy()
    ordered[:, :3] = np.sort(ordered[:, :3], axis=1)
    wild = raw[1000:]
    wild = wild[non_monotone(wild)]
    small = rs.randint(0, 4, (300, 4), dtype=np.uint64).astype(np.uint32)     # words that collide, in every order
    near = (TOP - rs.randint(0, 3, (300, 4), dtype=np.uint64)).astype(np.uint32)
    equal = np.repeat(rs.randint(0, 1 << 32, (100, 1), dtype=np.uint64).astype(np.uint32), 4, axis=1)
    pair = raw[:200].copy()
    pair[:100, 1] = pair[:100, 0]
    pair[100:, 2] = pair[100:, 0]
    corners = np.array(list(itertools.product((0, 1, 1 << 31, TOP - 1, TOP), repeat=3)), np.uint32)
    corners = np.concatenate([corners, np.zeros((len(corners), 1), np.uint32)], axis=1)
    fixed = np.array([[0, 0, 0, 0], [TOP, TOP, TOP, TOP], [10, 5, 20, 77], [0, TOP, 0, 5], [TOP, 0, TOP, 9]], np.uint32)
    kinds = dict(converter=conv, ordered=ordered, unsorted=wild, small=small, near_top=near, equal=equal, pair=pair, corners=corners,
                 fixed=fixed)
    table = np.concatenate(list(kinds.values()))
    table[:, 3] = rs.randint(0, 1 << 32, len(table), dtype=np.uint64).astype(np.uint32)      # word 3 is noise to both sides
    return table, kinds


def test_sampling_law_is_the_evaluated_weight(lm):
    table, kinds = mixed_table(lm._abi)
    assert len(kinds["unsorted"]) * 3 >= len(table) and non_monotone(table).sum() * 3 >= len(table)
    assert (table[:, :3] == 0).all(1).any() and (table[:, :3] == TOP).all(1).any()
    law = L.sampling_law(table)
    w = E.weights(thresholds=table)
    assert w.dtype == np.int64 and (w.sum(1) == E.FULL).all()
    bad = (4 * law != w).any(1)
    assert not bad.any(), (int(bad.sum()), table[bad][:5].tolist(), law[bad][:5].tolist(), w[bad][:5].tolist())
    assert (law[:, 3] >= 1).all() and (law[:, :3] == 0).any(0).all()          # 2^32 fits no word: action 3 keeps a draw
    # the same bits as int32, as the host wrappers hand them over
    assert (E.weights(thresholds=table.view(np.int32)) == w).all()


def test_reproduction_twenty_thousand_rows():
    """The rows of the report: every second row sorted.  The weights are the sampler's law on all of them; the inner
    differences mod 2^32 of the row as stored, which lmaze_evaluate took before, are its law on the monotone rows alone."""
    rows = np.random.RandomState(0).randint(0, 2 ** 32, (20000, 4)).astype(np.uint32)
    rows[::2, :3] = np.sort(rows[::2, :3], axis=1)
    law = L.sampling_law(rows)
    assert int((4 * law != E.weights(thresholds=rows)).any(1).sum()) == 0
    c = rows.astype(np.int64)
    before = 4 * np.stack([c[:, 0], (c[:, 1] - c[:, 0]) % L.TWO32, (c[:, 2] - c[:, 1]) % L.TWO32, L.TWO32 - c[:, 2]], -1)
    wrong = (4 * law != before).any(1)
    print("non-monotone rows", int(non_monotone(rows).sum()), "rows the former rule misweighs", int(wrong.sum()))
    assert (wrong == non_monotone(rows)).all() and int(wrong.sum()) == 8300
    assert set((before[wrong].sum(1) // E.FULL).tolist()) == {2, 3}


@pytest.mark.parametrize("e", [0, 1, (1 << 28) + 3, 1 << 31, (1 << 32) - 1])
def test_epsilon_greedy_law_is_the_evaluated_weight(e):
    entries = np.arange(4, dtype=np.uint8)
    law = L.epsilon_greedy_law(entries, e)
    assert (law[:, 4] == 0).all()
    assert (law[:, :4] == E.weights(policy=entries, epsilon_u32=e)).all(), (e, law.tolist())
    # a byte above 3: the exploring draws are weighed alike, the greedy share goes to no action on both sides
    above = np.array([4, 7, 200, 255], np.uint8)
    law = L.epsilon_greedy_law(above, e)
    w = E.weights(policy=above, epsilon_u32=e)
    assert (law[:, :4] == w).all() and (law[:, 4] == E.FULL - w.sum(1)).all() and (law[:, 4] == 4 * (L.TWO32 - e)).all()


def test_q_rows_first_max_against_greedy_table(lm):
    """All 2 401 rows over {-inf, -1, -0.0, 0.0, 1, inf, NaN}: without a NaN the two readings of a q row agree, so
    evaluate(q=) / score(q=) describe what rollout_policy(q=) runs; with a NaN, rollout_policy(q=) does not move (id 4) and
    the learner's rule still names an action -- there policy=greedy_table(q) is the table to evaluate or score."""
    vals = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], np.float32)
    q = np.array(list(itertools.product(vals, repeat=4)), np.float32)
    assert q.shape == (2401, 4)
    has_nan = np.isnan(q).any(1)
    assert int(has_nan.sum()) == 1105 and int((~has_nan).sum()) == 1296
    first = E.first_max(q)
    assert (first == QR.first_max(q)[1]).all()                                # evaluate_ref's and score_ref's are one rule
    table = lm.LmazeVecEnv.greedy_table(torch.from_numpy(q)).numpy()
    assert table.dtype == np.uint8
    assert (table[~has_nan] == first[~has_nan]).all()
    assert (table[has_nan] == 4).all() and (first[has_nan] <= 3).all()
    # so the laws coincide without a NaN, and through policy=greedy_table(q) everywhere
    for e in (0, (1 << 28) + 3):
        assert (E.weights(q=q[~has_nan], epsilon_u32=e) == E.weights(policy=table[~has_nan], epsilon_u32=e)).all()
        assert (L.epsilon_greedy_law(table, e)[:, :4] == E.weights(policy=table, epsilon_u32=e)).all()
