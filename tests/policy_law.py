"""The exact action law of the rules the closed-loop rollouts run: how many of the 2^32 draws r.x (sampling) or of the 2^64
draws (r.x, r.y) (epsilon-greedy) give each action.  Nothing is restated here: the counts come from calling the restated rules
the GPU replays are pinned to bit for bit -- closed_loop_ref.sample_action and env_table_ref.epsilon_greedy -- at both ends of
every block of draws on which they can only be constant, asserting that they are, and adding the blocks' sizes.  This is what
evaluate_ref.weights (and with it lmaze_evaluate) claims to weigh a table by.  Importing it needs no GPU."""
import numpy as np

from closed_loop_ref import sample_action
from env_table_ref import epsilon_greedy

TWO30 = 1 << 30
TWO32 = 1 << 32


def sampling_law(rows):
    """int64[n, 4]: of the 2^32 values of r, how many give action 0..3 on each row of a uint32 (or int32 bits) [n, 4] table.
    The rule is a sum of three steps in r, each at one of the row's words, so it is non-decreasing in r and constant between
    two neighbouring breakpoints of {0, c0, c1, c2, 2^32} exactly when it agrees at the two ends: that is asserted, interval
    by interval.  Every row sums to 2^32."""
    rows = np.ascontiguousarray(rows).reshape(-1, 4).view(np.uint32)
    n = len(rows)
    c = rows[:, :3].astype(np.int64)
    bp = np.sort(np.concatenate([np.zeros((n, 1), np.int64), c, np.full((n, 1), TWO32, np.int64)], axis=1), axis=1)
    law = np.zeros((n, 4), np.int64)
    for i in range(4):
        lo, hi = bp[:, i], bp[:, i + 1]
        live = np.flatnonzero(hi > lo)
        first = sample_action(rows[live], lo[live].astype(np.uint64))
        last = sample_action(rows[live], (hi[live] - 1).astype(np.uint64))
        assert (first == last).all(), "the sampling rule changes inside an interval of its own breakpoints"
        assert ((first >= 0) & (first <= 3)).all()
        np.add.at(law, (live, first), hi[live] - lo[live])
    assert (law.sum(1) == TWO32).all()
    return law


def epsilon_greedy_law(entries, eps32):
    """int64[n, 5] in units of 2^-34: of the 2^64 draws (r.x, r.y), how many 2^30-blocks give action 0..3 on each table entry
    (uint8[n]); column 4 counts the draws that leave an entry above 3 standing, "no move".  The blocks are r.x in [0, e) and
    [e, 2^32) times r.y in [k 2^30, (k + 1) 2^30): the rule compares r.x with e and reads the top two bits of r.y, so it is
    constant on a block exactly when it agrees at the block's four corners, which is asserted.  Every entry sums to 2^34."""
    entries = np.asarray(entries, np.uint8).reshape(-1)
    e = int(eps32)
    assert 0 <= e < TWO32
    n = len(entries)
    law = np.zeros((n, 5), np.int64)
    who = np.arange(n)
    for x_lo, x_hi in ((0, e), (e, TWO32)):
        if x_hi == x_lo:
            continue
        for k in range(4):
            y_lo, y_hi = k * TWO30, (k + 1) * TWO30
            corners = [epsilon_greedy(entries, e, np.full(n, x, np.uint64), np.full(n, y, np.uint64))[0]
                       for x in (x_lo, x_hi - 1) for y in (y_lo, y_hi - 1)]
            for other in corners[1:]:
                assert (other == corners[0]).all(), "the epsilon-greedy rule changes inside a block"
            np.add.at(law, (who, np.minimum(corners[0], 4)), (x_hi - x_lo) * ((y_hi - y_lo) // TWO30))
    assert (law.sum(1) == 1 << 34).all()
    return law
