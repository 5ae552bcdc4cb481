"""CPU: the inputs of the far-range tests of the v5 / v6 visit map (test_gpu_foveal_visit_range.py) are what those tests
need them to be -- asserted from the reference recording alone and, for the batched recipes, from the oracle alone, so that
the chosen seeds are checked wherever the suite runs."""
import numpy as np
import pytest

import foveal_visit_range as R
from helpers import load_golden

FIXTURE = "v5_noreset_deepdecay_seed7"


def test_noreset_deepdecay_fixture_reaches_the_far_range():
    g = load_golden(FIXTURE)
    ev, ld = np.asarray(g["ev_type"]), np.asarray(g["local_done"])
    assert ev[0] == 0 and (ev[1:] != 0).all() and set(ev[1:]) == {1, 2}      # one reset(), then plannerStep / step only
    assert not g["raised"].any()
    step = ev == 2
    updates = np.cumsum(step & (ld != 0))           # a step() that leaves localDone set has updated the map (v5:315-318)
    assert updates[-1] >= 500
    # the clock-equivalent count: 0 at the reset, back to 126 when a step finds it at 250 -- at least twice
    assert updates[-1] >= 250 + 124
    assert (g["layout_id"] == g["layout_id"][0]).all()                      # the single layout in force
    shown = R.decayed(g["fov_planes"][:, 2]).reshape(len(ev), -1)
    assert int((shown.any(axis=1) & step).sum()) >= 20
    # a shown cell that is exactly 0 now and was not at some earlier event
    visit = np.asarray(g["visit"])
    was = np.maximum.accumulate(visit, axis=0) > 0
    found = 0
    for t in np.flatnonzero(step):
        x, y = g["fovea0"][t]
        win = (slice(x - 2, x + 3), slice(y - 2, y + 3))
        assert (visit[t][win].view(np.uint32) == g["fov_planes"][t, 2].view(np.uint32)).all(), t
        found += int(((visit[t][win] == 0) & was[t][win]).sum())
    assert found >= 1
    # plane 6 never holds a decayed value under the reference's dynamics: the previous window was updated when it was set
    assert not R.decayed(g["fov_planes"][:, 6]).any()


@pytest.mark.parametrize("variant,G", [("v5", 18), ("v6", 18), ("v5", R.G_OFF)])
def test_hier_recipes_meet_their_input_conditions(variant, G):
    w, a, g = R.hier_case(variant, G)
    for _ in R.hier_steps(w, variant, a, g):
        pass
    c = w.check_common()
    assert c["decayed6"] == 0                        # as in the recording: case (e) is what reaches plane 6
    assert len(set(np.flatnonzero(w.renorms > 0) // 32)) > 1


def test_noreset_recipe_meets_its_input_conditions():
    w, a, g = R.noreset_case()
    all_updated = True
    for t, m, gt, at in R.noreset_steps(w, a, g):
        if t >= R.T_NORESET - 100:
            all_updated &= bool(w.st.foveal_done.all())
    R.check_noreset(w, all_updated)


def test_rollout_recipe_renormalises_inside_the_recorded_call():
    w, a, g = R.hier_case("v5", 18)
    n = sum(1 for _ in R.rollout_calls(w, a, g))     # asserts MIN_RENORM_IN_REC_CALL itself
    assert n == 9 > R.REC_CALL
    w.check_common()


def test_restore_recipe_shows_decayed_cells_in_the_previous_window():
    w, a, g, pointed = R.restore_case()
    assert len(pointed) >= R.MIN_POINTED
    for t, at, gt, epoch in R.restore_steps(w, a[:1], g[:1]):
        assert int(R.decayed(w.st.obs[:, 6]).sum()) >= 1
