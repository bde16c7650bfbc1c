"""The merge model's own pin (no GPU).  On the 64 x 48 noise map the model's R'
and rounds are pinned to the figures it gave when the definition was fixed
(from R = 809: 486 in 1 round, 104 in 2, 1 in 4, 570 in 4, 315 in 5, 809 in
0), so a weakened model cannot pass."""
from merge_model import NONE, merge_model
from region_inputs import merge_inputs

ALL = 1 << 31                  # min_area above every area: everything is restless
PINNED = {(2, NONE): (486, 1), (10, NONE): (104, 2), (ALL, NONE): (1, 4), (10, 20000): (570, 4),
          (ALL, 30000): (315, 5), (ALL, 0): (809, 0)}


def _reference(name, min_area, max_dist=NONE, max_rounds=0):
    i = merge_inputs(name)
    return merge_model(i["regions"], i["area"], i["first"], i["sums"], i["bbox"], i["edges"], min_area, max_dist,
                       max_rounds)


def test_the_model_reproduces_the_pinned_figures():
    assert merge_inputs("noise64x48")["R"] == 809
    for params, figures in PINNED.items():
        want = _reference("noise64x48", *params)
        assert (want["R"], want["rounds"]) == figures, params
