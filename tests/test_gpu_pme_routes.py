"""The routes of the calculator's autograd node, pinned: for a dozen cases of ``tools/trace_pme_routes.py`` the sequence of
launch labels (what ``ops.PROFILE`` would collect) of a first and a second evaluation, and which outputs of ``node.tail`` are
set.  The expected values were recorded from the commit BEFORE the node was split into a route decision and launch helpers
(the tool's trace of that commit is ``profiles/pme_function_trace.txt``): whoever adds the next route changes them on purpose.
The 343-atom box of ``tests/test_gpu_contract.py::setup``: bricks, planes and the gather tail are all reached."""

import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import trace_pme_routes as T  # noqa: E402

TAIL = ("energy", "grad")
DIRECT = ["kspace_forward", "forces_finalize"]  # the gather tail + weighted_sum's direct node
GENERAL = ["kspace_backward", "rspace_backward"]  # the general adjoints of the mesh part and of the fused pair kernel
TWO_CHANNELS = ["pair_distance_forward", "kspace_forward", "rspace_forward", "energy_sum", "energy_sum_backward",
                "kspace_backward", "rspace_backward", "pair_distance_backward"]
UNFUSED = ["kspace_forward", "rspace_forward", "energy_sum", "forces_finalize"]  # pair sum in a launch of its own, no tail

#: case -> (labels of either evaluation, set outputs of node.tail or None, slab_in_tail)
EXPECTED = {
    "base": (DIRECT, TAIL, False),
    "fp64": (DIRECT, TAIL, False),
    "no_mesh": (["rspace_forward", "energy_sum", "forces_finalize"], None, False),
    "two_channels": (TWO_CHANNELS, None, False),
    "mask": (UNFUSED, None, False),
    "slab": (DIRECT, TAIL, True),
    "slab_two_channels": (TWO_CHANNELS[:2] + ["slab_forward"] + TWO_CHANNELS[2:6] + ["slab_backward"] + TWO_CHANNELS[6:],
                          None, False),
    "reduce_random": (["kspace_forward", "scaled_match"] + GENERAL, TAIL, False),
    "grads_all": (DIRECT, ("G_deriv", "cell_work", "energy", "grad", "grad_cell", "grad_q"), False),
    "no_coschedule": (UNFUSED, None, False),
    "no_tail_fusion": (["kspace_forward", "energy_sum", "forces_finalize"], None, False),
    "no_energy_fast_path": (["kspace_forward", "energy_sum", "energy_sum_backward"] + GENERAL, None, False),
}


@pytest.mark.parametrize("name", list(EXPECTED))
def test_route_is_the_recorded_one(name):
    labels, tail, slab_in_tail = EXPECTED[name]
    _, got_labels, facts = T.run_case(name)
    assert got_labels == [labels, labels], got_labels
    for f in facts:
        assert f["tail"] == tail and f["slab_in_tail"] == slab_in_tail, f
