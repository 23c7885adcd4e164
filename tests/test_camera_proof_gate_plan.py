"""Host only: the camera miss proof gate's A/B knob (DESIGN.md §5 "Proof gate") as the launch plan
reads it.  rrt_plan_prove_first() runs the plan's own reading of the environment (rrt_host.cpp
read_ab_knobs -> plan_prove_first, the value plan_launch stores in KParams::prove_first), so the
default and the parsing checked here are the ones a launch gets."""
import os

import pytest

import rrt

KNOB = "RRT_AB_PROVE_FIRST"


@pytest.fixture
def planned():
    saved = os.environ.pop(KNOB, None)

    def at(value):
        if value is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = value
        return rrt.lib().rrt_plan_prove_first()

    yield at
    os.environ.pop(KNOB, None)
    if saved is not None:
        os.environ[KNOB] = saved


def test_default_gates_by_hypothesis(planned):
    assert planned(None) == 0


@pytest.mark.parametrize("text, want", [("0", 0), ("1", 1), ("2", 1), ("", 0), ("x", 0), ("00", 0), ("7", 1)])
def test_value_reaches_the_plan(planned, text, want):
    """0 (and text that is no number): by hypothesis; any other number: the batch kernels prove every ray first"""
    assert planned(text) == want


def test_read_anew_every_time(planned):
    assert [planned(v) for v in ("1", None, "1", "0", "1")] == [1, 0, 1, 0, 1]
