"""The K-steps-per-launch entries co_tsp_steps (csrc/tsp.hip) and co_slap_closest_steps
(csrc/slap.hip) on the device, on every dispatch path: direct C-ABI calls on guarded,
pre-filled buffers with arbitrary (not policy-reachable) states, every buffer bit for bit
against K applications of the oracle's step (and, for SLAP, its closest-free action), the
status bit raised by one bad row alone, and one call per documented rejection.  The cases,
the references and the map from template instantiation to case id are in
tests/steps_cases.py."""
import pytest

import steps_cases as kc

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ TSP
@pytest.mark.parametrize("case", kc.TSP_STEPS_CASES, ids=kc.tsp_steps_id)
def test_tsp_steps(dev, case):
    kc.check_tsp_steps(dev, case)


@pytest.mark.parametrize("which", list(kc.TSP_BAD))
@pytest.mark.parametrize("path", list(kc.TSP_STATUS_N))
def test_tsp_steps_status(dev, path, which):
    kc.check_tsp_steps_status(dev, path, which)


# ----------------------------------------------------------------------------- SLAP
@pytest.mark.parametrize("case", kc.SLAP_STEPS_CASES, ids=kc.slap_steps_id)
def test_slap_steps(dev, case):
    kc.check_slap_steps(dev, case)


@pytest.mark.parametrize("inplace", [True, False], ids=["ip", "oop"])
@pytest.mark.parametrize("l", kc.SLAP_SPECIAL_L, ids=lambda v: f"L{v}")
def test_slap_steps_special(dev, l, inplace):
    kc.check_slap_steps_special(dev, l, inplace)


@pytest.mark.parametrize("inplace", [True, False], ids=["ip", "oop"])
@pytest.mark.parametrize("step", kc.SLAP_STATUS_STEPS, ids=lambda v: f"t{v}")
@pytest.mark.parametrize("path", list(kc.SLAP_STATUS_L))
def test_slap_steps_status(dev, path, step, inplace):
    kc.check_slap_steps_status(dev, path, step, inplace)


# ----------------------------------------------------------------------- rejections
@pytest.mark.parametrize("name", list(kc.STEPS_REJECTIONS))
def test_steps_rejections(dev, name):
    kc.check_steps_rejections(dev, name)
