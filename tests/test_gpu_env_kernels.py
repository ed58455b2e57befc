"""The stepwise env kernels and the bench-policy kernels of csrc/cvrp.hip, csrc/slap.hip and
csrc/tsp.hip on the device, at every dispatch edge: direct C-ABI calls on guarded, pre-filled
buffers with arbitrary (not policy-reachable) states, state and actions bit for bit against
the oracle, rewards against the oracle and against float64 beside the derived bounds, status
bits on every kernel, and one call per documented rejection.  The cases, the references and
the map from template instantiation to case id are in tests/env_step_cases.py."""
import pytest

import env_step_cases as sc

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- CVRP
@pytest.mark.parametrize("case", sc.CVRP_STEP_CASES, ids=sc.cvrp_step_id)
def test_cvrp_step(dev, case):
    sc.check_cvrp_step(dev, case)


@pytest.mark.parametrize("hi", [True, False], ids=["hi", "lo"])
@pytest.mark.parametrize("path", list(sc.CVRP_STATUS_SHAPES))
def test_cvrp_step_status(dev, path, hi):
    sc.check_cvrp_step_status(dev, path, hi)


@pytest.mark.parametrize("off", [0, 4], ids=["off0", "off4"])
@pytest.mark.parametrize("kind", ["grid", "uniform"])
@pytest.mark.parametrize("nc", [32, 33, 64, 65, 112, 113, 128, 129], ids=lambda v: f"NC{v}")
def test_cvrp_nearest_step(dev, nc, kind, off):
    for b in (1, 15, 16, 17):
        sc.check_cvrp_nearest_step(dev, nc - 1, b, kind, off, inplace=(b % 2 == 0), count=(b > 15))


@pytest.mark.parametrize("kind", ["grid", "uniform"])
@pytest.mark.parametrize("n", [1, 64, 65, 160, 161, 320, 321], ids=lambda v: f"N{v}")
def test_cvrp_nearest_action(dev, n, kind):
    # 13 rows: the last lane group of 8, 4 and 2 rows per wave is partial; one row per wave
    # for N > 320, where 13 rows leave the last workgroup partial
    for b, off in ((13, 0), (1, 3)):
        sc.check_cvrp_nearest_action(dev, n, b, kind, off)


@pytest.mark.parametrize("b,n,off", [(1, 1, 0), (7, 5, 1), (33, 77, 3), (5, 130, 0), (32771, 2, 0)],
                         ids=lambda v: str(v))
def test_cvrp_action_mask(dev, b, n, off):
    sc.check_cvrp_action_mask(dev, n, b, off)


@pytest.mark.parametrize("b,n,off,vcap", [(1, 1, 0, 1.0), (7, 5, 1, 0.77), (33, 77, 3, 0.77),
                                          (5, 130, 0, 1.0), (32771, 1, 0, 0.77)],
                         ids=lambda v: str(v))
def test_cvrp_reset(dev, b, n, off, vcap):
    sc.check_cvrp_reset(dev, n, b, off, vcap)


@pytest.mark.parametrize("case", sc.CVRP_REWARD_CASES, ids=sc.cvrp_reward_id)
def test_cvrp_reward(dev, case):
    sc.check_cvrp_reward(dev, case)


@pytest.mark.parametrize("which", sc.CVRP_DIRTY)
@pytest.mark.parametrize("case", [c for c in sc.CVRP_REWARD_CASES if c.check and c.b >= 3 and c.t < 3000],
                         ids=sc.cvrp_reward_id)
def test_cvrp_reward_status(dev, case, which):
    sc.check_cvrp_reward_status(dev, case, which)


# ----------------------------------------------------------------------------- SLAP
@pytest.mark.parametrize("case", sc.SLAP_STEP_CASES, ids=sc.slap_step_id)
def test_slap_step(dev, case):
    sc.check_slap_step(dev, case)


@pytest.mark.parametrize("case", sc.SLAP_CASES, ids=sc.slap_closest_id)
def test_slap_closest_step(dev, case):
    sc.check_slap_closest_step(dev, case)


@pytest.mark.parametrize("kind", ["ties", "grid"])
@pytest.mark.parametrize("l", [1, 4, 63, 64, 65, 260], ids=lambda v: f"L{v}")
def test_slap_closest_action(dev, l, kind):
    for b, mask_off, dist_off in ((17, 0, 0), (1, 1, 4)):
        sc.check_slap_closest_action(dev, l, b, kind, mask_off, dist_off)


@pytest.mark.parametrize("which", sc.SLAP_STATUS_WHICH)
@pytest.mark.parametrize("shape", list(sc.SLAP_STATUS_SHAPES))
def test_slap_step_status(dev, shape, which):
    sc.check_slap_step_status(dev, shape, which)
    if which.startswith("product"):
        sc.check_slap_step_status(dev, shape, which, closest=True)


@pytest.mark.parametrize("b,l,p,off,full", [(1, 1, 1, 0, True), (7, 5, 3, 1, True), (33, 100, 20, 0, True),
                                            (1000, 4, 3, 3, False), (4099, 4100, 1, 0, False)],
                         ids=lambda v: str(v))
def test_slap_reset(dev, b, l, p, off, full):
    sc.check_slap_reset(dev, b, l, p, off, full)


@pytest.mark.parametrize("case", sc.SLAP_REWARD_CASES, ids=sc.slap_reward_id)
def test_slap_reward(dev, case):
    sc.check_slap_reward(dev, case)


@pytest.mark.parametrize("which", sc.SLAP_REWARD_WHICH)
@pytest.mark.parametrize("path", list(sc.SLAP_REWARD_STATUS_SHAPES))
def test_slap_reward_status(dev, path, which):
    sc.check_slap_reward_status(dev, path, which)


# ------------------------------------------------------------------------------ TSP
@pytest.mark.parametrize("b,n,alias", [(1, 1, False), (7, 5, True), (33, 77, False), (1048581, 1, True)],
                         ids=lambda v: str(v))
def test_tsp_reset(dev, b, n, alias):
    sc.check_tsp_reset(dev, b, n, alias)


@pytest.mark.parametrize("first_step", [0, 1], ids=["later", "first"])
@pytest.mark.parametrize("kind", ["grid", "uniform"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257], ids=lambda v: f"N{v}")
def test_tsp_nearest_action(dev, n, kind, first_step):
    for b in (1, 13):
        sc.check_tsp_nearest_action(dev, n, b, kind, first_step)
    if first_step:
        sc.check_tsp_nearest_action(dev, n, 5, kind, 1, nulls=True)


@pytest.mark.parametrize("case", sc.TSP_REWARD_CASES, ids=sc.tsp_reward_id)
def test_tsp_reward_generic(dev, case):
    sc.check_tsp_reward_generic(dev, case)


# ----------------------------------------------------------------------- rejections
@pytest.mark.parametrize("name", list(sc.REJECTIONS))
def test_rejections(dev, name):
    sc.check_rejections(dev, name)
