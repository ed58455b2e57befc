"""bench.py's plain run and --dump-outputs: a plain run reports the headline only (the mode
tables, the copy probe and the CPU baselines sit behind --full), --steps sets the timed
steps, and the dumped arrays are the fused episode's outputs for the batch the last timed
step ran -- checked against the tour lengths computed here from the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_full_and_dump_options_parse(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_full_legs_do_not_grow_with_a_large_steps(monkeypatch):
    """--steps is sized for the microsecond headline launch; the --full legs' episode count
    follows it (a fifth, at least 3) only up to the cap, unless --mode-steps sets it."""
    def k(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--full"] + list(argv))
        return bench.mode_steps(bench.parse())

    assert k() == 10 and k("--steps", "50") == 10 and k("--steps", "5") == 3
    assert k("--steps", "100") == 20 == bench.FULL_STEPS_CAP // 5
    assert k("--steps", "100000") == 20
    assert k("--steps", "100000", "--mode-steps", "7") == 7


def test_dump_outputs_dtypes_and_sample(tmp_path, monkeypatch):
    b = 50
    arrays = {"reward": torch.arange(b, dtype=torch.float32),
              "action_mask": torch.zeros(b, 7, dtype=torch.bool),
              "i": torch.arange(b, dtype=torch.int64).unsqueeze(1) + (1 << 40)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["action_mask", "i", "reward"]
    assert got["reward"].dtype == np.float32 and got["action_mask"].dtype == np.float32
    assert got["i"].dtype == np.float64 and got["i"].shape == (b, 1)
    assert (got["i"][:, 0] == np.arange(b) + float(1 << 40)).all()
    # over the limit: the same seeded rows of every array, within the limit, twice the same
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    s1 = {f[:-4]: np.load(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")}
    s2 = {f[:-4]: np.load(tmp_path / "s2" / f) for f in os.listdir(tmp_path / "s2")}
    assert sorted(s1) == ["action_mask", "i", "reward", "rows"]
    assert sum(v.nbytes for v in s1.values()) <= 1000
    rows = s1["rows"].astype(np.int64)
    assert 0 < len(rows) < b and (np.diff(rows) > 0).all()
    assert (s1["reward"] == rows).all() and (s1["i"][:, 0] == rows + float(1 << 40)).all()
    assert all((s1[k] == s2[k]).all() for k in s1)


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_last_step(dev, tmp_path):
    b, n, steps, warmup = 1024, 20, 3, 2
    out = tmp_path / "o"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", str(warmup), "--batch", str(b), "--num-loc", str(n),
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["steps"] == steps and j["warmup"] == warmup and j["n_gpus"] == 1
    assert j["unit"] == "env-steps/s" and j["higher_is_better"] is True and j["dtype"] == "u8+i64+f32"
    assert j["ms_per_step"] > 0
    assert abs(j["value"] - b * n / (j["ms_per_step"] * 1e-3)) <= 1e-6 * j["value"]
    for key in ("modes", "tsp_stepwise", "tsp_stepwise_chunked", "slap_b65536", "cpu_baseline",
                "step_kernels_vs_copy"):
        assert key not in j
    assert "copy_probe" not in j["roofline"]
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(got) == ["action_mask", "current_node", "done", "first_node", "i", "reward"]
    assert all(v.dtype in (np.float32, np.float64) and v.shape[0] == b for v in got.values())
    # the batch the last timed step ran: the bench cycles its seeded batches in order
    salt = (warmup + steps - 1) % j["config"]["input_batches_cycled"]
    locs, acts = bench.tsp_inputs(b, n, 0, salt=salt)
    tour = locs.double().gather(1, acts.unsqueeze(-1).expand(-1, -1, 2))
    length = (tour - tour.roll(-1, 1)).norm(dim=-1).sum(1).numpy()
    # float32 against float64: every edge length carries about 4 roundings (the differences,
    # the sum of squares, the root) and the running sum n more, each at most 2^-24 of a
    # value no larger than the tour length: (n + 4) * 2^-24 * length, doubled for slack
    err = np.abs(got["reward"].astype(np.float64) + length)
    assert (err <= (n + 4) * 2.0 ** -23 * length).all(), err.max()
    assert (got["action_mask"] == 0).all() and (got["done"] == 1).all()
    assert (got["i"] == n).all()
    assert (got["first_node"] == acts[:, 0].numpy()).all()
    assert (got["current_node"] == acts[:, -1].numpy()).all()
