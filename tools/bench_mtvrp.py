"""Env-steps/s of the MTVRP env kernels on a nearest-feasible episode's actions over a mixed
batch (``variant_preset="all"``), three legs per size: ``co_mtvrp_steps`` (the T preset
steps in one launch), T single ``co_mtvrp_step`` launches through the C ABI (fresh output
tensors per step, as the env's ``step`` makes them), and the host build on the first 256
rows (one thread).  Device legs are timed with device events, the median of ``--reps`` runs
after a warm-up.  The three legs' final states are compared equal in the same run.  Prints
one JSON line (``--out FILE`` also writes it).
Usage: ``python tools/bench_mtvrp.py [--sizes 100:32768,20:65536] [--reps 5] [--out F]``."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import mtvrp_cases as mc  # noqa: E402
from rl4co_slap_amd.envs import MTVRPGenerator  # noqa: E402

HOST_ROWS = 256
KEYS = ("cur", "time", "length", "used_l", "used_b", "visited", "action_mask", "done")


def device_instance(n, b, dev):
    torch.manual_seed(100 + n)
    td = MTVRPGenerator(num_loc=n, variant_preset="all",
                        device=None if dev == "cpu" else dev)([b])
    return {k: td[k].contiguous() for k in mc.ref.INSTANCE}


def reset(inst, dev):
    """co_mtvrp_reset on tensors already on ``dev`` (mc.abi_reset takes numpy arrays)."""
    b, nc = inst["locs"].shape[:2]
    st = dict(inst, **mc.fresh_state(b, nc, dev),
              action_mask=torch.empty((b, nc), dtype=torch.bool, device=dev))
    table = mc.inst_table(st)
    mc.nat.call("co_mtvrp_reset", b, nc - 1, table.address, *mc.state_ptrs(st),
                mc.nat.ptr(st["action_mask"]), mc.nat.stream_of(st["locs"]))
    return st


def nearest_episode(start):
    """Actions [T, B] of the nearest-feasible policy (depot when nothing is feasible)."""
    st, acts = start, []
    rows = torch.arange(start["locs"].shape[0], device=start["locs"].device)
    while True:
        m = st["action_mask"]
        d = (st["locs"][rows, st["cur"]][:, None, :] - st["locs"]).norm(p=2, dim=-1)
        a = d.masked_fill(~m, float("inf")).argmin(1)
        a = torch.where(m.any(1), a, torch.zeros_like(a))
        st = mc.abi_step(st, a)
        acts.append(a)
        if bool(st["done"].all()) or len(acts) >= 4 * m.shape[1]:
            return torch.stack(acts), st


def timed_device(fn, reps, dev):
    out = None
    ms = []
    for r in range(reps + 1):  # the first run warms up
        if dev == "cpu":  # a dry run of this tool without a device: wall clock
            t0 = time.perf_counter()
            out = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
            continue
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms[1:]) * 1e-3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100:32768,20:65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = a.device
    out = {"bench": "mtvrp", "device": dev, "reps": a.reps, "host_rows": HOST_ROWS}
    for size in a.sizes.split(","):
        n, b = (int(x) for x in size.split(":"))
        start = reset(device_instance(n, b, dev), dev)
        acts, last = nearest_episode(start)
        t = acts.shape[0]
        tag = f"n{n}_b{b}"

        def fused():
            return mc.abi_steps(start, acts, want=False)[0]

        def single():
            st = start
            for x in acts:
                st = mc.abi_step(st, x)
            return st

        sec_f, got_f = timed_device(fused, a.reps, dev)
        sec_s, got_s = timed_device(single, a.reps, dev)
        rows = min(HOST_ROWS, b)
        host_start = {k: v[:rows].cpu().contiguous() for k, v in start.items()}
        host_acts = acts[:, :rows].cpu().contiguous()
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        got_h = mc.abi_steps(host_start, host_acts, want=False)[0]
        sec_h = time.perf_counter() - t0
        for key in KEYS:
            assert torch.equal(got_f[key], got_s[key]), (tag, key)
            assert torch.equal(got_f[key][:rows].cpu(), got_h[key]), (tag, key, "host")
        out[tag] = {"steps": t, "all_done": bool(last["done"].all()),
                    "steps_launch_steps_per_s": round(b * t / sec_f, 1),
                    "single_launches_steps_per_s": round(b * t / sec_s, 1),
                    "host_1thread_steps_per_s": round(rows * t / sec_h, 1),
                    "steps_launch_ms": round(sec_f * 1e3, 3),
                    "single_launches_ms": round(sec_s * 1e3, 3),
                    "final_states_equal": True}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
