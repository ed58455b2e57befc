"""The PDP kernels' two measurements, per size (``--sizes 100:32768,100:1024``):

* env-steps/s of a whole random-feasible episode (N + 1 steps): ``co_pdp_steps`` (one launch),
  against N + 1 single ``co_pdp_step`` launches through the C ABI (fresh output tensors per
  step, as the env's ``step`` makes them), and against the host build on the first 256 rows
  (one thread, the median of three calls after a first one).  The three legs' final states
  are compared equal in the same run.
* us per step of ``co_pdp_decode_step`` (greedy, certified, clip 10) against the pair it
  replaces, ``co_decode_step`` + ``co_pdp_step``, on a mid-episode state, outputs
  preallocated; the two sides' outputs are compared equal.

Device legs are timed with device events around ``--inner`` back-to-back calls after a
warm-up; the sides of a comparison alternate window by window in this one process and the
median window of ``--reps`` is reported.  ``bytes_per_row_step`` is the header's arithmetic
(include/co_env.h) and ``tb_per_s`` what that traffic amounts to over the measured time,
against the 8 TB/s of HBM.  Prints one JSON line (``--out FILE`` also writes it).
Usage: ``python tools/bench_pdp.py [--sizes 100:32768,100:1024] [--reps 7] [--out F]``."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import torch  # noqa: E402

from rl4co_slap_amd import _native as nat  # noqa: E402

HOST_ROWS = 256
HBM_TB_PER_S = 8.0
STATE = ("available", "to_deliver", "action_mask", "i", "current_node", "done", "reward")


def reset(n, b, dev):
    g = torch.Generator().manual_seed(100 + n)
    depot, locs = torch.rand(b, 2, generator=g).to(dev), torch.rand(b, n, 2, generator=g).to(dev)
    e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    st = {"locs": e((b, n + 1, 2), torch.float32), "available": e((b, n + 1), torch.bool),
          "to_deliver": e((b, n + 1), torch.bool), "action_mask": e((b, n + 1), torch.bool),
          "current_node": e((b, 1), torch.int64), "i": e((b, 1), torch.int64),
          "done": e((b, 1), torch.bool), "terminated": e((b, 1), torch.bool)}
    nat.call("co_pdp_reset", b, n, nat.ptr(depot), nat.ptr(locs),
             *(nat.ptr(st[k]) for k in ("locs", "available", "to_deliver", "action_mask",
                                        "current_node", "i", "done", "terminated")),
             nat.stream_of(locs))
    return st


def step(st, action):
    """co_pdp_step into fresh tensors."""
    b, nc = st["available"].shape
    dev = action.device
    e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    out = {"available": e((b, nc), torch.bool), "to_deliver": e((b, nc), torch.bool),
           "action_mask": e((b, nc), torch.bool), "i": e((b, 1), torch.int64),
           "current_node": e((b, 1), torch.int64), "done": e((b,), torch.bool),
           "reward": e((b,), torch.bool)}
    nat.call("co_pdp_step", b, nc - 1, nat.ptr(action), nat.ptr(st["available"]),
             nat.ptr(st["to_deliver"]), nat.ptr(out["available"]), nat.ptr(out["to_deliver"]),
             nat.ptr(out["action_mask"]), nat.ptr(st["i"]), nat.ptr(out["i"]),
             nat.ptr(out["current_node"]), nat.ptr(out["done"]), nat.ptr(out["reward"]), None,
             nat.stream_of(action))
    return out


def steps(st, acts):
    """co_pdp_steps on copies of the state, feasible included."""
    t, b = acts.shape
    nc = st["available"].shape[1]
    dev = acts.device
    e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    out = {"available": st["available"].clone(), "to_deliver": st["to_deliver"].clone(),
           "i": st["i"].clone(), "action_mask": e((b, nc), torch.bool),
           "current_node": e((b, 1), torch.int64), "done": e((b,), torch.bool),
           "reward": e((b,), torch.bool), "feasible": e((t, b), torch.bool)}
    nat.call("co_pdp_steps", b, nc - 1, t, nat.ptr(acts), acts.stride(0), acts.stride(1),
             nat.ptr(st["action_mask"]), nat.ptr(out["available"]), nat.ptr(out["to_deliver"]),
             nat.ptr(out["action_mask"]), nat.ptr(out["i"]), nat.ptr(out["current_node"]),
             nat.ptr(out["done"]), nat.ptr(out["reward"]), nat.ptr(out["feasible"]), None,
             nat.stream_of(acts))
    return out


def random_episode(start, seed):
    """Actions [T, B] of a random-feasible episode, and the state after every step."""
    g = torch.Generator(device=start["available"].device).manual_seed(seed)
    st, acts, states = start, [], [start]
    while not bool(st["done"].all()):
        m = st["action_mask"]
        score = torch.rand(m.shape, generator=g, device=m.device).masked_fill(~m, -1.0)
        a = score.argmax(1)
        st = step(st, a)
        acts.append(a)
        states.append(st)
    return torch.stack(acts), states


def window(fn, inner, dev):
    """Seconds per call over ``inner`` back-to-back calls."""
    if dev == "cpu":  # a dry run of this tool without a device: wall clock
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        return (time.perf_counter() - t0) / inner
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def interleaved(sides, reps, inner, dev):
    """{name: median seconds per call}: the sides alternate window by window."""
    for fn in sides.values():  # warm-up: code objects, the allocator's blocks
        window(fn, 2, dev)
    took = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            took[k].append(window(fn, inner, dev))
    return {k: statistics.median(v) for k, v in took.items()}


def decode_sides(st, dev, clip=10.0, temp=1.0):
    """The fused call and the pair on the same mid-episode state, outputs preallocated."""
    b, nc = st["available"].shape
    logits = (torch.randn(b, nc, generator=torch.Generator().manual_seed(5)) * 3).to(dev)
    word = nat.DECODE_CERTIFIED  # greedy | certified
    s = nat.stream_of(logits)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def outputs():
        e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
        return {"action": e((b,), torch.int64), "logp": e((b,), torch.float32),
                "available": e((b, nc), torch.bool), "to_deliver": e((b, nc), torch.bool),
                "action_mask": e((b, nc), torch.bool), "i": e((b, 1), torch.int64),
                "current_node": e((b, 1), torch.int64), "done": e((b,), torch.bool),
                "reward": e((b,), torch.bool)}

    of, op = outputs(), outputs()

    def env_args(o):
        return ([nat.ptr(o[k]) for k in ("available", "to_deliver", "action_mask")]
                + [nat.ptr(st["i"]), nat.ptr(o["i"]), nat.ptr(o["current_node"]),
                   nat.ptr(o["done"]), nat.ptr(o["reward"])])

    def fused():
        nat.call("co_pdp_decode_step", b, nc - 1, nat.ptr(logits), logits.stride(0),
                 nat.ptr(st["action_mask"]), clip, temp, word, None, nat.ptr(of["action"]),
                 nat.ptr(of["logp"]), 0, 0, nat.ptr(st["available"]), nat.ptr(st["to_deliver"]),
                 *env_args(of), None, nat.ptr(status), s)

    def pair():
        nat.call("co_decode_step", b, nc, nat.ptr(logits), logits.stride(0),
                 nat.ptr(st["action_mask"]), clip, temp, word, None, nat.ptr(op["action"]),
                 nat.ptr(op["logp"]), None, 0, 0, nat.ptr(status), s)
        nat.call("co_pdp_step", b, nc - 1, nat.ptr(op["action"]), nat.ptr(st["available"]),
                 nat.ptr(st["to_deliver"]), *env_args(op), nat.ptr(status), s)

    return {"fused": fused, "pair": pair}, of, op, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100:32768,100:1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = a.device
    if dev != "cpu" and not torch.cuda.is_available():
        raise SystemExit("bench_pdp: no GPU (pass --device cpu for a dry run of the host path)")
    out = {"bench": "pdp", "device": dev, "reps": a.reps, "inner": a.inner,
           "host_rows": HOST_ROWS, "hbm_tb_per_s": HBM_TB_PER_S}
    for size in a.sizes.split(","):
        n, b = (int(x) for x in size.split(":"))
        nc = n + 1
        start = reset(n, b, dev)
        acts, states = random_episode(start, 7 + n)
        t = acts.shape[0]
        assert t == nc
        got = {}

        def launch_steps():
            got["steps"] = steps(start, acts)

        def launch_single():
            st = start
            for x in acts:
                st = step(st, x)
            got["single"] = st

        sec = interleaved({"steps": launch_steps, "single": launch_single}, a.reps,
                          max(1, a.inner // 10), dev)
        rows = min(HOST_ROWS, b)
        host_start = {k: v[:rows].cpu().contiguous() for k, v in start.items()}
        host_acts = acts[:, :rows].cpu().contiguous()
        torch.set_num_threads(1)
        host_s = []
        for _ in range(4):  # the first call loads the host library
            t0 = time.perf_counter()
            got_h = steps(host_start, host_acts)
            host_s.append(time.perf_counter() - t0)
        sec_h = statistics.median(host_s[1:])
        assert bool(got["steps"]["feasible"].all())
        for key in STATE:
            assert torch.equal(got["steps"][key], got["single"][key]), (size, key)
            assert torch.equal(got["steps"][key][:rows].cpu(), got_h[key]), (size, key, "host")
        dsec = None
        if dev != "cpu":  # the fused decode step has no host build
            sides, of, op, status = decode_sides(states[t // 2], dev)
            dsec = interleaved(sides, a.reps, a.inner, dev)
            assert int(status.item()) == 0
            for key in of:
                assert torch.equal(of[key], op[key]), (size, key, "fused decode vs the pair")
        steps_bytes = 9 + (5 * nc + 27) / t  # per row-step: the action, feasible; rows once
        decode_bytes = 10 * nc + 38
        out[f"n{n}_b{b}"] = {
            "steps": t,
            "steps_launch_steps_per_s": round(b * t / sec["steps"], 1),
            "single_launches_steps_per_s": round(b * t / sec["single"], 1),
            "host_1thread_steps_per_s": round(rows * t / sec_h, 1),
            "steps_launch_ms": round(sec["steps"] * 1e3, 4),
            "single_launches_ms": round(sec["single"] * 1e3, 4),
            "final_states_equal": True,
            "steps_bytes_per_row_step": round(steps_bytes, 2),
            "steps_tb_per_s": round(steps_bytes * b * t / sec["steps"] / 1e12, 4),
            "single_step_bytes_per_row_step": 5 * nc + 34,
            "single_step_tb_per_s": round((5 * nc + 34) * b * t / sec["single"] / 1e12, 4),
            "decode_bytes_per_row_step": decode_bytes}
        if dsec is not None:
            out[f"n{n}_b{b}"].update({
                "decode_fused_us_per_step": round(dsec["fused"] * 1e6, 3),
                "decode_pair_us_per_step": round(dsec["pair"] * 1e6, 3),
                "decode_outputs_equal": True,
                "decode_fused_tb_per_s": round(decode_bytes * b / dsec["fused"] / 1e12, 4),
                "fused_not_above_pair": dsec["fused"] <= dsec["pair"]})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
