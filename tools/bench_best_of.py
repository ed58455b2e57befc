"""TSPEnv.best_of (co_tsp_best_of, one launch) against the composition it replaces
(co_tsp_reward on the lazily replicated td, torch.max over the [K, B] view,
gather_by_index of the winning rows) -- measurement tool, not part of the product.

Cases: TSP-100 B=512 K=800, TSP-100 B=8192 K=8, TSP-20 B=4096 K=160.  The variants
alternate in one process (composition, fused, composition again: the composition is timed
twice so that its own run-to-run spread is known), one warm-up and 7 timed calls each,
device events around each call (which includes each variant's status read), outputs
compared before timing.  Reported: median ms per call, the algorithmic bytes (8*K*B*N of
action rows, 8*B*N of coordinates, the outputs), the resulting bytes/s and the
co_probe_copy rate of the same run.  A case passes when the fused call is no slower than
the composition by more than the composition's two runs differ.
Usage: python tools/bench_best_of.py [--quick] -> one JSON line."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rl4co_slap_amd import TensorDict  # noqa: E402
from rl4co_slap_amd import _native as nat  # noqa: E402
from rl4co_slap_amd.envs import TSPEnv  # noqa: E402
from rl4co_slap_amd.utils.ops import batchify, gather_by_index, unbatchify  # noqa: E402

CASES = ((100, 512, 800), (100, 8192, 8), (20, 4096, 160))  # (N, B, K)
WARMUP, CALLS = 1, 7


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def probe_copy_rate(dev, nbytes=1 << 28):
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def run():
        nat.call("co_probe_copy", nat.ptr(src), nat.ptr(dst), nbytes, nat.stream_of(src))

    run()
    ms = statistics.median(event_ms(run)[0] for _ in range(CALLS))
    return 2 * nbytes / (ms * 1e-3)


def measure(n, b, k, dev):
    g = torch.Generator().manual_seed(n * 1000 + k)
    locs = torch.rand(b, n, 2, generator=g).to(dev)
    acts = torch.rand(k * b, n, generator=g).argsort(1).to(dev)
    env = TSPEnv(generator_params=dict(num_loc=n), device=dev)
    env._BEST_OF_FORCE = True  # time the kernel on every case, whatever the dispatch says
    td = TensorDict({"locs": locs}, [b])

    def composition():
        rew = env.get_reward(batchify(td, k), acts)
        r, i = unbatchify(rew, k).max(dim=1)
        return r, i, gather_by_index(unbatchify(acts, k), i, dim=1)

    def fused():
        return env.best_of(td, acts, k)

    want, got = composition(), fused()
    same_idx = bool(torch.equal(want[1], got[1]) and torch.equal(want[2], got[2]))
    i32 = lambda t: t.view(torch.int32).long()  # noqa: E731  (rewards are negative: same sign)
    ulps = int((i32(want[0]) - i32(got[0])).abs().max().item())
    variants = (("composition_a", composition), ("fused", fused), ("composition_b", composition))
    times = {name: [] for name, _ in variants}
    for it in range(WARMUP + CALLS):
        for name, fn in variants:
            ms, _ = event_ms(fn)
            if it >= WARMUP:
                times[name].append(ms)
    med = {name: statistics.median(v) for name, v in times.items()}
    nbytes = 8 * k * b * n + 8 * b * n + b * (4 + 8 + 8 * n)
    spread = abs(med["composition_a"] - med["composition_b"])
    comp = min(med["composition_a"], med["composition_b"])
    return {"n": n, "instances": b, "candidates": k,
            "ms_fused": round(med["fused"], 4),
            "ms_composition_a": round(med["composition_a"], 4),
            "ms_composition_b": round(med["composition_b"], 4),
            "ms_all": {name: [round(x, 4) for x in v] for name, v in times.items()},
            "algorithmic_bytes": nbytes,
            "fused_bytes_per_s": round(nbytes / (med["fused"] * 1e-3), 1),
            "composition_bytes_per_s": round(nbytes / (comp * 1e-3), 1),
            "same_index_and_rows": same_idx, "reward_max_ulp": ulps,
            "passes": bool(med["fused"] - comp <= spread)}


def main():
    quick = "--quick" in sys.argv
    dev = torch.device("cuda:0")
    nat.load()
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "calls": CALLS,
           "probe_copy_bytes_per_s": round(probe_copy_rate(dev), 1), "cases": []}
    for n, b, k in CASES:
        if quick:
            b = max(1, b // 16)
        res["cases"].append(measure(n, b, k, dev))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
