"""What tools/bench_two_opt.py, bench_cvrp_ls.py and bench_slap_ls.py share (measurement
tools, not part of the product): the device timing of one search call and the host leg."""
import statistics
import time

import torch

HOST_ROWS, HOST_THREADS = 256, 1


def timed(fn, dev):
    """(ms per ``fn()`` call: the median of 5 calls after a warm-up, by device events around
    the call; the last call's result)."""
    fn()  # warm-up
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), res


def host_leg(fn, *tensors):
    """``fn`` on the first HOST_ROWS rows of every tensor (None stays None), moved to the
    CPU: the host build, wall clock, one thread (the host library is single-threaded).
    Returns (the CPU inputs, ms, the result)."""
    h = [None if x is None else x[:HOST_ROWS].cpu() for x in tensors]
    t0 = time.perf_counter()
    res = fn(*h)
    return h, (time.perf_counter() - t0) * 1e3, res


def same_rows(host, device):
    """Every host result equals the device result's first rows."""
    return bool(all(torch.equal(h, d[:HOST_ROWS].cpu()) for h, d in zip(host, device)))
