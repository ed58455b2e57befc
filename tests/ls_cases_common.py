"""What tests/two_opt_cases.py, cvrp_ls_cases.py and slap_ls_cases.py share: read-only case
arrays and the numpy <-> torch adaptors of their ``run`` functions."""
import numpy as np
import torch


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def to_device(a, dtype, device):
    """A numpy input (or None) as a tensor on ``device``; copies: the cases are read-only."""
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype)).to(device)


def to_numpy(tensors):
    return tuple(t.cpu().numpy() for t in tensors)
