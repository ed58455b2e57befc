"""``rl4co/tasks``: inference-time use of the engine (policy evaluation)."""
from .eval import (AugmentationEval, EvalBase, GreedyEval, GreedyMultiStartAugmentEval,
                   GreedyMultiStartEval, SamplingEval, evaluate_policy,
                   get_automatic_batch_size)

__all__ = ["AugmentationEval", "EvalBase", "GreedyEval", "GreedyMultiStartAugmentEval",
           "GreedyMultiStartEval", "SamplingEval", "evaluate_policy",
           "get_automatic_batch_size"]
