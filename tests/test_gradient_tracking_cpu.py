"""DecentralizedTrainer config key 'algorithm': unknown values and the combinations gradient
tracking does not support are refused before any device call (this file needs no GPU)."""
import numpy as np
import pytest

import trainer
from worker import Worker

CFG = {"problem_type": "logistic", "local_batch_size": 2, "learning_rate_eta0": 0.05,
       "l2_regularization_lambda": 1e-4, "strong_convexity_mu": 1e-4, "algorithm": "gradient_tracking"}


def make(topology="ring", **extra):
    cfg = dict(CFG, **extra)
    rng = np.random.default_rng(0)
    ws = [Worker(i, {"X": rng.standard_normal((3, 4)), "y": np.ones(3)}, 2, 4, cfg) for i in range(4)]
    return trainer.DecentralizedTrainer(ws, topology, 4, cfg)


def test_unknown_algorithm():
    with pytest.raises(ValueError, match="unknown algorithm"):
        make(algorithm="extra_gradient").run(1)


@pytest.mark.parametrize("topology, extra", [
    ("fully_connected", {"mean_mixing_min": 2}),
    ("ring", {"checkpoint_path": "ck.npz"}),
    ("ring", {"resume_from": "ck.npz"}),
    ("ring", {"sampling": "device"}),
])
def test_unsupported_combinations(topology, extra):
    with pytest.raises(NotImplementedError, match="gradient tracking"):
        make(topology, **extra).run(1)


def test_multi_rank_job(monkeypatch):
    monkeypatch.setattr(trainer, "_dist_info", lambda config: (0, 2, "gloo"))
    with pytest.raises(NotImplementedError, match="single process"):
        make().run(1)
