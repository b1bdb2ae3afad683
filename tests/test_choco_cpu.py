"""DecentralizedTrainer config 'algorithm' = 'choco': missing or out-of-range keys and the
combinations CHOCO-SGD does not support are refused before any device call (this file needs no GPU)."""
import numpy as np
import pytest

import trainer
from worker import Worker

CFG = {"problem_type": "logistic", "local_batch_size": 2, "learning_rate_eta0": 0.05,
       "l2_regularization_lambda": 1e-4, "strong_convexity_mu": 1e-4, "algorithm": "choco",
       "compression_k": 2, "choco_gamma": 0.5}


def make(topology="ring", **extra):
    cfg = {k: v for k, v in dict(CFG, **extra).items() if v is not None}
    rng = np.random.default_rng(0)
    ws = [Worker(i, {"X": rng.standard_normal((3, 4)), "y": np.ones(3)}, 2, 4, cfg) for i in range(4)]
    return trainer.DecentralizedTrainer(ws, topology, 4, cfg)


def test_unknown_algorithm_names_all_three():
    with pytest.raises(ValueError, match="unknown algorithm.*'dsgd', 'gradient_tracking' or 'choco'"):
        make(algorithm="extra_gradient").run(1)


@pytest.mark.parametrize("extra", [
    {"compression_k": None}, {"compression_k": 0}, {"compression_k": 5}, {"compression_k": 2.0},
    {"choco_gamma": None}, {"choco_gamma": 0.0}, {"choco_gamma": 1.5}, {"choco_gamma": "0.5"},
])
def test_bad_keys(extra):
    with pytest.raises(ValueError, match="CHOCO needs config '%s'" % next(iter(extra))):
        make(**extra).run(1)


@pytest.mark.parametrize("topology, extra", [
    ("fully_connected", {"mean_mixing_min": 2}),
    ("ring", {"checkpoint_path": "ck.npz"}),
    ("ring", {"resume_from": "ck.npz"}),
    ("ring", {"sampling": "device"}),
])
def test_unsupported_combinations(topology, extra):
    with pytest.raises(NotImplementedError, match="CHOCO"):
        make(topology, **extra).run(1)


def test_multi_rank_job(monkeypatch):
    monkeypatch.setattr(trainer, "_dist_info", lambda config: (0, 2, "gloo"))
    with pytest.raises(NotImplementedError, match="CHOCO"):
        make().run(1)
