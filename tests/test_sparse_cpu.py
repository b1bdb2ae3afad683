"""Workers with scipy.sparse X_local: the combinations the sparse round does not support are refused
before any device call (this file needs no GPU)."""
import numpy as np
import pytest
import scipy.sparse as sp

import trainer
from worker import Worker

CFG = {"problem_type": "logistic", "local_batch_size": 2, "learning_rate_eta0": 0.05,
       "l2_regularization_lambda": 1e-4, "strong_convexity_mu": 1e-4}


def workers(cfg, dense=()):
    rng = np.random.default_rng(0)
    out = []
    for i in range(4):
        X = rng.standard_normal((3, 4))
        out.append(Worker(i, {"X": X if i in dense else sp.csr_matrix(X), "y": np.array([1.0, -1.0, 1.0])}, 2, 4, cfg))
    return out


def make(topology="ring", dense=(), **extra):
    cfg = dict(CFG, **extra)
    return trainer.DecentralizedTrainer(workers(cfg, dense), topology, 4, cfg)


def test_mixed_sparse_and_dense_workers():
    with pytest.raises(ValueError, match="sparse and dense"):
        make(dense=(1,)).run(1)


@pytest.mark.parametrize("topology, extra", [
    ("ring", {"algorithm": "gradient_tracking"}),
    ("ring", {"algorithm": "choco", "compression_k": 2, "choco_gamma": 0.5}),
    ("fully_connected", {"mean_mixing_min": 2}),
    ("ring", {"checkpoint_path": "ck.npz"}),
    ("ring", {"resume_from": "ck.npz"}),
    ("ring", {"sampling": "device"}),
])
def test_unsupported_combinations(topology, extra):
    with pytest.raises(NotImplementedError, match="sparse shards"):
        make(topology, **extra).run(1)


def test_foreign_objective_rows():
    with pytest.raises(NotImplementedError, match="sparse shards.*X_full"):
        make().run(1, np.ones((12, 4)), np.tile([1.0, -1.0, 1.0], 4))


def test_centralized_trainer():
    with pytest.raises(NotImplementedError, match="sparse shards"):
        trainer.CentralizedTrainer(workers(CFG), 4, CFG).run(1)
