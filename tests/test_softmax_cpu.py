"""problem_type = 'softmax': a bad num_classes and the combinations the softmax round does not support
are refused before any device call, and obj_problems.softmax_gradient is the gradient of
softmax_objective (this file needs no GPU)."""
import numpy as np
import pytest

import obj_problems
import trainer
from worker import Worker

CFG = {"problem_type": "softmax", "num_classes": 3, "local_batch_size": 2, "learning_rate_eta0": 0.05,
       "l2_regularization_lambda": 1e-4, "strong_convexity_mu": 1e-4}


def workers(cfg):
    rng = np.random.default_rng(0)
    return [Worker(i, {"X": rng.standard_normal((3, 4)), "y": np.array([0.0, 1.0, 2.0])}, 2, 4, cfg) for i in range(4)]


def make(topology="ring", **extra):
    cfg = {k: v for k, v in dict(CFG, **extra).items() if v is not None}
    return trainer.DecentralizedTrainer(workers(dict(cfg, num_classes=3)), topology, 4, cfg)


@pytest.mark.parametrize("num_classes", [None, 1, 17, 3.0, True])
def test_bad_num_classes(num_classes):
    with pytest.raises(ValueError, match="softmax needs config 'num_classes'"):
        make(num_classes=num_classes).run(1)


@pytest.mark.parametrize("topology, extra", [
    ("ring", {"algorithm": "gradient_tracking"}),
    ("ring", {"algorithm": "choco", "compression_k": 2, "choco_gamma": 0.5}),
    ("fully_connected", {"mean_mixing_min": 2}),
    ("ring", {"checkpoint_path": "ck.npz"}),
    ("ring", {"resume_from": "ck.npz"}),
    ("ring", {"sampling": "device"}),
])
def test_unsupported_combinations(topology, extra):
    with pytest.raises(NotImplementedError, match="softmax"):
        make(topology, **extra).run(1)


def test_multi_rank_job(monkeypatch):
    monkeypatch.setattr(trainer, "_dist_info", lambda config: (0, 2, "gloo"))
    with pytest.raises(NotImplementedError, match="softmax"):
        make().run(1)


def test_foreign_objective_rows():
    with pytest.raises(NotImplementedError, match="softmax.*X_full"):
        make().run(1, np.ones((5, 4)), np.zeros(5))


def test_centralized_trainer():
    with pytest.raises(NotImplementedError, match="softmax"):
        trainer.CentralizedTrainer(workers(CFG), 4, CFG).run(1)


def test_worker_iterate_is_a_matrix():
    assert workers(CFG)[0].x.shape == (3, 4)


def test_gradient_is_the_objectives_derivative():
    """Central differences with h = 1e-6 in float64: truncation ~ h^2 |f'''| / 6 ~ 1e-13 and rounding
    ~ eps |f| / h ~ 3e-10 for f ~ 1; the bound is 1e-8."""
    rng = np.random.default_rng(1)
    W, X, y = rng.standard_normal((3, 5)), rng.standard_normal((7, 5)), rng.integers(0, 3, 7).astype(np.float64)
    fd, h = np.zeros_like(W), 1e-6
    for k in range(W.size):
        E = np.zeros(W.size)
        E[k] = h
        E = E.reshape(W.shape)
        fd.flat[k] = (obj_problems.softmax_objective(W + E, X, y, 0.1) -
                      obj_problems.softmax_objective(W - E, X, y, 0.1)) / (2 * h)
    np.testing.assert_allclose(obj_problems.softmax_gradient(W, X, y, 0.1), fd, rtol=0, atol=1e-8)
    assert obj_problems.softmax_objective(W, X[:0], y[:0], 0.1) == 0.0
    assert not obj_problems.softmax_gradient(W, X[:0], y[:0], 0.1).any()
