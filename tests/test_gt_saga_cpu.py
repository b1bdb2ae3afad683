"""The trainer's GT-SAGA refusals and the step_rule key; no GPU."""
import numpy as np
import pytest

from trainer import DecentralizedTrainer
from worker import Worker


def trainer(**cfg):
    cfg = dict({"problem_type": "logistic", "learning_rate_eta0": 0.05, "l2_regularization_lambda": 1e-4,
                "strong_convexity_mu": 1e-3, "algorithm": "gt_saga"}, **cfg)
    rng = np.random.default_rng(0)
    workers = [Worker(i, {"X": rng.standard_normal((6, 5)), "y": np.ones(6)}, 3, 5, cfg) for i in range(4)]
    return DecentralizedTrainer(workers, "ring", 5, cfg), workers


@pytest.mark.parametrize("cfg", [{"checkpoint_path": "ck.npz"}, {"resume_from": "ck.npz"}, {"local_steps": 2},
                                 {"problem_type": "softmax", "num_classes": 3}, {"sparse": True}, {"multi_rank": True}])
def test_gt_saga_refusals(cfg, monkeypatch):
    import _dopt
    import trainer as trainer_module

    def no_device(*args, **kwargs):
        raise AssertionError("refusals come before any device call")

    monkeypatch.setattr(_dopt, "Engine", no_device)
    cfg = dict(cfg)
    if cfg.pop("multi_rank", False):
        monkeypatch.setattr(trainer_module, "_dist_info", lambda config: (0, 2, "gloo"))
    sparse = cfg.pop("sparse", False)
    tr, workers = trainer(**cfg)
    if sparse:
        import scipy.sparse as sp

        for w in workers:
            w.X_local = sp.csr_matrix(w.X_local)
    with pytest.raises(NotImplementedError):
        tr.run(2)


def test_step_rule_validation():
    with pytest.raises(ValueError, match="step_rule"):
        trainer(step_rule="linear")
    for algorithm in ("dsgd", "gradient_tracking", "choco", "push_sum"):
        with pytest.raises(ValueError, match="step_rule='constant' runs algorithm='gt_saga'"):
            trainer(algorithm=algorithm, step_rule="constant")
    trainer(algorithm="gradient_tracking", step_rule="decay")
    assert trainer(step_rule="constant")[0].config["step_rule"] == "constant"


def test_unknown_algorithm_names_gt_saga():
    tr, _ = trainer(algorithm="adam")
    with pytest.raises(ValueError, match="unknown algorithm.*'dsgd', 'gradient_tracking' or 'choco'.*gt_saga"):
        tr.run(2)
