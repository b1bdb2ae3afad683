"""Directed topologies (column-stochastic CSR for push-sum) and the trainer's push-sum refusals; no GPU."""
import numpy as np
import pytest

import topology
from trainer import DecentralizedTrainer
from worker import Worker

BUILDERS = {"directed_ring": topology.directed_ring, "exponential": topology.exponential,
            "random_digraph": lambda n: topology.random_digraph(n, min(3, max(n - 1, 1)), seed=0)}


@pytest.mark.parametrize("n", [1, 2, 8, 12])
@pytest.mark.parametrize("name", list(BUILDERS))
def test_directed_csr(name, n):
    t = BUILDERS[name](n)
    A = t.dense_W()
    assert np.all(np.abs(A.sum(axis=0) - 1.0) <= 1e-15 * n) and np.all(np.diag(A) > 0)
    assert t.n == n and t.name == name and np.array_equal(t.degrees, t.out_degrees)
    for i in range(n):
        cols = t.col[t.row_ptr[i]:t.row_ptr[i + 1]]
        assert np.all(np.diff(cols) > 0)
        assert set(cols) == {i} | {j for j in range(n) if i in t.out_neighbours[j]}
        np.testing.assert_array_equal(t.w[t.row_ptr[i]:t.row_ptr[i + 1]], 1.0 / (1.0 + t.out_degrees[cols]))
    t.check()
    assert topology.build(name, n, {"regular_degree": min(3, max(n - 1, 1))}).col.tolist() == t.col.tolist()


def test_graph_shapes():
    assert set(topology.exponential(8).out_neighbours[0]) == {1, 2, 4}
    a, b, c = (topology.random_digraph(12, 3, seed=s) for s in (0, 0, 1))
    assert a.col.tolist() == b.col.tolist() and a.col.tolist() != c.col.tolist()
    assert len(set(np.diff(a.row_ptr))) > 1  # unequal in-degrees
    A = topology.DirectedTopology.from_undirected(topology.ring(8)).dense_W()
    np.testing.assert_allclose(A.sum(axis=0), 1.0, atol=1e-15)
    np.testing.assert_allclose(A.sum(axis=1), 1.0, atol=1e-15)


def trainer(topo="random_digraph", **cfg):
    cfg = dict({"problem_type": "logistic", "learning_rate_eta0": 0.05, "l2_regularization_lambda": 1e-4,
                "strong_convexity_mu": 1e-3, "algorithm": "push_sum", "regular_degree": 2}, **cfg)
    rng = np.random.default_rng(0)
    workers = [Worker(i, {"X": rng.standard_normal((6, 5)), "y": np.ones(6)}, 3, 5, cfg) for i in range(4)]
    return DecentralizedTrainer(workers, topo, 5, cfg), workers


def test_directed_name_needs_push_sum():
    for name in topology.DIRECTED:
        with pytest.raises(ValueError, match="directed"):
            trainer(name, algorithm="dsgd")
    tr, _ = trainer()
    np.testing.assert_allclose(tr.W.sum(axis=0), 1.0)
    assert np.array_equal(tr.degrees, [2.0] * 4)


@pytest.mark.parametrize("cfg", [{"checkpoint_path": "ck.npz"}, {"resume_from": "ck.npz"}, {"sampling": "device"},
                                 {"local_steps": 2}, {"problem_type": "softmax", "num_classes": 3}, {"sparse": True},
                                 {"multi_rank": True}])
def test_push_sum_refusals(cfg, monkeypatch):
    import trainer as trainer_module

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
