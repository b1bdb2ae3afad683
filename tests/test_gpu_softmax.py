"""Softmax-regression D-SGD (dopt_run_softmax, k_round_softmax) against a plain float64 numpy loop of
  z = X W_i^T;  G_i = (softmax(z) - Y)^T X / b + lam W_i  (0 for an empty shard);  W_i <- sum_j Wmix_ij W_j - eta_t G_i
with the objective (mean logsumexp(z) - z[y] at the average iterate, + lam / 2 ||.||_F^2) and the consensus
of every round.  float64 arithmetic (either row storage): the project's parity tolerance, rtol 1e-9
with atol 1e-12 max|ref|.  float32: see test_softmax_matches_reference."""
import functools

import numpy as np
import pytest

import _dopt
import topology
from trainer import DecentralizedTrainer
from worker import Worker

pytestmark = pytest.mark.gpu
T = 6
ETA0, LAM = 0.05, 1e-4
TOL64 = dict.fromkeys(("objective", "consensus", "x"), (1e-9, 1e-12))
# float32 row: 8 x the deviations in test_softmax_matches_reference's docstring, as (rtol, atol / max|ref|)
TOL32 = {"objective": (8 * 1.5e-7, 0.0), "consensus": (8 * 1.3e-7, 0.0), "x": (0.0, 8 * 1.1e-7)}

#        engine dtypes            d     C   shard sizes            batch  graph
CASES = {
    "one_tile": (("float64", None), 64, 16, [16] * 4, None, lambda: topology.ring(4)),
    "tails": (("float64", None), 200, 3, [0, 5, 17, 33] * 4, None, lambda: topology.ring(16)),
    "x32": (("float64", "float32"), 1024, 10, [24] * 16, None, lambda: topology.random_regular(16, 4)),
    "f32idx": (("float32", None), 77, 2, [11] * 12, 4, lambda: topology.fully_connected(12)),
    "widest": (("float64", None), 1024, 16, [9] * 8, None, lambda: topology.ring(8)),
}


def make_shards(d, C, sizes, seed, f32):
    rng = np.random.default_rng(seed)
    wstar = rng.standard_normal((C, d))
    shards = []
    for m in sizes:
        X = np.hstack([rng.standard_normal((m, d - 1)) / np.sqrt(d), np.ones((m, 1))])
        if f32:
            X = X.astype(np.float32).astype(np.float64)
        shards.append((X, np.argmax(X @ wstar.T, axis=1).astype(np.float64)))
    return shards


def softmax_reference(shards, W, C, rounds, idx=None, dtype=np.float64):
    Xs = [(X.astype(dtype), y.astype(np.int64)) for X, y in shards]
    Xf, yf = np.vstack([s[0] for s in Xs]), np.concatenate([s[1] for s in Xs])
    W = W.astype(dtype)
    x = np.zeros((len(shards), C, Xf.shape[1]), dtype=dtype)
    out = {"objective": [], "consensus": []}
    for t in range(rounds):
        g = np.zeros_like(x)
        for i, (X, k) in enumerate(Xs):
            sel = slice(None) if idx is None else idx[t, i, :min(idx.shape[2], len(k))]
            Xb, kb = X[sel], k[sel]
            if len(kb):
                z = Xb @ x[i].T
                P = np.exp(z - z.max(axis=1, keepdims=True))
                P /= P.sum(axis=1, keepdims=True)
                P[np.arange(len(kb)), kb] -= 1
                g[i] = P.T @ Xb / dtype(len(kb)) + dtype(LAM) * x[i]
        x = np.einsum("ij,jcd->icd", W, x) - dtype(ETA0 / np.sqrt(t + 1)) * g
        avg = x.mean(axis=0)
        out["consensus"].append(float(np.mean(np.sum((x - avg) ** 2, axis=(1, 2)))))
        z = Xf @ avg.T
        zmax = z.max(axis=1)
        loss = zmax + np.log(np.exp(z - zmax[:, None]).sum(axis=1)) - z[np.arange(len(yf)), yf]
        out["objective"].append(float(loss.mean() + dtype(LAM / 2) * np.sum(avg * avg)))
    out["x"] = x
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(shards, topology, minibatch indices or None, float64 reference) of a row, made once."""
    dtypes, d, C, sizes, b, graph = CASES[name]
    shards = make_shards(d, C, sizes, 11, "float32" in dtypes)
    top = graph()
    idx = None
    if b is not None:
        np.random.seed(7)
        idx = _dopt.mt_choice_rounds(T, sizes, b)
    return shards, top, idx, softmax_reference(shards, top.dense_W(), C, T, idx)


def engine(name):
    shards, top, _, _ = case(name)
    (dtype, data_dtype), C = CASES[name][0], CASES[name][2]
    eng = _dopt.Engine(0, dtype, data_dtype=data_dtype)
    off = np.concatenate([[0], np.cumsum([len(s[1]) for s in shards])])
    eng.load_shards("softmax", np.vstack([s[0] for s in shards]), np.concatenate([s[1] for s in shards]), off,
                    n_classes=C)
    eng.set_topology(top.row_ptr, top.col, top.w)
    return eng


def run(eng, name, rounds, t0=0):
    shards, _, idx, _ = case(name)
    b = CASES[name][4] or max(len(s[1]) for s in shards)
    obj, cons, _ = eng.run_softmax(rounds, ETA0, b, LAM, LAM, t0=t0, idx=None if idx is None else idx[t0:t0 + rounds])
    return obj, cons


def check(got, ref, tol):
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        print(k, "max |got - ref| / max|ref| =", np.max(np.abs(np.asarray(got[k]) - r)) / np.max(np.abs(r)))
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        np.testing.assert_allclose(got[k], r, rtol=rtol, atol=atol * np.max(np.abs(r)), err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_softmax_matches_reference(name):
    """Every round's objective and consensus and the final iterates against the float64 loop.
    float32 row (f32idx): the same loop in numpy float32 deviates from float64, on the CPU, by
    objective 1.5e-7 and consensus 1.3e-7 (relative, worst round) and x 1.1e-7 (max abs / max|ref|);
    each tolerance is 8 x that, for the GPU's other summation order."""
    ref = case(name)[3]
    eng = engine(name)
    obj, cons = run(eng, name, T)
    got = {"objective": obj, "consensus": cons, "x": eng.softmax_get_models()}
    eng.close()
    check(got, ref, TOL64 if CASES[name][0][0] == "float64" else TOL32)


def test_softmax_split_calls_bitwise():
    one = engine("x32")
    whole = run(one, "x32", T) + (one.softmax_get_models(),)
    one.close()
    two = engine("x32")
    first, second = run(two, "x32", 3), run(two, "x32", 3, t0=3)
    split = (np.concatenate([first[0], second[0]]), np.concatenate([first[1], second[1]]), two.softmax_get_models())
    two.close()
    for a, b in zip(whole, split):
        np.testing.assert_array_equal(a, b)


def test_trainer_softmax():
    rounds, sizes, d, C, b = 8, [14] * 9, 20, 3, 5
    cfg = {"problem_type": "softmax", "num_classes": C, "local_batch_size": b, "learning_rate_eta0": ETA0,
           "l2_regularization_lambda": LAM, "strong_convexity_mu": 1e-3}
    shards = make_shards(d, C, sizes, 3, False)
    Xf, yf = np.vstack([s[0] for s in shards]), np.concatenate([s[1] for s in shards])
    np.random.seed(21)
    state = np.random.get_state()
    idx = _dopt.mt_choice_rounds(rounds, sizes, b)
    ref = softmax_reference(shards, topology.grid(9).dense_W(), C, rounds, idx)
    np.random.set_state(state)
    workers = [Worker(i, {"X": X, "y": y}, b, d, cfg) for i, (X, y) in enumerate(shards)]
    tr = DecentralizedTrainer(workers, "grid", d, cfg)
    hist, avg = tr.run(rounds, Xf, yf)
    assert [len(hist[k]) for k in ("objective", "consensus_error", "time")] == [rounds] * 3
    assert all(w.x.shape == (C, d) for w in workers)
    got = {"objective": hist["objective"], "consensus": hist["consensus_error"],
           "x": np.stack([w.x for w in workers])}
    check(got, ref, TOL64)
    np.testing.assert_allclose(avg, ref["x"].mean(axis=0), rtol=1e-9, atol=1e-12 * np.max(np.abs(ref["x"])))
    assert tr.total_floats_transmitted == rounds * int(np.sum(tr.degrees)) * d * C


def test_vector_rounds_refuse_a_softmax_context():
    eng = engine("one_tile")
    with pytest.raises(NotImplementedError, match="softmax context"):
        eng.run_dsgd(1, ETA0, 16, LAM, LAM)
    eng.close()
