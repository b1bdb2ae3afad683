"""D-SGD over CSR shards (dopt_run_sparse, k_round_sparse) against a plain float64 numpy loop with
scipy.sparse products:
  z = X_i x_i;  r = -y sigma(-y z) | z - y;  g_i = X_i^T r / b + lam x_i  (0 for an empty shard);
  x_i <- sum_j W_ij x_j - eta_t g_i
with the objective at the average iterate and the consensus of every round.  float64 arithmetic (either
value storage): the project's parity tolerance, rtol 1e-9 with atol 1e-12 max|ref|.  float32: see
test_sparse_matches_reference."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _dopt
import topology
from trainer import DecentralizedTrainer
from worker import Worker

pytestmark = pytest.mark.gpu
T = 6
ETA0, LAM = 0.05, 1e-4
TOL64 = dict.fromkeys(("objective", "consensus", "x"), (1e-9, 1e-12))
# float32 row: 8 x the deviations in test_sparse_matches_reference's docstring, as (rtol, atol / max|ref|)
TOL32 = {"objective": (8 * 1.4e-7, 0.0), "consensus": (8 * 1.6e-7, 0.0), "x": (0.0, 8 * 2.0e-7)}

#        engine dtypes           problem      d      shard sizes           nnz / row  batch  graph
CASES = {
    "tiny": (("float64", None), "logistic", 70, [6] * 4, 0.3 * 69, None, lambda: topology.ring(4)),
    # one row of every shard is blanked (no non-zeros, not even the bias); the bias column of the 150-row
    # shards has 149 entries, past the long-column threshold (32)
    "tails": (("float64", None), "quadratic", 300, [0, 5, 17, 150] * 4, 0.05 * 299, None, lambda: topology.ring(16)),
    "wide": (("float64", "float32"), "logistic", 70001, [40] * 8, 30, None, lambda: topology.random_regular(8, 4)),
    "f32idx": (("float32", None), "logistic", 129, [11] * 12, 0.2 * 128, 4, lambda: topology.fully_connected(12)),
}


def make_shards(problem, d, sizes, per_row, seed, f32, blank_row=False):
    rng = np.random.default_rng(seed)
    wstar = rng.standard_normal(d)
    shards = []
    for m in sizes:
        X = sp.hstack([sp.random(m, d - 1, density=per_row / (d - 1), random_state=rng, format="csr"),
                       np.ones((m, 1))], format="lil")
        if blank_row and m:
            X[m // 2] = 0
        X = X.tocsr()
        X.eliminate_zeros()
        if f32:
            X = X.astype(np.float32).astype(np.float64)
        z = X @ wstar
        y = np.where(z >= 0, 1.0, -1.0) if problem == "logistic" else z + 0.1 * rng.standard_normal(m)
        if f32:
            y = y.astype(np.float32).astype(np.float64)
        shards.append((X, y))
    return shards


def sparse_reference(shards, W, problem, rounds, idx=None, dtype=np.float64):
    Xs = [(X.astype(dtype), y.astype(dtype)) for X, y in shards]
    Xf, yf = sp.vstack([s[0] for s in Xs], format="csr"), np.concatenate([s[1] for s in Xs])
    W = W.astype(dtype)
    x = np.zeros((len(shards), Xf.shape[1]), dtype=dtype)
    out = {"objective": [], "consensus": []}
    for t in range(rounds):
        g = np.zeros_like(x)
        for i, (X, y) in enumerate(Xs):
            sel = slice(None) if idx is None else idx[t, i, :min(idx.shape[2], len(y))]
            Xb, yb = X[sel], y[sel]
            if len(yb):
                z = Xb @ x[i]
                r = -yb / (1 + np.exp(yb * z)) if problem == "logistic" else z - yb
                g[i] = Xb.T @ r / dtype(len(yb)) + dtype(LAM) * x[i]
        x = W @ x - dtype(ETA0 / np.sqrt(t + 1)) * g
        avg = x.mean(axis=0)
        out["consensus"].append(float(np.mean(np.sum((x - avg) ** 2, axis=1))))
        u = Xf @ avg
        loss = np.mean(np.log(1 + np.exp(-yf * u))) if problem == "logistic" else dtype(0.5) * np.mean((u - yf) ** 2)
        out["objective"].append(float(loss + dtype(LAM / 2) * (avg @ avg)))
    out["x"] = x
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(shards, topology, minibatch indices or None, float64 reference) of a row, made once."""
    dtypes, problem, d, sizes, per_row, b, graph = CASES[name]
    shards = make_shards(problem, d, sizes, per_row, 11, "float32" in dtypes, blank_row=name == "tails")
    top = graph()
    idx = None
    if b is not None:
        np.random.seed(7)
        idx = _dopt.mt_choice_rounds(T, sizes, b)
    return shards, top, idx, sparse_reference(shards, top.dense_W(), problem, T, idx)


def load(eng, shards, problem):
    X = sp.vstack([s[0] for s in shards], format="csr")
    off = np.concatenate([[0], np.cumsum([len(s[1]) for s in shards])])
    eng.load_shards_csr(problem, X.indptr, X.indices, X.data, np.concatenate([s[1] for s in shards]), off, X.shape[1])


def engine(name):
    shards, top, _, _ = case(name)
    (dtype, data_dtype), problem = CASES[name][:2]
    eng = _dopt.Engine(0, dtype, data_dtype=data_dtype)
    load(eng, shards, problem)
    eng.set_topology(top.row_ptr, top.col, top.w)
    return eng


def run(eng, name, rounds, t0=0):
    shards, _, idx, _ = case(name)
    b = CASES[name][5] or max(len(s[1]) for s in shards)
    obj, cons, _ = eng.run_sparse(rounds, ETA0, b, LAM, LAM, t0=t0, idx=None if idx is None else idx[t0:t0 + rounds])
    return obj, cons


def check(got, ref, tol):
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        print(k, "max |got - ref| / max|ref| =", np.max(np.abs(np.asarray(got[k]) - r)) / np.max(np.abs(r)))
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        np.testing.assert_allclose(got[k], r, rtol=rtol, atol=atol * np.max(np.abs(r)), err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_sparse_matches_reference(name):
    """Every round's objective and consensus and the final iterates against the float64 loop.
    float32 row (f32idx): the same loop in numpy float32 deviates from float64, on the CPU, by
    objective 1.4e-7 and consensus 1.6e-7 (relative, worst round) and x 2.0e-7 (max abs / max|ref|);
    each tolerance is 8 x that, for the GPU's other summation order."""
    ref = case(name)[3]
    eng = engine(name)
    obj, cons = run(eng, name, T)
    got = {"objective": obj, "consensus": cons, "x": eng.get_models()}
    if name == "tails":  # the densified shard, blank row and bias column included
        np.testing.assert_array_equal(eng.get_shard(3)[0], case(name)[0][3][0].toarray())
    eng.close()
    check(got, ref, TOL64 if CASES[name][0][0] == "float64" else TOL32)


def test_sparse_split_calls_bitwise():
    one = engine("wide")
    whole = run(one, "wide", T) + (one.get_models(),)
    one.close()
    two = engine("wide")
    first, second = run(two, "wide", 3), run(two, "wide", 3, t0=3)
    split = (np.concatenate([first[0], second[0]]), np.concatenate([first[1], second[1]]), two.get_models())
    two.close()
    for a, b in zip(whole, split):
        np.testing.assert_array_equal(a, b)


def test_sparse_two_runs_bitwise():
    runs = []
    for _ in range(2):
        eng = engine("tails")
        runs.append(run(eng, "tails", T) + (eng.get_models(),))
        eng.close()
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


def test_trainer_sparse():
    rounds, sizes, d, b = 8, [14] * 9, 40, 5
    cfg = {"problem_type": "logistic", "local_batch_size": b, "learning_rate_eta0": ETA0,
           "l2_regularization_lambda": LAM, "strong_convexity_mu": LAM}
    shards = make_shards("logistic", d, sizes, 8, 3, False)
    Xf, yf = sp.vstack([s[0] for s in shards], format="csr"), np.concatenate([s[1] for s in shards])
    np.random.seed(21)
    state = np.random.get_state()
    idx = _dopt.mt_choice_rounds(rounds, sizes, b)
    ref = sparse_reference(shards, topology.grid(9).dense_W(), "logistic", rounds, idx)
    np.random.set_state(state)
    workers = [Worker(i, {"X": X, "y": y}, b, d, cfg) for i, (X, y) in enumerate(shards)]
    tr = DecentralizedTrainer(workers, "grid", d, cfg)
    hist, avg = tr.run(rounds, Xf, yf)
    assert [len(hist[k]) for k in ("objective", "consensus_error", "time")] == [rounds] * 3
    got = {"objective": hist["objective"], "consensus": hist["consensus_error"],
           "x": np.stack([w.x for w in workers])}
    check(got, ref, TOL64)
    np.testing.assert_allclose(avg, ref["x"].mean(axis=0), rtol=1e-9, atol=1e-12 * np.max(np.abs(ref["x"])))
    assert tr.total_floats_transmitted == rounds * int(np.sum(tr.degrees)) * d


def test_dense_rounds_refuse_a_sparse_context():
    eng = engine("tiny")
    with pytest.raises(NotImplementedError, match="sparse context"):
        eng.run_dsgd(1, ETA0, 6, LAM, LAM)
    X, y = case("tiny")[0][0]
    eng.load_shards("logistic", np.vstack([X.toarray()] * 4), np.tile(y, 4), np.arange(5) * 6)  # ordinary again
    eng.set_topology(*[getattr(case("tiny")[1], k) for k in ("row_ptr", "col", "w")])
    with pytest.raises(RuntimeError, match="not a sparse context"):
        eng.run_sparse(1, ETA0, 6, LAM, LAM)
    eng.close()


@pytest.mark.parametrize("indices", [[0, 5], [3, 1], [2, 2]], ids=["col_ge_d", "descending", "duplicate"])
def test_bad_csr(indices):
    eng = _dopt.Engine(0, "float64")
    with pytest.raises(ValueError, match="column"):
        eng.load_shards_csr("logistic", [0, 2], indices, [1.0, 2.0], [1.0], [0, 1], 5)
    eng.close()
