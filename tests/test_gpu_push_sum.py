"""Push-sum SGD (dopt_run_pushsum, k_round_pushsum) against a plain float64 numpy loop of the recursion
  v = A u;  phi <- A phi;  z = v / phi;  u <- v - eta_t (grad f(z) + lam z);  metrics at zt = u / phi
over a column-stochastic A (u = 0, phi = 1 at t = 0).  float64 arithmetic (either row storage): the
project's parity tolerance, rtol 1e-9 with atol 1e-12 max|ref|.  float32: see
test_push_sum_matches_reference."""
import functools

import numpy as np
import pytest

import _dopt
import dsgd_oracle as O
import topology
from trainer import DecentralizedTrainer
from worker import Worker

pytestmark = pytest.mark.gpu
T = 6
CFG = {"learning_rate_eta0": 0.05, "l2_regularization_lambda": 1e-4, "strong_convexity_mu": 1e-3}
TOL64 = dict.fromkeys(("objective", "consensus", "u", "phi", "z"), (1e-9, 1e-12))
# float32 row: 8 x the deviations in test_push_sum_matches_reference's docstring, as (rtol, atol / max|ref|)
TOL32 = {"objective": (8 * 1.4e-7, 0.0), "consensus": (8 * 2.4e-7, 0.0), "u": (0.0, 8 * 1.6e-7),
         "phi": (8 * 2.3e-7, 0.0), "z": (0.0, 8 * 5.0e-8)}

#        problem      engine dtypes            d     shard sizes            batch  graph
CASES = {
    "x32": ("logistic", ("float64", "float32"), 1024, [24] * 64, None, lambda: topology.random_digraph(64, 3)),
    "ragged": ("quadratic", ("float64", None), 200, [0, 5, 9, 33] * 4, None, lambda: topology.random_digraph(16, 3)),
    "f32idx": ("logistic", ("float32", None), 77, [11] * 12, 4, lambda: topology.random_digraph(12, 2)),
    "cpl16": ("logistic", ("float64", None), 2048, [9] * 8, None, lambda: topology.exponential(8)),
}


def make_shards(problem, d, sizes, seed, f32):
    rng = np.random.default_rng(seed)
    wstar = rng.standard_normal(d)
    shards = []
    for m in sizes:
        X = np.hstack([rng.standard_normal((m, d - 1)) / np.sqrt(d), np.ones((m, 1))])
        if f32:
            X = X.astype(np.float32).astype(np.float64)
        y = np.sign(X @ wstar + 1e-9) if problem == "logistic" else X @ wstar + 0.1 * rng.standard_normal(m)
        shards.append((X, y.astype(np.float32).astype(np.float64) if f32 else y))
    return shards


def pushsum_reference(problem, shards, A, rounds, cfg, idx=None, dtype=np.float64):
    Xs = [(X.astype(dtype), y.astype(dtype)) for X, y in shards]
    Xf, yf = np.vstack([s[0] for s in Xs]), np.concatenate([s[1] for s in Xs])
    A = A.astype(dtype)
    u = np.zeros((len(shards), Xf.shape[1]), dtype=dtype)
    phi = np.ones(len(shards), dtype=dtype)
    out = {"objective": [], "consensus": []}
    for t in range(rounds):
        v, phi = A @ u, A @ phi
        z = v / phi[:, None]
        g = np.zeros_like(u)
        for i, (X, yv) in enumerate(Xs):
            sel = slice(None) if idx is None else idx[t, i, :min(idx.shape[2], len(yv))]
            g[i] = O.gradient(problem, z[i], X[sel], yv[sel], cfg)
        u = v - dtype(cfg["learning_rate_eta0"] / np.sqrt(t + 1)) * g
        zt = u / phi[:, None]
        avg = zt.mean(axis=0)
        out["consensus"].append(float(np.mean(np.sum((zt - avg) ** 2, axis=1))))
        out["objective"].append(float(O.objective(problem, avg, Xf, yf, cfg["l2_regularization_lambda"])))
    out.update(u=u, phi=phi, z=zt)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, shards, topology, minibatch indices or None, float64 reference) of a row, made once."""
    problem, dtypes, d, sizes, b, graph = CASES[name]
    shards = make_shards(problem, d, sizes, 11, "float32" in dtypes)
    top = graph()
    idx = None
    if b is not None:
        np.random.seed(7)
        idx = _dopt.mt_choice_rounds(T, sizes, b)
    cfg = dict(CFG, problem_type=problem)
    return problem, shards, top, idx, pushsum_reference(problem, shards, top.dense_W(), T, cfg, idx)


def engine(name):
    problem, shards, top, idx, _ = case(name)
    dtype, data_dtype = CASES[name][1]
    eng = _dopt.Engine(0, dtype, data_dtype=data_dtype)
    off = np.concatenate([[0], np.cumsum([len(s[1]) for s in shards])])
    eng.load_shards(problem, np.vstack([s[0] for s in shards]), np.concatenate([s[1] for s in shards]), off)
    eng.set_topology(top.row_ptr, top.col, top.w)
    return eng


def run(eng, name, rounds, t0=0):
    problem, shards, _, idx, _ = case(name)
    b = CASES[name][4] or max(len(s[1]) for s in shards)
    lam = CFG["l2_regularization_lambda"] if problem == "logistic" else CFG["strong_convexity_mu"]
    obj, cons, _ = eng.run_pushsum(rounds, CFG["learning_rate_eta0"], b, lam, CFG["l2_regularization_lambda"], t0=t0,
                                   idx=None if idx is None else idx[t0:t0 + rounds])
    return obj, cons


def check(got, ref, tol):
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        print(k, "max |got - ref| / max|ref| =", np.max(np.abs(np.asarray(got[k]) - r)) / np.max(np.abs(r)))
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        np.testing.assert_allclose(got[k], r, rtol=rtol, atol=atol * np.max(np.abs(r)), err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_push_sum_matches_reference(name):
    """Every round's objective and consensus, the final u, phi and z against the float64 loop.
    float32 row (f32idx): the same loop in numpy float32 deviates from float64, on the CPU, by
    objective 1.4e-7, consensus 2.4e-7 and phi 2.3e-7 (relative, worst entry), u 1.6e-7 and z 5.0e-8
    (max abs / max|ref|); each tolerance is 8 x that, for the GPU's other summation order."""
    ref = case(name)[4]
    if "random_digraph" in case(name)[2].name:  # the weights leave 1: a kernel that ignored phi cannot pass
        assert ref["phi"].min() < 0.5
    eng = engine(name)
    obj, cons = run(eng, name, T)
    phi, z = eng.pushsum_get_state()
    got = {"objective": obj, "consensus": cons, "u": eng.get_models(), "phi": phi, "z": z}
    eng.close()
    f64 = CASES[name][1][0] == "float64"
    check(got, ref, TOL64 if f64 else TOL32)
    if f64:  # A is column-stochastic: the weights keep their sum
        assert abs(phi.sum() - len(phi)) <= 1e-12 * len(phi)


def test_push_sum_split_calls_bitwise():
    one = engine("x32")
    whole = run(one, "x32", T) + (one.get_models(),) + one.pushsum_get_state()
    one.close()
    two = engine("x32")
    first, second = run(two, "x32", 3), run(two, "x32", 3, t0=3)
    split = (np.concatenate([first[0], second[0]]), np.concatenate([first[1], second[1]]), two.get_models())
    split += two.pushsum_get_state()
    two.close()
    for a, b in zip(whole, split):
        np.testing.assert_array_equal(a, b)


def test_trainer_push_sum():
    rounds, sizes, d, b = 8, [14] * 9, 20, 5
    cfg = dict(CFG, problem_type="logistic", local_batch_size=b, algorithm="push_sum", regular_degree=3)
    shards = make_shards("logistic", d, sizes, 3, False)
    Xf, yf = np.vstack([s[0] for s in shards]), np.concatenate([s[1] for s in shards])
    np.random.seed(21)
    state = np.random.get_state()
    idx = _dopt.mt_choice_rounds(rounds, sizes, b)
    ref = pushsum_reference("logistic", shards, topology.random_digraph(9, 3).dense_W(), rounds, cfg, idx)
    np.random.set_state(state)
    workers = [Worker(i, {"X": X, "y": y}, b, d, cfg) for i, (X, y) in enumerate(shards)]
    tr = DecentralizedTrainer(workers, "random_digraph", d, cfg)
    hist, avg = tr.run(rounds, Xf, yf)
    assert [len(hist[k]) for k in ("objective", "consensus_error", "time")] == [rounds] * 3
    got = {"objective": hist["objective"], "consensus": hist["consensus_error"],
           "z": np.stack([w.x for w in workers])}
    check(got, ref, {k: TOL64[k] for k in got})
    np.testing.assert_allclose(avg, ref["z"].mean(axis=0), rtol=1e-9, atol=1e-12 * np.max(np.abs(ref["z"])))
    assert tr.total_floats_transmitted == rounds * int(np.sum(tr.degrees)) * (d + 1)
