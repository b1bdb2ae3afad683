"""Local steps (dopt_run_local, k_round_local) against a plain float64 numpy loop of the recursion
  x_{s+1} = W_s x_s - eta_s g_s(x_s),  W_s = W if s mod tau == 0 else I,  eta_s = eta0 / sqrt(s + 1)
with one history row per communication round.  float64 arithmetic (either row storage): the project's
parity tolerance, rtol 1e-9 with atol 1e-12 max|ref|.  float32: see test_local_matches_reference."""
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
TOL64 = dict.fromkeys(("objective", "consensus", "x"), (1e-9, 1e-12))
# float32 row: 8 x the deviations in test_local_matches_reference's docstring, as (rtol, atol / max|ref|)
TOL32 = {"objective": (8 * 1.3e-7, 0.0), "consensus": (8 * 2.8e-7, 0.0), "x": (0.0, 8 * 9.7e-8)}

#        problem      engine dtypes            d     shard sizes            batch  graph                              tau
CASES = {
    "x32": ("logistic", ("float64", "float32"), 1024, [24] * 64, None, lambda: topology.random_regular(64, 4), 3),
    "ragged": ("quadratic", ("float64", None), 200, [0, 5, 9, 33] * 4, None, lambda: topology.ring(16), 2),
    "f32idx": ("logistic", ("float32", None), 77, [11] * 12, 4, lambda: topology.fully_connected(12), 4),
    "cpl16": ("logistic", ("float64", None), 2048, [9] * 8, None, lambda: topology.ring(8), 2),
    "tau1": ("quadratic", ("float64", None), 100, [7] * 5, 3, lambda: topology.ring(5), 1),
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


def local_reference(problem, shards, W, rounds, tau, cfg, idx=None, dtype=np.float64):
    Xs = [(X.astype(dtype), y.astype(dtype)) for X, y in shards]
    Xf, yf = np.vstack([s[0] for s in Xs]), np.concatenate([s[1] for s in Xs])
    W = W.astype(dtype)
    x = np.zeros((len(shards), Xf.shape[1]), dtype=dtype)
    out = {"objective": [], "consensus": []}
    for s in range(rounds * tau):
        g = np.zeros_like(x)
        for i, (X, yv) in enumerate(Xs):
            sel = slice(None) if idx is None else idx[s, i, :min(idx.shape[2], len(yv))]
            g[i] = O.gradient(problem, x[i], X[sel], yv[sel], cfg)
        x = (W @ x if s % tau == 0 else x) - dtype(cfg["learning_rate_eta0"] / np.sqrt(s + 1)) * g
        if s % tau == tau - 1:
            avg = x.mean(axis=0)
            out["consensus"].append(float(np.mean(np.sum((x - avg) ** 2, axis=1))))
            out["objective"].append(float(O.objective(problem, avg, Xf, yf, cfg["l2_regularization_lambda"])))
    out["x"] = x
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, shards, topology, minibatch indices or None, float64 reference) of a row, made once."""
    problem, dtypes, d, sizes, b, graph, tau = CASES[name]
    shards = make_shards(problem, d, sizes, 11, "float32" in dtypes)
    top = graph()
    idx = None
    if b is not None:
        np.random.seed(7)
        idx = _dopt.mt_choice_rounds(T * tau, sizes, b)
    cfg = dict(CFG, problem_type=problem)
    return problem, shards, top, idx, local_reference(problem, shards, top.dense_W(), T, tau, cfg, idx)


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
    tau = CASES[name][6]
    b = CASES[name][4] or max(len(s[1]) for s in shards)
    lam = CFG["l2_regularization_lambda"] if problem == "logistic" else CFG["strong_convexity_mu"]
    obj, cons, _ = eng.run_local(rounds, CFG["learning_rate_eta0"], b, lam, CFG["l2_regularization_lambda"], tau, t0=t0,
                                 idx=None if idx is None else idx[t0 * tau:(t0 + rounds) * tau])
    return obj, cons


def check(got, ref, tol):
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        print(k, "max |got - ref| / max|ref| =", np.max(np.abs(np.asarray(got[k]) - r)) / np.max(np.abs(r)))
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        np.testing.assert_allclose(got[k], r, rtol=rtol, atol=atol * np.max(np.abs(r)), err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_local_matches_reference(name):
    """Every round's objective and consensus and the final iterates against the float64 loop.
    float32 row (f32idx): the same loop in numpy float32 deviates from float64, on the CPU, by
    objective 1.3e-7 and consensus 2.8e-7 (relative, worst round) and x 9.7e-8 (max abs / max|ref|);
    each tolerance is 8 x that, for the GPU's other summation order."""
    ref = case(name)[4]
    eng = engine(name)
    obj, cons = run(eng, name, T)
    got = {"objective": obj, "consensus": cons, "x": eng.get_models()}
    eng.close()
    check(got, ref, TOL64 if CASES[name][1][0] == "float64" else TOL32)


def test_local_split_calls_bitwise():
    one = engine("x32")
    whole = run(one, "x32", T) + (one.get_models(),)
    one.close()
    two = engine("x32")
    first, second = run(two, "x32", 3), run(two, "x32", 3, t0=3)
    split = (np.concatenate([first[0], second[0]]), np.concatenate([first[1], second[1]]), two.get_models())
    two.close()
    for a, b in zip(whole, split):
        np.testing.assert_array_equal(a, b)


def test_trainer_local_steps():
    rounds, sizes, d, b, tau = 8, [14] * 9, 20, 5, 3
    cfg = dict(CFG, problem_type="logistic", local_batch_size=b, local_steps=tau)
    shards = make_shards("logistic", d, sizes, 3, False)
    Xf, yf = np.vstack([s[0] for s in shards]), np.concatenate([s[1] for s in shards])
    np.random.seed(21)
    state = np.random.get_state()
    idx = _dopt.mt_choice_rounds(rounds * tau, sizes, b)
    after = np.random.get_state()
    ref = local_reference("logistic", shards, topology.grid(9).dense_W(), rounds, tau, cfg, idx)
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
    now = np.random.get_state()
    assert now[2] == after[2] and np.array_equal(now[1], after[1])


@pytest.mark.parametrize("tau", [0, 65])
def test_local_steps_refused(tau):
    eng = engine("tau1")
    with pytest.raises(ValueError, match="local_steps"):
        eng.run_local(1, CFG["learning_rate_eta0"], 7, 0.0, 0.0, tau)
    eng.close()
