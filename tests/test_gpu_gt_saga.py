"""GT-SAGA (dopt_run_gt_saga, k_round_saga) against a plain float64 numpy loop of the recursion
  tab, gbar at x_0;  c = coef(x_i . row_j, y_j), s = sum_{j in B} (c_j - tab[j]) row_j,
  g' = s / nb + gbar + lam x;  gbar += s / m;  tab[B] = c;  y <- W y + g' - g;  x <- W x - eta_t y;  g <- g'
from x = y = g = 0.  float64 arithmetic (either row storage): the project's parity tolerance,
rtol 1e-9 with atol 1e-12 max|ref|.  float32: see test_gt_saga_matches_reference."""
import functools

import numpy as np
import pytest
from scipy.special import expit

import _dopt
import dsgd_oracle as O
import topology
from trainer import DecentralizedTrainer
from worker import Worker

pytestmark = pytest.mark.gpu
T = 6
CFG = {"learning_rate_eta0": 0.05, "l2_regularization_lambda": 1e-4, "strong_convexity_mu": 1e-3}
KEYS = ("objective", "consensus", "x", "y", "g", "tab", "gbar")
TOL64 = dict.fromkeys(KEYS, (1e-9, 1e-12))
# float32 row: 8 x the deviations in test_gt_saga_matches_reference's docstring, as (rtol, atol / max|ref|)
TOL32 = {"objective": (8 * 1.5e-7, 0.0), "consensus": (8 * 4.5e-7, 0.0), "x": (0.0, 8 * 1.2e-7), "y": (0.0, 8 * 2.0e-7),
         "g": (0.0, 8 * 7.9e-8), "tab": (0.0, 8 * 1.1e-7), "gbar": (0.0, 8 * 6.3e-8)}

#        problem      engine dtypes            d     shard sizes         b  graph                       const_step
CASES = {
    "x32": ("logistic", ("float64", "float32"), 1024, [24] * 64, 6, lambda: topology.random_regular(64, 4), False),
    "ragged": ("quadratic", ("float64", None), 200, [0, 5, 9, 33] * 4, 7, lambda: topology.ring(16), False),
    "f32": ("logistic", ("float32", None), 77, [11] * 12, 4, lambda: topology.random_regular(12, 3), False),
    "cpl16": ("logistic", ("float64", None), 2048, [9] * 8, 3, lambda: topology.ring(8), False),
    "const": ("logistic", ("float64", None), 64, [10] * 6, 3, lambda: topology.ring(6), True),
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


def coef(problem, z, y):
    return -y * expit(-y * z) if problem == "logistic" else z - y


def saga_reference(problem, shards, W, rounds, cfg, idx, const_step=False, dtype=np.float64):
    Xs = [(X.astype(dtype), y.astype(dtype)) for X, y in shards]
    Xf, yf = np.vstack([s[0] for s in Xs]), np.concatenate([s[1] for s in Xs])
    W = W.astype(dtype)
    lam = dtype(cfg["l2_regularization_lambda"] if problem == "logistic" else cfg["strong_convexity_mu"])
    x = np.zeros((len(shards), Xf.shape[1]), dtype=dtype)
    y, g = np.zeros_like(x), np.zeros_like(x)
    tab = [coef(problem, X @ x[i], yv) for i, (X, yv) in enumerate(Xs)]
    gbar = np.stack([t @ X / dtype(len(t)) if len(t) else np.zeros_like(x[0]) for t, (X, _) in zip(tab, Xs)])
    tab0 = np.concatenate(tab)
    out = {"objective": [], "consensus": []}
    for t in range(rounds):
        gn = np.zeros_like(x)
        for i, (X, yv) in enumerate(Xs):
            sel = idx[t, i, :min(idx.shape[2], len(yv))]
            if len(sel):
                cn = coef(problem, X[sel] @ x[i], yv[sel])
                s = (cn - tab[i][sel]) @ X[sel]
                gn[i] = s / dtype(len(sel)) + gbar[i] + lam * x[i]
                gbar[i] = gbar[i] + s / dtype(len(yv))
                tab[i][sel] = cn
        y = W @ y + gn - g
        x = W @ x - dtype(cfg["learning_rate_eta0"] / (1.0 if const_step else np.sqrt(t + 1))) * y
        g = gn
        avg = x.mean(axis=0)
        out["consensus"].append(float(np.mean(np.sum((x - avg) ** 2, axis=1))))
        out["objective"].append(float(O.objective(problem, avg, Xf, yf, cfg["l2_regularization_lambda"])))
    out.update(x=x, y=y, g=g, tab=np.concatenate(tab), gbar=gbar, tab0=tab0)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, shards, topology, minibatch indices, float64 reference) of a row, made once."""
    problem, dtypes, d, sizes, b, graph, const = CASES[name]
    shards = make_shards(problem, d, sizes, 11, "float32" in dtypes)
    top = graph()
    np.random.seed(7)
    idx = _dopt.mt_choice_rounds(T, sizes, b)
    cfg = dict(CFG, problem_type=problem)
    return problem, shards, top, idx, saga_reference(problem, shards, top.dense_W(), T, cfg, idx, const)


def engine(name):
    problem, shards, top, _, _ = case(name)
    dtype, data_dtype = CASES[name][1]
    eng = _dopt.Engine(0, dtype, data_dtype=data_dtype)
    off = np.concatenate([[0], np.cumsum([len(s[1]) for s in shards])])
    eng.load_shards(problem, np.vstack([s[0] for s in shards]), np.concatenate([s[1] for s in shards]), off)
    eng.set_topology(top.row_ptr, top.col, top.w)
    return eng


def run(eng, name, rounds, t0=0):
    """(objective, consensus) of the rounds, then x, y, g, tab, gbar after them."""
    problem, _, _, idx, _ = case(name)
    lam = CFG["l2_regularization_lambda"] if problem == "logistic" else CFG["strong_convexity_mu"]
    obj, cons, _ = eng.run_gt_saga(rounds, CFG["learning_rate_eta0"], CASES[name][4], lam, CFG["l2_regularization_lambda"],
                                   t0=t0, idx=idx[t0:t0 + rounds], const_step=CASES[name][6])
    return (obj, cons, eng.get_models()) + eng.gt_get_state() + eng.saga_get_state()


def check(got, ref, tol):
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        print(k, "max |got - ref| / max|ref| =", np.max(np.abs(np.asarray(got[k]) - r)) / np.max(np.abs(r)))
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        np.testing.assert_allclose(got[k], r, rtol=rtol, atol=atol * np.max(np.abs(r)), err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_gt_saga_matches_reference(name):
    """Every round's objective and consensus, the final x, y, g, tab and gbar against the float64 loop.
    float32 row (f32): the same loop in numpy float32 deviates from float64, on the CPU, by objective
    1.5e-7 and consensus 4.5e-7 (relative, worst entry), x 1.2e-7, y 2.0e-7, g 7.9e-8, tab 1.1e-7 and
    gbar 6.3e-8 (max abs / max|ref|); each tolerance is 8 x that, for the GPU's other summation order."""
    _, shards, _, idx, ref = case(name)
    # some row is drawn in two rounds, so an updated table entry is read back: a kernel that ignored
    # the table cannot pass
    used = [idx[:, i, :min(idx.shape[2], len(s[1]))].ravel() for i, s in enumerate(shards)]
    assert any(len(np.unique(u)) < len(u) for u in used)
    assert np.max(np.abs(ref["tab"] - ref["tab0"])) > 1e-3 * np.max(np.abs(ref["tab0"]))
    eng = engine(name)
    got = dict(zip(KEYS, run(eng, name, T)))
    eng.close()
    check(got, ref, TOL64 if CASES[name][1][0] == "float64" else TOL32)


def test_gt_saga_split_calls_bitwise():
    one = engine("x32")
    whole = run(one, "x32", T)
    one.close()
    two = engine("x32")
    first, second = run(two, "x32", 3), run(two, "x32", 3, t0=3)
    two.close()
    split = (np.concatenate([first[0], second[0]]), np.concatenate([first[1], second[1]])) + second[2:]
    for a, b in zip(whole, split):
        np.testing.assert_array_equal(a, b)


def test_trainer_gt_saga():
    rounds, sizes, d, b = 8, [14] * 9, 20, 5
    cfg = dict(CFG, problem_type="logistic", local_batch_size=b, algorithm="gt_saga", regular_degree=4)
    shards = make_shards("logistic", d, sizes, 3, False)
    Xf, yf = np.vstack([s[0] for s in shards]), np.concatenate([s[1] for s in shards])
    np.random.seed(21)
    state = np.random.get_state()
    idx = _dopt.mt_choice_rounds(rounds, sizes, b)
    np.random.set_state(state)
    workers = [Worker(i, {"X": X, "y": y}, b, d, cfg) for i, (X, y) in enumerate(shards)]
    tr = DecentralizedTrainer(workers, "random_regular", d, cfg)
    ref = saga_reference("logistic", shards, np.asarray(tr.W), rounds, cfg, idx)
    hist, avg = tr.run(rounds, Xf, yf)
    assert [len(hist[k]) for k in ("objective", "consensus_error", "time")] == [rounds] * 3
    got = {"objective": hist["objective"], "consensus": hist["consensus_error"],
           "x": np.stack([w.x for w in workers])}
    check(got, ref, {k: TOL64[k] for k in got})
    np.testing.assert_allclose(avg, ref["x"].mean(axis=0), rtol=1e-9, atol=1e-12 * np.max(np.abs(ref["x"])))
    assert tr.total_floats_transmitted == rounds * 2 * int(np.sum(tr.degrees)) * d
