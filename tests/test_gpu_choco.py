"""CHOCO-SGD (dopt_run_choco, k_round_choco) against a plain float64 numpy loop of the recursion
  x_new = x - eta_t g + gamma (W xhat - xhat);  xhat <- xhat + top_k(x_new - xhat);  x <- x_new   (xhat = 0 at t = 0)
with the selection by a stable argsort of -|v| (equal magnitudes: the lower column wins).
float64 arithmetic (either row storage): the project's parity tolerance, rtol 1e-9 with atol
1e-12 max|ref|.  float32: see test_choco_matches_reference."""
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
GAMMA = 0.4
CFG = {"learning_rate_eta0": 0.05, "l2_regularization_lambda": 1e-4, "strong_convexity_mu": 1e-3}
TOL64 = dict.fromkeys(("objective", "consensus", "x", "xhat"), (1e-9, 1e-12))
# float32 row: 8 x the deviations in test_choco_matches_reference's docstring, as (rtol, atol / max|ref|)
TOL32 = {"objective": (8 * 1.6e-7, 0.0), "consensus": (8 * 1.4e-7, 0.0), "x": (0.0, 8 * 6.7e-8),
         "xhat": (0.0, 8 * 9.2e-8)}

#        problem      engine dtypes            d     shard sizes            batch  graph  k  seed  margin
CASES = {
    "x32": ("logistic", ("float64", "float32"), 1024, [24] * 64, None, lambda: topology.random_regular(64, 4),
            128, 14, 1e-6),
    "ragged": ("quadratic", ("float64", None), 200, [0, 5, 9, 33] * 4, None, lambda: topology.ring(16), 1, 11, 1e-6),
    "f32idx": ("logistic", ("float32", None), 77, [11] * 12, 4, lambda: topology.fully_connected(12), 10, 13, 1e-4),
    "cpl16": ("logistic", ("float64", None), 2048, [9] * 8, None, lambda: topology.ring(8), 300, 13, 1e-6),
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


def choco_reference(problem, shards, W, rounds, cfg, k, gamma, idx=None, dtype=np.float64, x0=None):
    """The recursion, and the reference's own selection margin: the minimum over workers and rounds
    of (|v|_(k) - |v|_(k+1)) / |v|_(k), wherever k < d and |v|_(k) > 0."""
    Xs = [(X.astype(dtype), y.astype(dtype)) for X, y in shards]
    Xf, yf = np.vstack([s[0] for s in Xs]), np.concatenate([s[1] for s in Xs])
    W = W.astype(dtype)
    d = Xf.shape[1]
    x = np.zeros((len(shards), d), dtype=dtype) if x0 is None else x0.astype(dtype)
    xhat = np.zeros_like(x)
    out = {"objective": [], "consensus": [], "margin": np.inf, "selected": []}
    for t in range(rounds):
        g = np.zeros_like(x)
        for i, (X, yv) in enumerate(Xs):
            sel = slice(None) if idx is None else idx[t, i, :min(idx.shape[2], len(yv))]
            g[i] = O.gradient(problem, x[i], X[sel], yv[sel], cfg)
        x = x - dtype(cfg["learning_rate_eta0"] / np.sqrt(t + 1)) * g + dtype(gamma) * (W @ xhat - xhat)
        v = x - xhat
        order = np.argsort(-np.abs(v), axis=1, kind="stable")
        mag = np.take_along_axis(np.abs(v), order, axis=1)
        if k < d and np.any(mag[:, k - 1] > 0):
            ok = mag[:, k - 1] > 0
            out["margin"] = min(out["margin"], float(np.min((mag[ok, k - 1] - mag[ok, k]) / mag[ok, k - 1])))
        q = np.zeros_like(v)
        np.put_along_axis(q, order[:, :k], np.take_along_axis(v, order[:, :k], axis=1), axis=1)
        xhat = xhat + q
        out["selected"].append(np.sort(order[:, :k], axis=1))
        avg = x.mean(axis=0)
        out["consensus"].append(float(np.mean(np.sum((x - avg) ** 2, axis=1))))
        out["objective"].append(float(O.objective(problem, avg, Xf, yf, cfg["l2_regularization_lambda"])))
    out.update(x=x, xhat=xhat)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, shards, topology, minibatch indices or None, float64 reference) of a row, made once."""
    problem, dtypes, d, sizes, b, graph, k, seed, _ = CASES[name]
    shards = make_shards(problem, d, sizes, seed, "float32" in dtypes)
    top = graph()
    idx = None
    if b is not None:
        np.random.seed(7)
        idx = _dopt.mt_choice_rounds(T, sizes, b)
    cfg = dict(CFG, problem_type=problem)
    return problem, shards, top, idx, choco_reference(problem, shards, top.dense_W(), T, cfg, k, GAMMA, idx)


def engine(dtypes, problem, shards, top):
    eng = _dopt.Engine(0, dtypes[0], data_dtype=dtypes[1])
    off = np.concatenate([[0], np.cumsum([len(s[1]) for s in shards])])
    eng.load_shards(problem, np.vstack([s[0] for s in shards]), np.concatenate([s[1] for s in shards]), off)
    eng.set_topology(top.row_ptr, top.col, top.w)
    return eng


def run(eng, name, rounds, t0=0):
    problem, shards, _, idx, _ = case(name)
    b = CASES[name][4] or max(len(s[1]) for s in shards)
    lam = CFG["l2_regularization_lambda"] if problem == "logistic" else CFG["strong_convexity_mu"]
    return eng.run_choco(rounds, CFG["learning_rate_eta0"], b, lam, CFG["l2_regularization_lambda"], k=CASES[name][6],
                         gamma=GAMMA, t0=t0, idx=None if idx is None else idx[t0:t0 + rounds])


def check(got, ref, tol):
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        print(k, "max |got - ref| / max|ref| =", np.max(np.abs(np.asarray(got[k]) - r)) / np.max(np.abs(r)))
    for k, (rtol, atol) in tol.items():
        r = np.asarray(ref[k])
        np.testing.assert_allclose(got[k], r, rtol=rtol, atol=atol * np.max(np.abs(r)), err_msg=k)


@pytest.mark.parametrize("name", list(CASES))
def test_choco_matches_reference(name):
    """Every round's objective and consensus, the final x and xhat against the float64 loop, after
    the reference's own selection margin has been checked against the row's bound (a selection that
    flips under rounding swaps two entries of xhat of size |v|, which no tolerance covers).  On the
    CPU the margins are 2.0e-5 (x32), 3.3e-3 (ragged), 8.2e-4 (f32idx) and 6.4e-5 (cpl16).
    float32 row (f32idx): the same loop in numpy float32 makes the float64 loop's selections at
    every worker and round and deviates from it, on the CPU, by objective 1.6e-7 and consensus
    1.4e-7 (relative, worst round), x 6.7e-8, xhat 9.2e-8 (max abs / max|ref|); each tolerance is
    8 x that, for the GPU's other summation order."""
    problem, shards, top, _, ref = case(name)
    print("margin", ref["margin"])
    assert ref["margin"] >= CASES[name][8]
    eng = engine(CASES[name][1], problem, shards, top)
    obj, cons = run(eng, name, T)
    got = {"objective": obj, "consensus": cons, "x": eng.get_models(), "xhat": eng.choco_get_state()}
    eng.close()
    check(got, ref, TOL64 if CASES[name][1][0] == "float64" else TOL32)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_choco_topk_ties(dtype):
    """One round with eta0 = 0 from xhat = 0: v = x.  The models hold +-{1, 2, 3} / 8, about 100
    columns per magnitude, so the 37th place falls inside the group of 3 / 8: the lower columns
    win, bit for bit, and x does not move.  d = 300 leaves lanes of the workgroup without a chunk."""
    d, k = 300, 37
    shards = make_shards("logistic", d, [3] * 4, 5, False)
    top = topology.ring(4)
    x0 = np.random.default_rng(9).choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=(4, d)) / 8
    cfg = dict(CFG, problem_type="logistic", learning_rate_eta0=0.0)
    ref = choco_reference("logistic", shards, top.dense_W(), 1, cfg, k, GAMMA, x0=x0)
    assert ref["margin"] == 0.0  # the tie group straddles the k-th place
    eng = engine((dtype, None), "logistic", shards, top)
    eng.set_models(x0)
    eng.run_choco(1, 0.0, 3, 1e-4, 1e-4, k=k, gamma=GAMMA)
    x, xhat = eng.get_models(), eng.choco_get_state()
    eng.close()
    np.testing.assert_array_equal(xhat, ref["xhat"])
    np.testing.assert_array_equal(x, x0)


def test_choco_split_calls_bitwise():
    problem, shards, top, _, _ = case("x32")
    one = engine(CASES["x32"][1], problem, shards, top)
    whole = run(one, "x32", T) + (one.get_models(), one.choco_get_state())
    one.close()
    two = engine(CASES["x32"][1], problem, shards, top)
    first, second = run(two, "x32", 3), run(two, "x32", 3, t0=3)
    split = (np.concatenate([first[0], second[0]]), np.concatenate([first[1], second[1]]), two.get_models(),
             two.choco_get_state())
    two.close()
    for a, b in zip(whole, split):
        np.testing.assert_array_equal(a, b)


def test_trainer_choco():
    rounds, sizes, d, b, k = 8, [14] * 9, 20, 5, 4
    cfg = dict(CFG, problem_type="logistic", local_batch_size=b, algorithm="choco", compression_k=k,
               choco_gamma=GAMMA)
    shards = make_shards("logistic", d, sizes, 3, False)
    Xf, yf = np.vstack([s[0] for s in shards]), np.concatenate([s[1] for s in shards])
    np.random.seed(21)
    state = np.random.get_state()
    idx = _dopt.mt_choice_rounds(rounds, sizes, b)
    ref = choco_reference("logistic", shards, topology.grid(9).dense_W(), rounds, cfg, k, GAMMA, idx)
    assert ref["margin"] >= 1e-6
    np.random.set_state(state)
    workers = [Worker(i, {"X": X, "y": y}, b, d, cfg) for i, (X, y) in enumerate(shards)]
    tr = DecentralizedTrainer(workers, "grid", d, cfg)
    hist, avg = tr.run(rounds, Xf, yf)
    assert [len(hist[k]) for k in ("objective", "consensus_error", "time")] == [rounds] * 3
    got = {"objective": hist["objective"], "consensus": hist["consensus_error"],
           "x": np.stack([w.x for w in workers])}
    check(got, ref, {k: TOL64[k] for k in got})
    np.testing.assert_allclose(avg, ref["x"].mean(axis=0), rtol=1e-9, atol=1e-12 * np.max(np.abs(ref["x"])))
    assert tr.total_floats_transmitted == rounds * 2 * k * int(np.sum(tr.degrees))
