"""k_round_softmax against k_round of the same build at the C3 shape (profiles/softmax_round.txt):
HIP events around the launches of every round (dopt_set_profiling / dopt_kernel_stats), runs of 20 rounds from
zero iterates, one warm-up run per variant, then 7 repetitions with the variants interleaved in one process;
medians.  A softmax round with the objective on is two launches (the metrics launch at Wbar, then the step):
the event pair brackets both, and the run without the objective times the step launch alone.
Usage: python tools/softmax_round_probe.py [workers]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization_amd"))
import numpy as np  # noqa: E402

import _dopt  # noqa: E402
import topology  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
D, M, ROUNDS, REPS, ETA0, LAM = 1024, 512, 20, 7, 0.05, 1e-4
HBM, PEAK64, PEAK32 = 8e12, 78.6e12, 157.3e12  # MI355X: bytes/s, matrix FLOP/s in float64 and float32 (vendor figures)

top = topology.random_regular(N, 4, seed=0)
rng = np.random.default_rng(1)
X = rng.standard_normal((N * M, D), dtype=np.float32)
X[:, -1] = 1.0
y = rng.integers(0, 10, N * M).astype(np.float32)  # valid labels for C = 10 and C = 16
off = np.arange(N + 1, dtype=np.int64) * M


def softmax_engine(dtype, data_dtype, C):
    e = _dopt.Engine(0, dtype, data_dtype=data_dtype)
    e.load_shards("softmax", X, y, off, n_classes=C)
    e.set_topology(top.row_ptr, top.col, top.w)
    return e


dsgd = _dopt.Engine(0, "float64", data_dtype="float32")
dsgd.generate_shards("logistic", N, D, M, seed=1)
dsgd.set_topology(top.row_ptr, top.col, top.w)
# variant -> (engine, classes, objective on, bytes per state element)
ENG = {"x32 C=10": softmax_engine("float64", "float32", 10), "x32 C=16": softmax_engine("float64", "float32", 16),
       "f32 C=10": softmax_engine("float32", None, 10)}
del X, y
VARIANTS = {"dsgd": (dsgd, 1, True, 8)}
for name, e in ENG.items():
    C, sb = int(name.split("=")[1]), 4 if name.startswith("f32") else 8
    VARIANTS[name] = (e, C, True, sb)
    VARIANTS[name + " step"] = (e, C, False, sb)


def timed(v):
    e, C, objective, _ = VARIANTS[v]
    e.zero_models()
    e.set_profiling(True, 1)
    e.kernel_stats()
    if v == "dsgd":
        e.run_dsgd(ROUNDS, ETA0, M, LAM, LAM)
    else:
        e.run_softmax(ROUNDS, ETA0, M, LAM, LAM, objective=objective)
    n, ms = e.kernel_stats()
    e.set_profiling(False)
    return ms / n, n


for name, e in ENG.items():
    e.zero_models()
    a = e.run_softmax(6, ETA0, M, LAM, LAM)
    e.zero_models()
    b = e.run_softmax(6, ETA0, M, LAM, LAM)
    print(f"{name}: two runs of 6 rounds bitwise equal = {all(np.array_equal(p, q) for p, q in zip(a[:2], b[:2]))}  "
          f"objective[5] = {float(a[0][5])!r}  consensus[5] = {float(a[1][5])!r}", flush=True)
for v in VARIANTS:
    ms, n = timed(v)
    print(f"warm-up {v}: {ms:.4f} ms over {n} event pairs  {_dopt.last_round_kernel()}", flush=True)
reps = {v: [] for v in VARIANTS}
for r in range(REPS):
    for v in VARIANTS:
        reps[v].append(timed(v)[0])
    print(f"rep {r} " + "  ".join(f"{v} {reps[v][-1]:.4f}" for v in VARIANTS), flush=True)
med = {v: statistics.median(reps[v]) for v in VARIANTS}
print(f"C3 median ms per round ({ROUNDS} rounds x {REPS} interleaved reps): " + ", ".join(f"{v} {med[v]:.4f}" for v in VARIANTS))
# bytes by the project's counting: per worker the shard rows and labels (float32) once per launch that streams
# them, and the state row read and written (2 C ld elements); useful FLOPs: 2 m d C per product and worker
rows = N * 4 * (M * D + M)
for v, (e, C, objective, sb) in VARIANTS.items():
    if v == "dsgd":
        b = rows + N * 8 * 2 * D
        print(f"{v}: {med[v]:.4f} ms; algorithmic bytes {b:.4e} -> {b / med[v] / 1e9:.3f} TB/s = {b / med[v] / 1e-3 / HBM:.3f} of 8 TB/s")
        continue
    b = rows * (2 if objective else 1) + N * sb * 2 * C * D
    fl = N * 2 * M * D * C * (3 if objective else 2)
    peak = PEAK32 if sb == 4 else PEAK64
    t = med[v] * 1e-3
    print(f"{v}: {med[v]:.4f} ms = {med[v] / med['dsgd']:.3f} x k_round; algorithmic bytes {b:.4e} -> {b / t / 1e12:.3f} TB/s = "
          f"{b / t / HBM:.3f} of 8 TB/s; useful FLOPs {fl:.4e} -> {fl / t / 1e12:.2f} TFLOP/s = {fl / t / peak:.3f} of the "
          f"{peak / 1e12:.1f} TFLOP/s matrix peak; bound by {'HBM' if b / HBM > fl / peak else 'the matrix pipe'} on paper "
          f"({b / HBM * 1e3:.3f} ms vs {fl / peak * 1e3:.3f} ms)")
for e in list(ENG.values()) + [dsgd]:
    e.close()
