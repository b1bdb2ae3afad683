"""k_round_sparse at an rcv1-like shape (profiles/sparse_round.txt): synthetic CSR shards, 4096 workers
x 512 rows, d = 47 236, about 75 non-zeros per row (74 draws from a power-law column distribution, duplicates
dropped, plus a bias column), random 4-regular graph, float64 iterates over float32 values.  HIP events around the
launches of every round (dopt_set_profiling / dopt_kernel_stats), runs of 10 rounds from zero iterates, one warm-up
run per variant, then 7 repetitions with the variants interleaved in one process; medians.  Variants: the hybrid
column split at the built threshold with the objective fused (full batches) and without it, every support column
by a wave (DOPT_SPARSE_ALLWAVE=1), and two other thresholds (DOPT_SPARSE_LONG at load).
Usage: python tools/sparse_round_probe.py [workers]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization_amd"))
import numpy as np  # noqa: E402

import _dopt  # noqa: E402
import topology  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
D, M, PER_ROW, ROUNDS, REPS, ETA0, LAM, DEG = 47236, 512, 74, 10, 7, 0.05, 1e-4, 4
HBM = 8e12  # MI355X bytes/s (vendor figure)

top = topology.random_regular(N, DEG, seed=0)
rng = np.random.default_rng(1)
rows = N * M
# column = (d - 1) u^3: a third of the draws fall into the first 4 % of the columns; the last column is the bias
cols = np.sort(((D - 1) * rng.random((rows, PER_ROW), dtype=np.float32) ** 3).astype(np.int32), axis=1)
keep = np.ones(cols.shape, dtype=bool)
keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
cols = np.concatenate([cols, np.full((rows, 1), D - 1, np.int32)], axis=1)
keep = np.concatenate([keep, np.ones((rows, 1), bool)], axis=1)
indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
indices = cols[keep]
del cols, keep
data = rng.standard_normal(indices.shape[0], dtype=np.float32) / np.float32(np.sqrt(PER_ROW))
data[indptr[1:] - 1] = 1.0
y = np.where(rng.random(rows) < 0.5, -1.0, 1.0).astype(np.float32)
off = np.arange(N + 1, dtype=np.int64) * M
nnz = int(indptr[-1])
# support columns per worker: counted on the first 64 workers
ns = float(np.mean([np.unique(indices[indptr[off[i]]:indptr[off[i + 1]]]).size for i in range(min(N, 64))]))
print(f"shape: {N} workers x {M} rows, d = {D}, nnz = {nnz} ({nnz / rows:.1f} per row), support columns per worker "
      f"{ns:.0f} (mean of the first {min(N, 64)} workers)", flush=True)


def engine(long_min):
    if long_min:
        os.environ["DOPT_SPARSE_LONG"] = str(long_min)
    e = _dopt.Engine(0, "float64", data_dtype="float32")
    e.load_shards_csr("logistic", indptr, indices, data, y, off, D)
    os.environ.pop("DOPT_SPARSE_LONG", None)
    e.set_topology(top.row_ptr, top.col, top.w)
    return e


base = engine(0)
# variant -> (engine, objective on, all-wave arm)
VARIANTS = {"hybrid": (base, True, False), "hybrid step": (base, False, False), "all-wave step": (base, False, True),
            "long>=8 step": (engine(8), False, False), "long>=128 step": (engine(128), False, False)}
del indices, data


def timed(v):
    e, objective, all_wave = VARIANTS[v]
    os.environ["DOPT_SPARSE_ALLWAVE"] = "1" if all_wave else "0"
    e.zero_models()
    e.set_profiling(True, 1)
    e.kernel_stats()
    e.run_sparse(ROUNDS, ETA0, M, LAM, LAM, objective=objective)
    n, ms = e.kernel_stats()
    e.set_profiling(False)
    return ms / n, n


os.environ["DOPT_SPARSE_ALLWAVE"] = "0"
base.zero_models()
a = base.run_sparse(6, ETA0, M, LAM, LAM)
base.zero_models()
b = base.run_sparse(6, ETA0, M, LAM, LAM)
print(f"two runs of 6 rounds bitwise equal = {all(np.array_equal(p, q) for p, q in zip(a[:2], b[:2]))}  "
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
print(f"median ms per launch ({ROUNDS} rounds x {REPS} interleaved reps): " + ", ".join(f"{v} {med[v]:.4f}" for v in VARIANTS))
# algorithmic bytes of a step launch, float64 state (8 B) over float32 values (4 B), ld = the padded row:
#   phase 2  (DEG + 1) state rows read (the CSR row of W, diagonal included) + 1 written: N (DEG + 2) ld 8
#   phase 3  per support column DEG + 1 neighbour elements + x_i[c] read, x_new[c] written:  N ns (DEG + 3) 8
#   row view     nnz (4 col + 4 val + 8 gathered x_i[col]) + rows (8 row_ptr + 4 label); the objective adds nnz 8 (xbar[col])
#   column view  nnz (4 srow + 4 sval) + N ns (4 scol + 4 sptr)
#   r            rows 8 written + nnz 8 read -- in LDS, listed but not counted against HBM
ld = (D + 3) // 4 * 4
p2, p3 = N * (DEG + 2) * ld * 8, N * ns * (DEG + 3) * 8
rv, cv, rl = nnz * 16 + rows * 12, nnz * 8 + N * ns * 8, rows * 8 + nnz * 8
print(f"bytes per step launch: phase 2 {p2:.4e}, phase 3 {p3:.4e}, row view {rv:.4e} (+ {nnz * 8:.4e} with the objective), "
      f"column view {cv:.4e}; r in LDS {rl:.4e}")
for v, (e, objective, _) in VARIANTS.items():
    bts = p2 + p3 + rv + cv + (nnz * 8 if objective else 0)
    t = med[v] * 1e-3
    print(f"{v}: {med[v]:.4f} ms; algorithmic HBM bytes {bts:.4e} -> {bts / t / 1e12:.3f} TB/s = {bts / t / HBM:.3f} of 8 TB/s "
          f"({bts / HBM * 1e3:.3f} ms at the peak)")
for e in {id(v[0]): v[0] for v in VARIANTS.values()}.values():
    e.close()
