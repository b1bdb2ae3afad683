"""k_round_choco against k_round of the same build at the C3 shape (profiles/choco_round.txt):
HIP events around every round-kernel launch (dopt_set_profiling / dopt_kernel_stats), runs of 40 rounds
from zero iterates and zero public copies, one warm-up run per variant, then 7 repetitions with the
variants interleaved in one process; medians.  Usage: python tools/choco_round_probe.py [workers]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization_amd"))
import numpy as np  # noqa: E402

import _dopt  # noqa: E402
import topology  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
D, M, ROUNDS, REPS, ETA0, LAM, GAMMA = 1024, 512, 40, 7, 0.05, 1e-4, 0.4
KS = (102, 1024)

eng = _dopt.Engine(0, "float64", data_dtype="float32")
eng.generate_shards("logistic", N, D, M, seed=1)
top = topology.random_regular(N, 4, seed=0)
eng.set_topology(top.row_ptr, top.col, top.w)


def fresh():
    eng.zero_models()
    eng.choco_set_state(None)


def choco(k, rounds, wave_hist=False):
    os.environ["DOPT_CHOCO_WAVEHIST"] = "1" if wave_hist else "0"
    fresh()
    out = eng.run_choco(rounds, ETA0, M, LAM, LAM, k=k, gamma=GAMMA)
    return out + (eng.get_models(), eng.choco_get_state())


def timed(variant):
    fresh()
    eng.set_profiling(True, 1)
    eng.kernel_stats()
    if variant == "dsgd":
        eng.run_dsgd(ROUNDS, ETA0, M, LAM, LAM)
    else:  # k, or "<k>w" = the per-wave sub-histograms
        os.environ["DOPT_CHOCO_WAVEHIST"] = "1" if str(variant).endswith("w") else "0"
        eng.run_choco(ROUNDS, ETA0, M, LAM, LAM, k=int(str(variant).rstrip("w")), gamma=GAMMA)
    n, ms = eng.kernel_stats()
    eng.set_profiling(False)
    return ms / n, n


for k in KS:
    a, b, c = choco(k, 6), choco(k, 6), choco(k, 6, wave_hist=True)
    same = all(np.array_equal(x, y) for x, y in zip(a, b))
    same_w = all(np.array_equal(x, y) for x, y in zip(a, c))
    print(f"k = {k}: two runs of 6 rounds bitwise equal = {same}; shared vs per-wave histograms bitwise equal = "
          f"{same_w}  objective[5] = {float(a[0][5])!r}  consensus[5] = {float(a[1][5])!r}", flush=True)
variants = ("dsgd",) + KS + tuple(f"{k}w" for k in KS)
for v in variants:
    ms, n = timed(v)
    print(f"warm-up {v} {ms:.4f} ms over {n} launches  {_dopt.last_round_kernel()}", flush=True)
reps = {v: [] for v in variants}
for r in range(REPS):
    for v in variants:
        reps[v].append(timed(v)[0])
    print(f"rep {r} " + " ".join(f"{v} {reps[v][-1]:.4f}" for v in variants), flush=True)
med = {v: statistics.median(reps[v]) for v in variants}
# bytes by the project's counting: per worker the shard rows and labels (float32) and the iterate read and
# written (float64); CHOCO adds one xhat row read and one written per worker
dsgd_bytes = N * (4 * (M * D + M) + 8 * 2 * D)
choco_bytes = dsgd_bytes + N * 8 * 2 * D
print(f"C3 median ms per round kernel ({ROUNDS} launches x {REPS} interleaved reps): " +
      ", ".join(f"{v} {med[v]:.4f}" for v in variants))
for k in KS:
    print(f"per-wave / shared histograms at k = {k}: {med[f'{k}w'] / med[k]:.4f}; shared faster in "
          f"{sum(a < b for a, b in zip(reps[k], reps[f'{k}w']))} of {REPS} reps")
for k in KS:
    print(f"ratio choco(k = {k}) / dsgd = {med[k] / med['dsgd']:.4f} (byte ratio {choco_bytes / dsgd_bytes:.4f}); "
          f"choco slower in {sum(a > b for a, b in zip(reps[k], reps['dsgd']))} of {REPS} reps")
print(f"algorithmic bytes: dsgd {dsgd_bytes:.4e} -> {dsgd_bytes / med['dsgd'] / 1e9:.3f} TB/s; " +
      "; ".join(f"choco k = {k} {choco_bytes:.4e} -> {choco_bytes / med[k] / 1e9:.3f} TB/s" for k in KS))
eng.close()
