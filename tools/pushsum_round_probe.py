"""k_round_pushsum against k_round and k_round_gt of the same build at the C3 shape (profiles/pushsum_round.txt,
DESIGN.md 6k): HIP events around every round-kernel launch (dopt_set_profiling / dopt_kernel_stats), runs of
ROUNDS rounds from zero iterates with the metrics every round, one warm-up run per variant, then 7 repetitions
with the three variants interleaved in one process; medians.  D-SGD and gradient tracking mix through the
random 4-regular graph (Metropolis-Hastings weights), push-sum through random_digraph(N, 4): 5 N non-zeros each.
Usage: python tools/pushsum_round_probe.py [workers]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization_amd"))
import numpy as np  # noqa: E402

import _dopt  # noqa: E402
import topology  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
D, M, REPS, ROUNDS, ETA0, LAM = 1024, 512, 7, 40, 0.05, 1e-4

eng = _dopt.Engine(0, "float64", data_dtype="float32")
eng.generate_shards("logistic", N, D, M, seed=1)
UND = topology.random_regular(N, 4, seed=0)
DIR = topology.random_digraph(N, 4, seed=0)
DIR.check()
RUN = {"dsgd": eng.run_dsgd, "gt": eng.run_gt, "pushsum": eng.run_pushsum}


def run(variant, rounds):
    top = DIR if variant == "pushsum" else UND
    eng.set_topology(top.row_ptr, top.col, top.w)
    eng.zero_models()
    if variant == "gt":
        eng.gt_set_state(None, None)
    if variant == "pushsum":
        eng.pushsum_set_state(None)
    return RUN[variant](rounds, ETA0, M, LAM, LAM)


def timed(variant):
    """ms per round-kernel launch of one run."""
    eng.set_profiling(True, 1)
    eng.kernel_stats()
    run(variant, ROUNDS)
    n, ms = eng.kernel_stats()
    eng.set_profiling(False)
    return ms / n


a, b = run("pushsum", 6), run("pushsum", 6)
phi, _ = eng.pushsum_get_state()
print(f"C3 push-sum, 6 rounds twice: outputs bitwise equal = {all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2]))}  "
      f"objective[5] = {float(a[0][5])!r}  consensus[5] = {float(a[1][5])!r}  min phi = {phi.min():.4f}  "
      f"max phi = {phi.max():.4f}  sum phi - N = {phi.sum() - N:.3e}", flush=True)
variants = ("dsgd", "gt", "pushsum")
for v in variants:
    print(f"warm-up {v} {timed(v):.4f} ms {_dopt.last_round_kernel()}", flush=True)
ker = {v: [] for v in variants}
for rep in range(REPS):
    for v in variants:
        ker[v].append(timed(v))
    print(f"rep {rep} " + " ".join(f"{v} {ker[v][-1]:.4f}" for v in variants), flush=True)
mk = {v: statistics.median(ker[v]) for v in variants}
print(f"C3 median ms per round kernel ({ROUNDS} launches x {REPS} interleaved reps): " +
      ", ".join(f"{v} {mk[v]:.4f}" for v in variants))
# bytes by the project's counting: per worker the rows and labels (float32) and the iterate read and written
# once (float64); gradient tracking adds a y write and a g read + write, push-sum one more state row written
# (zt) and two weights
dsgd = N * (4 * (M * D + M) + 8 * 2 * D)
by = {"dsgd": dsgd, "gt": dsgd + N * 8 * 3 * D, "pushsum": dsgd + N * 8 * D + 2 * N * 8}
for v in variants:
    print(f"algorithmic bytes {v} {by[v]:.4e} -> {by[v] / mk[v] / 1e9:.3f} TB/s ({by[v] / mk[v] / 1e9 / 8:.3f} of 8 TB/s)")
for base in ("dsgd", "gt"):
    print(f"ratio pushsum / {base} = {mk['pushsum'] / mk[base]:.4f} (byte ratio {by['pushsum'] / by[base]:.4f}); pushsum faster "
          f"in {sum(x < y for x, y in zip(ker['pushsum'], ker[base]))} of {REPS} reps")
eng.close()
