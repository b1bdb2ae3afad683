"""k_round_local against k_round of the same build at the C3 shape (profiles/local_round.txt):
HIP events around every round-kernel launch (dopt_set_profiling / dopt_kernel_stats) and the device
stamps at the end of every round (which also cover the column-sum launch), runs from zero iterates,
one warm-up run per variant, then 7 repetitions with the variants interleaved in one process; medians.
  (a) full-shard batches, tau = 4: one local round against 4 D-SGD rounds
  (b) b = 16, tau = 8, host indices: one local round against 8 D-SGD rounds at b = 16
  (c) the prefetch across the reduction barrier (DOPT_LOCAL_PREFETCH) on and off, and their bits
Usage: python tools/local_round_probe.py [workers]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization_amd"))
import numpy as np  # noqa: E402

import _dopt  # noqa: E402
import topology  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
D, M, REPS, ETA0, LAM = 1024, 512, 7, 0.05, 1e-4
TAU_A, ROUNDS_A = 4, 12   # (a): 12 local rounds = 48 gradient steps
B, TAU_B, ROUNDS_B = 16, 8, 12  # (b): 12 local rounds = 96 gradient steps

eng = _dopt.Engine(0, "float64", data_dtype="float32")
eng.generate_shards("logistic", N, D, M, seed=1)
top = topology.random_regular(N, 4, seed=0)
eng.set_topology(top.row_ptr, top.col, top.w)
np.random.seed(5)
IDX = _dopt.mt_choice_rounds(ROUNDS_B * TAU_B, np.full(N, M, dtype=np.int64), B)


def local(rounds, tau, prefetch, idx=None, batch=M):
    os.environ["DOPT_LOCAL_PREFETCH"] = "1" if prefetch else "0"
    eng.zero_models()
    out = eng.run_local(rounds, ETA0, batch, LAM, LAM, tau, idx=None if idx is None else idx[:rounds * tau])
    return out[:2] + (eng.get_models(),)


def timed(variant):
    """(ms per round-kernel launch, ms per round between the device stamps, launches) of one run."""
    eng.zero_models()
    eng.set_profiling(True, 1)
    eng.kernel_stats()
    if variant == "dsgd_full":
        tim = eng.run_dsgd(ROUNDS_A * TAU_A, ETA0, M, LAM, LAM)[2]
    elif variant == "dsgd_b16":
        tim = eng.run_dsgd(ROUNDS_B * TAU_B, ETA0, B, LAM, LAM, idx=IDX)[2]
    else:  # "a0" / "a1" / "b0" / "b1": the case and the prefetch arm
        os.environ["DOPT_LOCAL_PREFETCH"] = variant[1]
        if variant[0] == "a":
            tim = eng.run_local(ROUNDS_A, ETA0, M, LAM, LAM, TAU_A)[2]
        else:
            tim = eng.run_local(ROUNDS_B, ETA0, B, LAM, LAM, TAU_B, idx=IDX)[2]
    n, ms = eng.kernel_stats()
    eng.set_profiling(False)
    return ms / n, 1e3 * (tim[-1] - tim[0]) / (len(tim) - 1), n


for name, args in (("a", (6, TAU_A, None, M)), ("b", (6, TAU_B, IDX, B))):
    on, on2, off = (local(args[0], args[1], p, args[2], args[3]) for p in (True, True, False))
    print(f"({name}) two runs of 6 rounds bitwise equal = {all(np.array_equal(x, y) for x, y in zip(on, on2))}; "
          f"prefetch on vs off bitwise equal = {all(np.array_equal(x, y) for x, y in zip(on, off))}  "
          f"objective[5] = {float(on[0][5])!r}  consensus[5] = {float(on[1][5])!r}", flush=True)
variants = ("dsgd_full", "a1", "a0", "dsgd_b16", "b1", "b0")
for v in variants:
    k, r, n = timed(v)
    print(f"warm-up {v} kernel {k:.4f} ms, round {r:.4f} ms over {n} launches  {_dopt.last_round_kernel()}", flush=True)
ker, rnd = {v: [] for v in variants}, {v: [] for v in variants}
for rep in range(REPS):
    for v in variants:
        k, r, _ = timed(v)
        ker[v].append(k)
        rnd[v].append(r)
    print(f"rep {rep} " + " ".join(f"{v} {ker[v][-1]:.4f}/{rnd[v][-1]:.4f}" for v in variants), flush=True)
mk = {v: statistics.median(ker[v]) for v in variants}
mr = {v: statistics.median(rnd[v]) for v in variants}
print(f"C3 median ms, round kernel / whole round (kernel + column sums), {REPS} interleaved reps: " +
      ", ".join(f"{v} {mk[v]:.4f}/{mr[v]:.4f}" for v in variants))
# bytes by the project's counting: per worker the rows and labels a step reads (float32) and the iterate
# read and written once per launch (float64); a local round reads tau batches and one state round trip
state = 8 * 2 * D
for name, tau, rows, base in (("a", TAU_A, M, "dsgd_full"), ("b", TAU_B, B, "dsgd_b16")):
    lb, db = N * (tau * 4 * (rows * D + rows) + state), tau * N * (4 * (rows * D + rows) + state)
    best = min((f"{name}1", f"{name}0"), key=lambda v: mk[v])
    print(f"({name}) tau = {tau}: local kernel {mk[name + '1']:.4f} ms vs {tau} x k_round {tau * mk[base]:.4f} ms = "
          f"{mk[name + '1'] / (tau * mk[base]):.4f}; whole round {mr[name + '1']:.4f} vs {tau} x {mr[base]:.4f} = "
          f"{mr[name + '1'] / (tau * mr[base]):.4f}; gradient-row byte ratio {lb / db:.4f}; local kernel "
          f"{lb / mk[name + '1'] / 1e9:.3f} TB/s of its gradient rows; faster arm {best}")
    print(f"({name}) prefetch on / off kernel = {mk[name + '1'] / mk[name + '0']:.4f}; on faster in "
          f"{sum(x < y for x, y in zip(ker[name + '1'], ker[name + '0']))} of {REPS} reps")
eng.close()
