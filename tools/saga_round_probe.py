"""k_round_saga against k_round_gt of the same build at the C3 shape (profiles/saga_round.txt): HIP
events around every round-kernel launch (dopt_set_profiling / dopt_kernel_stats), runs of ROUNDS rounds with the
metrics every round, one warm-up run per variant, then 7 repetitions with the variants interleaved in one
process; medians.  Legs: full-shard batches (b = m = 512), host minibatches of b = 16 rows, and the pass that
opens a GT-SAGA chain.  Every timed run continues a chain opened by one untimed round from zero iterates, so no
timed GT-SAGA run holds the opening pass; that pass is timed as (opening pass + one round) - (one round), each the
median of 7 single runs.  Both algorithms mix through the random 4-regular graph.
Usage: python tools/saga_round_probe.py [workers]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization_amd"))
import numpy as np  # noqa: E402

import _dopt  # noqa: E402
import topology  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
D, M, B, REPS, ROUNDS, ETA0, LAM = 1024, 512, 16, 7, 40, 0.05, 1e-4

eng = _dopt.Engine(0, "float64", data_dtype="float32")
eng.generate_shards("logistic", N, D, M, seed=1)
top = topology.random_regular(N, 4, seed=0)
eng.set_topology(top.row_ptr, top.col, top.w)
np.random.seed(5)
IDX = _dopt.mt_choice_rounds(ROUNDS + 1, [M] * N, B)
RUN = {"gt": eng.run_gt, "saga": eng.run_gt_saga}


def run(variant, b, rounds, t0=0):
    idx = None if b == M else IDX[t0:t0 + rounds]
    return RUN[variant](rounds, ETA0, b, LAM, LAM, idx=idx, t0=t0)


def fresh(variant):
    eng.zero_models()
    if variant == "saga":
        eng.saga_reset()
    else:
        eng.gt_set_state(None, None)


def stats(f):
    """(launches, ms) of the round-kernel launches f makes."""
    eng.set_profiling(True, 1)
    eng.kernel_stats()
    f()
    n, ms = eng.kernel_stats()
    eng.set_profiling(False)
    return n, ms


def timed(variant, b):
    """ms per round-kernel launch of ROUNDS rounds that continue a chain of one round."""
    fresh(variant)
    run(variant, b, 1)
    n, ms = stats(lambda: run(variant, b, ROUNDS, t0=1))
    assert n == ROUNDS
    return ms / n


def opening():
    """(ms of the opening pass + round 0, ms of round 1 of the chain), full-shard batches."""
    fresh("saga")
    n2, both = stats(lambda: run("saga", M, 1))
    n1, one = stats(lambda: run("saga", M, 1, t0=1))
    assert (n2, n1) == (2, 1)
    return both, one


fresh("saga")
a = run("saga", B, 6)
fresh("saga")
b2 = run("saga", B, 6)
tab, gbar = eng.saga_get_state()
print(f"C3 GT-SAGA b = {B}, 6 rounds twice: outputs bitwise equal = "
      f"{all(np.array_equal(x, y) for x, y in zip(a[:2], b2[:2]))}  objective[5] = {float(a[0][5])!r}  "
      f"consensus[5] = {float(a[1][5])!r}  max |tab| = {np.abs(tab).max():.4f}  max |gbar| = {np.abs(gbar).max():.4e}",
      flush=True)
legs = [(v, b) for b in (M, B) for v in ("gt", "saga")]
for v, b in legs:
    print(f"warm-up {v} b={b} {timed(v, b):.4f} ms {_dopt.last_round_kernel()}", flush=True)
ker = {leg: [] for leg in legs}
op = []
for rep in range(REPS):
    for leg in legs:
        ker[leg].append(timed(*leg))
    op.append(opening())
    print(f"rep {rep} " + " ".join(f"{v}/b={b} {ker[(v, b)][-1]:.4f}" for v, b in legs) +
          f" opening+round {op[-1][0]:.4f} round {op[-1][1]:.4f}", flush=True)
mk = {leg: statistics.median(ker[leg]) for leg in legs}
m_open = statistics.median(x for x, _ in op) - statistics.median(y for _, y in op)
print(f"C3 median ms per round kernel ({ROUNDS} launches x {REPS} interleaved reps): " +
      ", ".join(f"{v}/b={b} {mk[(v, b)]:.4f}" for v, b in legs) + f"; opening pass {m_open:.4f}")


# bytes by the project's counting: per worker the batch rows and labels (float32), the iterate read and written
# (float64), gradient tracking's y write and g read + write; host minibatches add their indices; GT-SAGA adds gbar
# read + written and the batch's table entries read + written (float64)
def gt_bytes(b):
    return N * (4 * (b * D + b) + 8 * 5 * D + (4 * b if b != M else 0))


def saga_bytes(b):
    return gt_bytes(b) + N * (8 * 2 * D + 2 * 8 * b)


open_bytes = N * (4 * (M * D + M) + 8 * 2 * D + 8 * M)  # rows, labels, x read, gbar and the table written
for b in (M, B):
    tg, ts = mk[("gt", b)], mk[("saga", b)]
    print(f"b={b}: bytes gt {gt_bytes(b):.4e} -> {gt_bytes(b) / tg / 1e9:.3f} TB/s, saga {saga_bytes(b):.4e} -> "
          f"{saga_bytes(b) / ts / 1e9:.3f} TB/s; ratio saga / gt = {ts / tg:.4f} (byte ratio "
          f"{saga_bytes(b) / gt_bytes(b):.4f}); saga faster in "
          f"{sum(x < y for x, y in zip(ker[('saga', b)], ker[('gt', b)]))} of {REPS} reps")
print(f"opening pass: bytes {open_bytes:.4e} -> {open_bytes / m_open / 1e9:.3f} TB/s; ratio to gt/b={M} = "
      f"{m_open / mk[('gt', M)]:.4f} (byte ratio {open_bytes / gt_bytes(M):.4f})")
eng.close()
