"""CPU checks of bench.py's measurement helpers (no GPU): the algorithmic bytes per launch that
roofline.achieved divides by the kernel time (C3 8.665 GB, C4 138.6 GB,
C5 direct 77.3 GB, C5 row-space 68.72 GB), and the committed PMC summary each configuration's line
reads its traffic from (profiles/), which must sit within 2 % of those bytes (no re-reads)."""
import os
import sys
import types

import pytest

import _dopt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

F32, F64 = _dopt.F32, _dopt.F64
C3 = "void dopt::k_round<double, float, 4, 0, true, true, 161843>(dopt::RoundArgs)"
C5RS = "void dopt::k_rs_pass<float, true, 2, 6>(dopt::RsArgs)"
C5X32 = "void dopt::k_rs_pass_x32<true, 2, 6>(dopt::RsArgs)"
C5D = "void dopt::k_split_step<float, 4, true, true, true, 1>(dopt::RoundArgs)"  # round-2 spelling
C5DX = "void dopt::k_split_step<double, float, 4, true, true, true, 1>(dopt::RoundArgs)"


def _eng(dtype, xdtype):
    return types.SimpleNamespace(dtype=dtype, data_dtype=xdtype)


# (config, kernel, engine dtype, row storage, workers, d, m, GB in DESIGN.md, profile file)
CASES = [
    ("c3", C3, F64, F32, 4096, 1024, 512, 8.665, "profiles/r3_pmc.json"),
    ("c5", C5DX, F64, F32, 1024, 1 << 20, 16, 85.90, "profiles/r3_c5x32direct_pmc.json"),
    ("c4", C3, F64, F32, 65536, 1024, 512, 138.6, "profiles/r3_c4_pmc.json"),
    ("c5", C5D, F32, F32, 1024, 1 << 20, 16, 77.3, "profiles/r2_c5_pmc.json"),
    ("c5", C5RS, F32, F32, 1024, 1 << 20, 16, 68.72, "profiles/r2_c5rs_pmc.json"),
    ("c5", C5X32, F64, F32, 1024, 1 << 20, 16, 68.72, "profiles/r2_c5x32_pmc.json"),
]


@pytest.mark.parametrize("config,kernel,dt,xdt,n,d,m,gb,prof", CASES)
def test_bytes_and_committed_traffic(config, kernel, dt, xdt, n, d, m, gb, prof):
    b = bench.bytes_per_round(_eng(dt, xdt), n, d, m, kernel)
    assert abs(b / 1e9 - gb) < 0.01 * gb, b
    traffic, src, _ = bench.pmc_traffic(kernel, config)
    assert src == prof, src
    assert 1.0 <= traffic / b < 1.02, traffic / b


def test_dump_outputs_writes_float64_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: the timed rounds' metrics and the iterates as float64 .npy; iterates past the byte
    budget are cut to the same sorted worker rows in every run."""
    import numpy as np

    x = np.arange(40 * 8, dtype=np.float64).reshape(40, 8)
    eng = types.SimpleNamespace(get_models=lambda: x.copy())
    obj, cons = np.linspace(1.0, 0.5, 6), np.linspace(0.0, 0.1, 6)
    bench.dump_outputs(str(tmp_path / "a"), eng, obj, cons, 1, 0)
    assert sorted(os.listdir(tmp_path / "a")) == ["consensus.npy", "models.npy", "objective.npy"]
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("models", "objective", "consensus")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["models"], x) and np.array_equal(got["objective"], obj)
    assert np.array_equal(got["consensus"], cons)
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * 8 * 8)  # room for 10 of the 40 rows
    for k in "bc":
        bench.dump_outputs(str(tmp_path / k), eng, obj, cons, 1, 0)
    b, c = np.load(tmp_path / "b" / "models.npy"), np.load(tmp_path / "c" / "models.npy")
    assert b.shape == (10, 8) and np.array_equal(b, c)
    rows = (b[:, 0] / 8).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(b, x[rows])


def test_traffic_lookup_is_per_configuration():
    """C3 and C4 launch the same kernel instance: each line reads its own configuration's file."""
    t3, s3, _ = bench.pmc_traffic(C3, "c3")
    t4, s4, _ = bench.pmc_traffic(C3, "c4")
    assert s3 != s4 and t4 > 10 * t3
    assert bench.pmc_traffic("void dopt::k_no_such_kernel()", "c5") == (None, None, None)
