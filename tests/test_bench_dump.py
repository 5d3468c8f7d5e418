"""CPU: bench.py --dump-outputs writes float32 / float64 .npy files within its byte budget, and an
array over its share is cut to the same seeded rows on every run; the extra figures of the bench
line are off unless --full is given."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402


def test_dump_outputs_dtypes_budget_and_fixed_sample(tmp_path, monkeypatch):
    rng = np.random.default_rng(3)
    arrays = {"flags": rng.integers(0, 2, size=(5000, 24), dtype=np.uint8),
              "tally": rng.integers(0, 256, size=(20, 2, 512), dtype=np.uint8),
              "counts": np.arange(20, dtype=np.int64) * 100_003}
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 96_000)  # flags (480,000 bytes as float32) is over its share
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, arrays)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert got["flags"].dtype == np.float32 and got["tally"].dtype == np.float32 and got["counts"].dtype == np.float64
    assert np.array_equal(got["tally"], arrays["tally"]) and np.array_equal(got["counts"], arrays["counts"])
    assert got["flags"].shape == (1000, 24)  # 96,000 bytes / (24 x 4 bytes per row)
    assert sum(x.nbytes for x in got.values()) <= bench.DUMP_BYTES
    # the sample is rows of the input, in order, and the same rows in both runs
    rows = {r.tobytes() for r in arrays["flags"].astype(np.float32)}
    assert all(r.tobytes() in rows for r in got["flags"])
    for n in arrays:
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))


def test_full_is_off_by_default():
    assert bench.parse([]).full is False and bench.parse([]).dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "x"])
    assert a.full is True and a.dump_outputs == "x"
    assert bench.DUMP_BYTES <= 64_000_000
