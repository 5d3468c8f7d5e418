"""CPU: the chunked staging driver (electionguard-remote_amd/csrc/eg_stage.hpp) that the host and
_dev variants of the codes, contest-data, range and pre-encryption entry points share, driven by
memcpy-backed operations that count their calls (tests/cpp/stage_test.cpp): n in {1, 3, 4, 5, 11}
at a chunk of 4, columns of 1, 32 and 1,024 bytes per item, one once-per-call column and one null
optional output, in host and in device mode.  The callable must see exactly the caller's bytes of
its chunk, outputs must land at i0 * stride between intact guard bytes, the once column is uploaded
once, host mode synchronises once per chunk and device mode calls no operation at all, column
offsets are 256-byte multiples, and a failing callable or copy ends the run with its status before
any later copy."""
import json
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_staging_driver_with_counting_memcpy_operations(tmp_path):
    exe = tmp_path / "stage_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", str(ROOT / "electionguard-remote_amd" / "csrc"),
                    "-o", str(exe), str(ROOT / "tests" / "cpp" / "stage_test.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout)
    assert res == {"cases": 15, "failures": 0}, (res, r.stderr)
