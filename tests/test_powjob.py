"""CPU: the k_pow job record and launch shapes (electionguard-remote_amd/csrc/eg_powjob.hpp), by
tests/cpp/powjob_test.cpp: PowJob's named fields sit at the nine word offsets the kernel reads, an
untouched job is nine kNone, and every named shape constructor is memcmp-equal to the PowShape its
sites used to fill field by field, which pins the key of the schedule cache."""
import json
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_job_layout_and_named_shapes(tmp_path):
    exe = tmp_path / "powjob_test"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", str(ROOT / "electionguard-remote_amd" / "csrc"),
                    "-o", str(exe), str(ROOT / "tests" / "cpp" / "powjob_test.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout)
    assert res["failures"] == 0 and res["cases"] == 41, (res, r.stderr)
