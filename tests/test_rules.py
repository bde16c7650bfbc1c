"""csrc/dq_rules.h on the CPU: the rules the kernels and the engine share
(split threshold, cut choice, FP64 2-means decision, fixed-point corner test,
child-box clip, record tiling), compiled without HIP and checked against
their definitions written out in tests/native/rules_check.cpp.

The device's float-reciprocal division cannot run here; on the GPU the tiling
stays pinned by the count check of every planned round (Engine::finish_round).
"""
import os
import subprocess

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_rules_header_matches_definitions(tmp_path):
    exe = str(tmp_path / "rules_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(NATIVE, "rules_check.cpp")], timeout=120)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " mismatches 0" in res.stdout
