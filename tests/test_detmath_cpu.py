"""CPU checks of the shared deterministic math (csrc/rt_detmath.h)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checker_sign_shortcut_matches_det_sinf(tmp_path):
    """sin_neg_fast == sign(det_sinf) on a strided sweep of every binade of 2^-20..2^17 (the
    exhaustive run, stride 1, checked all 620 756 994 floats: scripts/check_checker_sign.cpp)."""
    exe = tmp_path / "ccs"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off",
                    os.path.join(ROOT, "scripts", "check_checker_sign.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), "97"], check=True, capture_output=True, text=True).stdout
    assert "mismatches 0" in out, out
