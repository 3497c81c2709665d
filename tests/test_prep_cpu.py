"""Scene preparation (csrc/rt_scene_prep.cpp), host only (no GPU): scripts/check_scene_prep.cpp runs it under the
address and undefined-behaviour sanitizers over fourteen scenes and every upload-time option, asserts the trees'
invariants, and prints one digest line per run of everything rt_scene_upload copies to the device.
tests/golden/prep_digests.txt pins those lines: a change to a builder that still yields a valid tree renders the
same pixels, and shows here."""
import os
import re
import subprocess

import pytest

from raytracing_gpu_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_gpu_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"  # build_qtree uses _Float16, which g++ 11 does not have


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("prep") / "check_scene_prep"
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "scripts", "check_scene_prep.cpp"),
                    *[os.path.join(CSRC, f) for f in ("rt_scene_prep.cpp", "rt_scene.cpp", "rt_obj.cpp", "rt_image.cpp",
                                                      "rt_validate.cpp")], "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_invariants_hold_and_sanitizers_are_silent(run):
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert not re.search(r"runtime error|Sanitizer", run.stderr), run.stderr[-2000:]
    assert not run.stderr.strip(), run.stderr[-2000:]


def test_digests_equal_the_golden_lines(run):
    want = open(os.path.join(ROOT, "tests", "golden", "prep_digests.txt")).read().splitlines()
    got = run.stdout.splitlines()
    assert len(want) >= 14 and [ln.split("/")[0] for ln in want if "/default:" in ln] == [
        "basic", "first", "big1", "two_spheres", "two_perlin", "cornell", "cornell_smoke", "triangle", "triangles",
        "coincident", "coincident_step", "earth", "door", "final"]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {k + 1}: {g.split(':')[0]} differs from the golden {w.split(':')[0]}"
    assert len(got) == len(want)


def test_prep_file_has_no_hip_include():
    """The unit links into a stand-alone program: no HIP header in its file or its header."""
    for f in ("rt_scene_prep.cpp", "rt_scene_prep.h", "rt_host_geom.h"):
        src = open(os.path.join(CSRC, f)).read()
        assert not re.search(r'#\s*include\s*[<"]hip', src), f
    assert "int prepare(" in open(os.path.join(CSRC, "rt_scene_prep.cpp")).read()


def test_prep_is_built_into_the_library():
    assert "rt_scene_prep.cpp" in _build.HIP_SOURCES and "rt_scene_prep.h" in _build.HIP_DEPS


def test_builders_left_the_kernel_file():
    src = open(os.path.join(CSRC, "rt_kernels.hip")).read()
    assert not [n for n in ("SahBuilder", "build_qtree", "build_world_tree") if n in src]
    assert "rtprep::prepare(" in src
