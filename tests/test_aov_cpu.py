"""Feature planes averaged over lens, footprint and shutter samples, host side (no GPU): the rt_aov_* ABI is
declared, exported and bound as a closed set; rt_aov_pattern equals the numpy restatement of tests/aov_ref.py bit
for bit; rt_aov_render_host equals numpy rays cast through rt.cast_host and summed in sample order, byte for byte
in all five planes; one sample without lens and shutter is rt_guide_render_host; coverage is hits / samples."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import aov_ref as ar
import guide_cases as gc
from flat_scenes import FlatScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_gpu_amd", "csrc")
F32 = np.float32
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
W, H = 24, 16
SCENES = ["big1", "cornell", "world_medium_over_xform", "tri_flat"]
INT_NAMES = ["rt_aov_pattern", "rt_aov_render", "rt_aov_coverage", "rt_aov_render_host"]


# ---------------------------------------------------------------- ABI and sources
def test_aov_abi_declared_exported_bound(rtlib):
    hdr = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert set(re.findall(r"^\s*int\s+(rt_aov_\w+)\s*\(", hdr, re.M)) == set(INT_NAMES)
    assert re.findall(r"^\s*float\s+(rt_aov_\w+)\s*\(", hdr, re.M) == ["rt_aov_last_ms"]
    assert re.findall(r"^\s*void\s+(rt_aov_\w+)\s*\(", hdr, re.M) == ["rt_aov_params_default"]
    L = rtlib.lib()
    names = INT_NAMES + ["rt_aov_last_ms", "rt_aov_params_default"]
    for n in names:
        assert hasattr(L, n) and n in rtlib.ABI, n
    assert sorted(n for n in rtlib.ABI if n.startswith("rt_aov_")) == sorted(names)
    assert ctypes.sizeof(rtlib.rt_aov_params) == 16
    assert rtlib.aov_params().as_dict() == {"samples": 16, "lens": 1, "footprint": 1, "shutter": 1}
    assert rtlib.aov_params(samples=3, lens=False).as_dict() == {"samples": 3, "lens": 0, "footprint": 1, "shutter": 1}
    with pytest.raises(TypeError):
        rtlib.aov_params(aperture=1)
    # the closed families and pinned sizes beside it are as they were
    assert ctypes.sizeof(rtlib.rt_guide_params) == 16 and ctypes.sizeof(rtlib.rt_denoise_params) == 24


def test_aov_sources_share_one_definition():
    """The twin is host only, both halves compile csrc/rt_aov.h, whose pattern has no HIP include."""
    from raytracing_gpu_amd import _build

    twin = open(os.path.join(CSRC, "rt_guide_host.cpp")).read()
    dev = open(os.path.join(CSRC, "rt_guide.hip")).read()
    core = open(os.path.join(CSRC, "rt_aov.h")).read()
    assert not re.search(r'#\s*include\s*[<"]hip', twin) and not re.search(r'#\s*include\s*[<"]hip', core)
    for src in (twin, dev):
        assert '#include "rt_aov.h"' in src and "rtaov::pixel(" in src and "rtaov::pattern(" in src
    assert "rtfh::cast(" in core and "aov_render_kernel" in dev
    assert "rt_aov.h" in _build.HIP_DEPS


def test_check_aov_host_program_builds_and_passes(tmp_path):
    """scripts/check_aov_host.cpp: the twin on images smaller than a tile, 1, 2, 5 and 256 samples, every switch
    combination and every refusal, in a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "check_aov_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "scripts", "check_aov_host.cpp"), os.path.join(CSRC, "rt_guide_host.cpp"),
                    os.path.join(CSRC, "rt_validate.cpp"),
                    *[os.path.join(CSRC, f"rt_{x}_blob.cpp") for x in ("accum", "noise", "adapt", "denoise")], "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_aov_host ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- the pattern
@pytest.mark.parametrize("S", [1, 2, 3, 5, 16, 64, 256])
def test_pattern_is_the_definitions(rtlib, S):
    for sw in [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)]:
        got = rtlib.aov_pattern(samples=S, lens=sw[0], footprint=sw[1], shutter=sw[2])
        want = ar.pattern(S, *sw)
        assert got.shape == (S, 5) and got.tobytes() == want.tobytes(), sw
        assert (got[:, 2].astype(np.float64) ** 2 + got[:, 3].astype(np.float64) ** 2 <= 1.0 + 1e-7).all()
        if sw[0]:
            assert len(np.unique(got[:, 2:4], axis=0)) == S
        else:
            assert (got[:, 2:4] == 0).all()
        if sw[1]:
            assert (np.diff(got[:, 0]) > 0).all() and len(np.unique(got[:, 1])) == S
            assert ((got[:, :2] > 0) & (got[:, :2] < 1)).all()
        else:
            assert (got[:, :2] == F32(0.5)).all()
        assert (got[:, 4] == F32(0.5)).all() if not sw[2] else (len(np.unique(got[:, 4])) == S and (got[:, 4] < 1).all())
    one = rtlib.aov_pattern(samples=1)
    assert one[0, 0] == F32(0.5) and one[0, 1] == F32(0.5)


# ---------------------------------------------------------------- the planes
@pytest.mark.parametrize("S", [1, 2, 5, 16])
@pytest.mark.parametrize("name", SCENES)
def test_host_twin_equals_numpy_rays_through_cast_host(rtlib, name, S):
    got = ar.host_planes(name, W, H, S)
    want = ar.planes(gc.soa(name), W, H, S)
    assert not ar.same_planes(got, want)
    assert (got["prim"] >= 0).any()
    if name == "big1" and S > 1:  # the lens and the footprint blur: normals shorter than 1 somewhere, partial coverage
        assert ((got["coverage"] > 0) & (got["coverage"] < 1)).any()


@pytest.mark.parametrize("sw", [(1, 0, 0), (0, 1, 0), (0, 0, 1)])
def test_each_switch_alone_on_big1(rtlib, sw):
    S = 5
    got = ar.host_planes("big1", W, H, S, *map(bool, sw))
    want = ar.planes(gc.soa("big1"), W, H, S, *sw)
    assert not ar.same_planes(got, want)
    off = ar.host_planes("big1", W, H, S, False, False, False)
    assert ar.same_planes(got, off), "the switch changes something"  # big1 has an aperture and moving spheres
    centre = rtlib.guide_host(gc.soa("big1"), W, H)  # five equal rays: the centre pass's hits (5 n / 5 may round)
    assert np.array_equal(off["prim"], centre["prim"]) and np.array_equal(off["coverage"], (centre["prim"] >= 0).astype(F32))


@pytest.mark.parametrize("name", SCENES + ["rect_xy"])
def test_one_centre_sample_is_the_centre_pass(rtlib, name):
    soa = gc.soa(name)
    centre = rtlib.guide_host(soa, W, H)
    for footprint in (True, False):
        got = rtlib.guide_host(soa, W, H, samples=1, lens=False, footprint=footprint, shutter=False)
        for k in ("normal", "albedo", "depth", "prim"):
            assert got[k].tobytes() == centre[k].tobytes(), k
        assert np.array_equal(got["coverage"], (centre["prim"] >= 0).astype(F32))
    if name == "cornell":  # a rect seen from behind: -outward holds negative zeros, which 0 + n would lose
        n = centre["normal"]
        assert ((n == 0) & np.signbit(n)).any()


def _ball_in_the_sky() -> FlatScene:
    s = FlatScene()
    s.camera((0, 0, -6), (0, 0, 0), 30.0, aperture=0.3, focus=4.0)
    s.world = [s.obj_prim(s.sphere((0, 0, 0), 1.0, s.lambertian((0.8, 0.3, 0.3))))]
    return s


def test_coverage_is_hits_over_samples(rtlib):
    S = 16
    sc = _ball_in_the_sky()
    got = rtlib.guide_host(sc.soa, W, H, samples=S)
    want = ar.planes(sc.soa, W, H, S)
    assert not ar.same_planes(got, want)
    cov, hits = got["coverage"], want["hits"]
    assert np.array_equal(cov, hits.astype(F32) / F32(S))
    assert (cov[0] == 0).all() and (cov[:, 0] == 0).all()                  # empty sky: no hit, depth 0, prim -1
    assert ((cov == 0) == (got["prim"] < 0)).all() and ((cov == 0) == (got["depth"] == 0)).all()
    # the background summed 16 times and divided: 15 additions and a division, each within 2^-24 relative, of values <= 1
    assert (np.abs(got["albedo"][cov == 0] - np.array(list(sc.soa.background), F32)) <= 16 * 2.0 ** -24).all()
    assert (got["normal"][cov == 0] == 0).all()
    assert cov[H // 2, W // 2] == 1                                        # the ball's middle
    assert ((cov > 0) & (cov < 1)).any()                                   # its silhouette
    inside = rtlib.guide_host(gc.soa("cornell"), W, H, samples=S)["coverage"]
    assert (inside[2:-2, 2:-2] == 1).all()                                 # the box's interior


# ---------------------------------------------------------------- arguments
def test_aov_argument_table(rtlib):
    L = rtlib.lib()
    s = gc.scene("garden_3_bvh")
    soa = s.soa
    keep = np.full(256 * 5, 7.0, F32)
    ok = rtlib.aov_params(samples=4)
    assert L.rt_aov_pattern(ctypes.byref(ok), keep.ctypes.data) == 0 and not (keep[:20] == 7).any() and (keep[20:] == 7).all()
    keep[:] = 7
    bad = [dict(samples=0), dict(samples=-1), dict(samples=257), dict(lens=2), dict(lens=-1), dict(footprint=2),
           dict(footprint=-1), dict(shutter=2), dict(shutter=-1)]
    for kw in bad:
        p = rtlib.aov_params(dict(samples=4), **kw)
        assert L.rt_aov_pattern(ctypes.byref(p), keep.ctypes.data) == RT_ERR_ARG, kw
        assert L.rt_aov_render_host(ctypes.byref(soa), 3, 2, ctypes.byref(p), keep.ctypes.data, keep.ctypes.data, keep.ctypes.data,
                                    None, keep.ctypes.data) == RT_ERR_ARG, kw
        with pytest.raises(rtlib.RtError) as e:
            rtlib.guide_host(soa, 3, 2, **{"samples": 4, **kw})
        assert e.value.status == RT_ERR_ARG
    assert L.rt_aov_pattern(ctypes.byref(ok), None) == RT_ERR_ARG
    for w, h in [(0, 2), (3, 0), (-1, 2)]:
        assert L.rt_aov_render_host(ctypes.byref(soa), w, h, ctypes.byref(ok), None, None, keep.ctypes.data, None, None) == RT_ERR_ARG
    assert L.rt_aov_render_host(None, 3, 2, ctypes.byref(ok), None, None, keep.ctypes.data, None, None) == RT_ERR_ARG
    broken = s.soa
    broken.world[0] = 99
    assert L.rt_aov_render_host(ctypes.byref(broken), 3, 2, ctypes.byref(ok), None, None, keep.ctypes.data, None, None) == RT_ERR_SCENE
    assert (keep == 7).all()
    # null parameters are the defaults; every plane pointer may be null
    tab = np.zeros((16, 5), F32)
    assert L.rt_aov_pattern(None, tab.ctypes.data) == 0 and tab.tobytes() == ar.pattern(16).tobytes()
    cov = np.zeros((2, 3), F32)
    assert L.rt_aov_render_host(ctypes.byref(soa), 3, 2, None, None, None, None, None, cov.ctypes.data) == 0
    assert cov.tobytes() == rtlib.guide_host(soa, 3, 2, samples=16)["coverage"].tobytes()
    assert L.rt_aov_render_host(ctypes.byref(soa), 3, 2, None, None, None, None, None, None) == 0
    assert "coverage" not in rtlib.guide_host(soa, 3, 2)
