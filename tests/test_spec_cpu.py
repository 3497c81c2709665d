"""Casts and feature planes that follow mirrors and glass, host side (no GPU): the rt_spec_* ABI is declared,
exported and bound as a closed set; rt_spec_cast_host equals the numpy restatement of tests/spec_ref.py in every
field as bytes; max_bounces = 0 is the plain cast and the plain planes; the chain's segments are the CPU oracle's
own path wherever the reference's random choice is the deterministic one; every status is reached; the planes are
the chains summed as the averaged pass sums."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import aov_ref as ar
import guide_cases as gc
import spec_cases as sc
import spec_ref as sr
from flat_scenes import FlatScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_gpu_amd", "csrc")
F32 = np.float32
RT_ERR_ARG, RT_ERR_SCENE = 1, 4
W, H = sc.W, sc.H
INT_NAMES = ["rt_spec_cast", "rt_spec_render", "rt_spec_cast_host", "rt_spec_render_host"]
MISS, SURFACE, ESCAPED, LIMIT, ABSORBED = range(5)


# ---------------------------------------------------------------- ABI and sources
def test_spec_abi_declared_exported_bound(rtlib):
    hdr = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert set(re.findall(r"^\s*int\s+(rt_spec_\w+)\s*\(", hdr, re.M)) == set(INT_NAMES)
    assert re.findall(r"^\s*float\s+(rt_spec_\w+)\s*\(", hdr, re.M) == ["rt_spec_last_ms"]
    assert re.findall(r"^\s*void\s+(rt_spec_\w+)\s*\(", hdr, re.M) == ["rt_spec_params_default"]
    L = rtlib.lib()
    names = INT_NAMES + ["rt_spec_last_ms", "rt_spec_params_default"]
    for n in names:
        assert hasattr(L, n) and n in rtlib.ABI, n
    assert sorted(n for n in rtlib.ABI if n.startswith("rt_spec_")) == sorted(names)
    assert ctypes.sizeof(rtlib.rt_spec_params) == 16 and ctypes.sizeof(rtlib.rt_spec_path) == 32
    assert rtlib.SPEC_PATH_DTYPE.itemsize == 32 and rtlib.GUIDE_HIT_DTYPE.itemsize == 64
    d = rtlib.spec_params().as_dict()
    assert d["max_bounces"] == 4 and d["glass"] == 1 and d["max_fuzz"] == float(np.float32(0.1))
    assert rtlib.spec_params(7).max_bounces == 7 and rtlib.spec_params(True).max_bounces == 4
    assert rtlib.spec_params(dict(max_bounces=2), glass=False).as_dict() == {"max_bounces": 2, "max_fuzz": d["max_fuzz"], "glass": 0}
    with pytest.raises(TypeError):
        rtlib.spec_params(roughness=1)
    assert [getattr(rtlib, "SPEC_" + k) for k in ("MISS", "SURFACE", "ESCAPED", "LIMIT", "ABSORBED")] == [0, 1, 2, 3, 4]
    for k, v in sc.STATUS.items():
        assert re.search(rf"RT_SPEC_{k} = {v}\b", hdr), k
    # the closed families and pinned sizes beside it are as they were
    assert ctypes.sizeof(rtlib.rt_guide_params) == 16 and ctypes.sizeof(rtlib.rt_aov_params) == 16
    assert ctypes.sizeof(rtlib.rt_guide_hit) == 64


def test_spec_sources_share_one_definition():
    """The twin is host only, both halves compile csrc/rt_spec.h, which has no HIP include and one call site of the
    world query per loop."""
    from raytracing_gpu_amd import _build

    twin = open(os.path.join(CSRC, "rt_guide_host.cpp")).read()
    dev = open(os.path.join(CSRC, "rt_guide.hip")).read()
    core = open(os.path.join(CSRC, "rt_spec.h")).read()
    assert not re.search(r'#\s*include\s*[<"]hip', twin) and not re.search(r'#\s*include\s*[<"]hip', core)
    for src in (twin, dev):
        assert '#include "rt_spec.h"' in src and "rtspec::pixel(" in src and "rtspec::trace(" in src
    assert "spec_cast_kernel" in dev and "spec_render_kernel" in dev
    assert "rt_spec.h" in _build.HIP_DEPS
    for fn in ("trace", "pixel"):  # a do-while over segments around the one cast
        body = core.split(f"RT_HD void {fn}(", 1)[1].split("\n}\n", 1)[0]
        assert body.count("rtfh::cast(") == 1 and re.search(r"do rtfh::cast\(sc, e, &h\);\s*while \(advance\(", body), fn


def test_check_spec_host_program_builds_and_passes(tmp_path):
    """scripts/check_spec_host.cpp: the twin on images smaller than a tile, every status, max_bounces 0 and 16 and
    every refusal, in a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "check_spec_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "scripts", "check_spec_host.cpp"), os.path.join(CSRC, "rt_guide_host.cpp"),
                    os.path.join(CSRC, "rt_validate.cpp"),
                    *[os.path.join(CSRC, f"rt_{x}_blob.cpp") for x in ("accum", "noise", "adapt", "denoise")], "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_spec_host ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- the chain
@pytest.mark.parametrize("mb", sc.BOUNCES)
@pytest.mark.parametrize("name", list(sc.SCENES))
def test_host_twin_equals_the_numpy_restatement(rtlib, name, mb):
    hits, paths = sc.host_trace(name, mb)
    want_h, want_p, _ = sr.chain(sc.soa(name), sc.rays(name), mb, 0.25, 1)
    assert gc.same_hits(hits, want_h), gc.diff_hits(hits, want_h)
    assert paths.tobytes() == want_p.tobytes(), sc.diff_paths(paths, want_p)
    assert (paths["bounces"] <= mb).all() and ((paths["status"] == LIMIT) <= (paths["bounces"] == mb)).all()
    assert ((paths["status"] == MISS) == (paths["first_prim"] < 0)).all() and (paths["depth"][paths["status"] == MISS] == 0).all()


def test_every_status_and_every_chain_length(rtlib):
    """The scenes reach what they were written for."""
    _, p = sc.host_trace("mirror_hall", 16)
    assert set(np.unique(p["bounces"])) == set(range(17)) and set(np.unique(p["status"])) == {MISS, SURFACE, ESCAPED, LIMIT}
    rows = p["bounces"][:W * H].reshape(H, W)  # chains of 1 to 12 bounces and more inside one 16 x 4 block of pixels
    assert max(len(np.unique(rows[j:j + 4, :16])) for j in range(H - 3)) >= 12
    thr = p["throughput"][p["bounces"] == 2]
    assert np.allclose(thr, F32(0.9) * np.array([0.8, 0.85, 0.9], F32), rtol=1e-6)  # one bounce on each mirror
    _, p = sc.host_trace("short_normal", 4)
    assert (p["status"] == ABSORBED).sum() > 20 and (p["bounces"][p["status"] == ABSORBED] == 0).all()
    assert (p["throughput"][p["status"] == ABSORBED] == 1).all()  # absorbed before the tint is taken
    # glass: front faces, back faces, total internal reflection in the box
    h, p = sc.host_trace("glass", 16)
    assert p["bounces"].max() >= 5 and (p["throughput"] == 1).all()
    _, _, segs = sr.chain(sc.soa("glass"), sc.rays("glass"), 16, 0.25, 1)
    fronts = set()
    for idx, e in segs[:-1]:
        hh = rtlib.cast_host(sc.soa("glass"), e)
        fronts |= set(np.unique(hh["front"][hh["material"] == 0]).tolist())
    assert fronts == {0, 1}
    # without glass the dielectrics end the chain; (1, 1, 1) stays their albedo
    h0, p0 = sc.host_trace("glass", 16, 0.25, 0)
    assert (p0["bounces"] == 0).all() and gc.same_hits(h0, rtlib.cast_host(sc.soa("glass"), sc.rays("glass")))
    # the fuzz threshold is <=
    h, p = sc.host_trace("fuzz_threshold", 4)
    assert set(np.unique(p["first_material"][p["bounces"] > 0])) == {0, 1}
    assert {2, 3} <= set(np.unique(p["first_material"][(p["bounces"] == 0) & (p["status"] == SURFACE)]))
    h, p = sc.host_trace("fuzz_threshold", 4, 0.0)
    assert set(np.unique(p["first_material"][p["bounces"] > 0])) == {0}
    # the medium ends the chain, seen directly and in the mirror
    h, p = sc.host_trace("medium_mirror", 4)
    fog = h["material"] == 0
    assert (p["status"][fog] == SURFACE).all() and {0, 1} <= set(np.unique(p["bounces"][fog]))
    assert (h["albedo"][fog] == np.array([0.6, 0.7, 0.9], F32)).all()


def test_time_is_carried_along_the_chain(rtlib):
    soa = sc.soa("moving_mirror")
    r = sc.rays("moving_mirror")
    _, _, segs = sr.chain(soa, r, 4, 0.25, 1)
    assert len(segs) >= 2
    for idx, e in segs:
        assert (e[:, 6] == r[idx, 6]).all()
    assert len(np.unique(r[:, 6])) == 3
    # the same rays at another time see the mirror elsewhere
    r2 = r.copy()
    r2[:, 6] = F32(1.0) - r2[:, 6]
    assert rtlib.trace_host(soa, r2, max_bounces=4)[1].tobytes() != sc.host_trace("moving_mirror", 4)[1].tobytes()


@pytest.mark.parametrize("name", list(sc.SCENES))
def test_no_bounce_is_the_plain_cast_and_the_plain_planes(rtlib, name):
    soa = sc.soa(name)
    hits, paths = sc.host_trace(name, 0)
    plain = rtlib.cast_host(soa, sc.rays(name))
    assert gc.same_hits(hits, plain), gc.diff_hits(hits, plain)
    assert (paths["bounces"] == 0).all() and paths["depth"].tobytes() == plain["t"].tobytes()
    assert np.array_equal(paths["first_prim"], plain["prim"]) and np.array_equal(paths["first_material"], plain["material"])
    assert (paths["throughput"] == 1).all() and set(np.unique(paths["status"])) <= {MISS, SURFACE, LIMIT}
    centre, got = rtlib.guide_host(soa, W, H), sc.host_planes(name, W, H, None, 0)
    for k in ("normal", "albedo", "depth", "prim"):
        assert got[k].tobytes() == centre[k].tobytes(), k
    assert np.array_equal(got["coverage"], (centre["prim"] >= 0).astype(F32))
    for S in (1, 5):
        avg = rtlib.guide_host(soa, W, H, samples=S)
        assert not ar.same_planes(sc.host_planes(name, W, H, S, 0), avg), S


# ---------------------------------------------------------------- the planes
def _planes_from_chains(rtlib, soa, W, H, S, sw, **spec):
    """The definition's planes: the averaged pass's rays traced by the host twin and summed in sample order."""
    tab = ar.pattern(S, *sw) if S else ar.pattern(1, 0, 0, 0)
    lens = sw[0] if S else 0
    bg = np.array(list(soa.background), F32)
    sn = sa = None
    st, hits, first = np.zeros(H * W, F32), np.zeros(H * W, np.int32), np.full(H * W, -1, np.int32)
    for s in range(len(tab)):
        h, p = rtlib.trace_host(soa, ar.rays(soa.camera, W, H, tab[s], lens), **spec)
        sky = (p["status"] == MISS) | (p["status"] == ESCAPED)
        al = p["throughput"] * np.where(sky[:, None], bg, h["albedo"])
        sn = h["n"].copy() if s == 0 else sn + h["n"]
        sa = al if s == 0 else sa + al
        hit = p["first_prim"] >= 0
        st = np.where(hit, np.where(hits > 0, st + p["depth"], p["depth"]), st)
        first = np.where(hit & (hits == 0), p["first_prim"], first)
        hits = hits + hit
    fs = F32(len(tab))
    with np.errstate(all="ignore"):
        depth = np.where(hits > 0, st / hits.astype(F32), F32(0.0)).astype(F32)
    out = {"normal": (sn / fs).reshape(H, W, 3), "albedo": (sa / fs).reshape(H, W, 3), "depth": depth.reshape(H, W),
           "prim": first.reshape(H, W), "coverage": (hits.astype(F32) / fs).reshape(H, W)}
    assert all(out[k].dtype == F32 for k in ("normal", "albedo", "depth", "coverage"))
    return out


@pytest.mark.parametrize("S", [None, 1, 5])
@pytest.mark.parametrize("name", ["mirror_hall", "glass", "moving_mirror", "big1"])
def test_planes_are_the_chains_summed_in_sample_order(rtlib, name, S):
    soa = sc.soa(name)
    for mb in (1, 16):
        got = sc.host_planes(name, W, H, S, mb)
        want = _planes_from_chains(rtlib, soa, W, H, S, (1, 1, 1), max_bounces=mb)
        assert not ar.same_planes(got, want), (mb, ar.same_planes(got, want))
    # the silhouette is the first surface's; what a mirror shows is not the mirror
    plain = rtlib.guide_host(soa, W, H) if S is None else rtlib.guide_host(soa, W, H, samples=S)
    assert np.array_equal(got["prim"], plain["prim"]) and np.array_equal(got["coverage"] > 0, plain["prim"] >= 0)
    assert got["albedo"].tobytes() != plain["albedo"].tobytes() and (got["depth"] >= plain["depth"]).all()
    if S is not None:
        assert np.array_equal(got["coverage"], plain["coverage"])


def test_absorbed_is_not_reached_by_the_written_scenes_with_mirrors_swapped_in(rtlib):
    """The written scenes of tests/guide_cases.py with every material turned into a fuzz-0 metal: the
    set_face_normal quirks of the instances leave no normal along the ray, so no chain is absorbed there.  (The
    branch stays -- it is the reference's return value -- and tests/spec_cases.py's short_normal reaches it.)"""
    total = 0
    for name, build in gc.SCENES.items():
        s = build()
        if not isinstance(s, FlatScene):
            continue
        white = s.solid((0.9, 0.9, 0.9))
        for i, m in enumerate(s.mats):
            s.mats[i] = rtlib.rt_material(rtlib.MAT_METAL, m.texture if m.texture >= 0 else white, 0.0, 0)
        soa = s.soa
        _, p = rtlib.trace_host(soa, ar.rays(soa.camera, W, H, ar.pattern(1, 0, 0, 0)[0], 0), max_bounces=16, max_fuzz=0.0)
        assert (p["status"] != ABSORBED).all(), name
        total += int((p["bounces"] > 0).sum())
    assert total > 1000  # the chains did bounce


# ---------------------------------------------------------------- the oracle's own path
def _records_by_pixel(rec):
    """The oracle's records split at every camera ray (bounce depth 0)."""
    cam = np.flatnonzero(rec[:, 7] == 0)
    assert len(cam) == W * H
    return [rec[a:b] for a, b in zip(cam, list(cam[1:]) + [len(rec)])]


def _pin(rtlib, oracle, name, B, random_lobe):
    """Compares every pixel's chain with the oracle's path of the same camera ray.  Returns (pixels whose primary
    hit is specular, those of them whose comparison stopped at the first bounce because the oracle took another
    lobe, segments compared)."""
    soa = sc.soa(name)
    rec, _ = gc.capture(oracle, soa, B + 2)
    per = _records_by_pixel(rec)
    cam = np.stack([r[0] for r in per])
    assert all((r[:, 7] == np.arange(len(r))).all() for r in per)
    hits_k = [rtlib.trace_host(soa, cam, max_bounces=k) for k in range(B + 1)]
    _, paths, segs = sr.chain(soa, cam, B, 0.25, 1)
    assert paths.tobytes() == hits_k[B][1].tobytes()
    direction = {}  # (pixel, k) -> the chain's segment-k ray
    for k, (idx, e) in enumerate(segs):
        for i, row in zip(idx, e):
            direction[(int(i), k)] = row
    specular = stopped = compared = 0
    for px, r in enumerate(per):
        b, status = int(paths["bounces"][px]), int(paths["status"][px])
        specular += b > 0 or status == LIMIT
        for k in range(b + 1):
            hk, pk = hits_k[k][0][px], hits_k[k][1][px]
            if status == MISS or (k == b and status == ESCAPED):
                assert len(r) == k + 1, (px, k, "the oracle's path leaves the scene where the chain does")
                break
            assert len(r) > k + 1, (px, k, "the oracle scatters where the chain stands on a surface")
            assert (r[k + 1, :3] == hk["p"]).all(), (px, k, r[k + 1, :3], hk["p"])  # numeric: -0 == +0
            assert r[k + 1, 6] == cam[px, 6]
            if k == b:
                break  # the last surface: what leaves it is the oracle's random lobe
            assert int(pk["status"]) == LIMIT and int(pk["bounces"]) == k
            if not (r[k + 1, 3:6] == direction[(px, k + 1)][3:6]).all():
                assert random_lobe, (px, k, "a direction differs where nothing is random")
                stopped += k == 0
                break
            compared += 1
    return specular, stopped, compared


def test_mirror_hall_chains_are_the_oracles_paths(rtlib, oracle):
    """24 x 16, B = 16: every pixel through all its bounces (fuzz-0 metal has no random lobe)."""
    specular, stopped, compared = _pin(rtlib, oracle, "mirror_hall", 16, False)
    assert specular > 150 and stopped == 0 and compared > 400


def test_glass_chains_are_the_oracles_paths_until_its_lobe_differs(rtlib, oracle):
    """24 x 16 on the glass ball seen from the front and on the glass scene: compared until the oracle reflects
    where the chain refracts (Schlick's random choice).  At most a quarter of the glass-hitting pixels may stop at the
    first bounce.  Measured when this was written: 15 of 167 (9.0 %) on glass_ball and 7 of 105 (6.7 %) on glass.
    The reference alone, counted from the oracle's records without the chain (a depth-1 direction that is the
    mirrored camera ray), reflects 15 of 167 and 16 of 105 (15.2 %): on glass that count includes the nine pixels
    of total internal reflection on the hollow sphere's inside-out face, where the chain reflects too."""
    for name in ("glass_ball", "glass"):
        specular, stopped, compared = _pin(rtlib, oracle, name, 8, True)
        # the reference alone: the oracle's depth-1 ray leaves a dielectric as the mirror image of the camera ray
        soa = sc.soa(name)
        rec, _ = gc.capture(oracle, soa, 2)
        per = _records_by_pixel(rec)
        cam = np.stack([r[0] for r in per])
        h = rtlib.cast_host(soa, cam)
        glass_px = np.flatnonzero((h["prim"] >= 0) & (np.array([soa.materials[max(m, 0)].type for m in h["material"]]) == rtlib.MAT_DIELECTRIC))
        d = cam[glass_px, 3:6]
        ud = sr._scaled(F32(1.0) / np.sqrt(sr.dot(d, d)), d)
        refl = sr.reflect(ud, h["n"][glass_px])
        alone = sum(bool((per[p][1, 3:6] == refl[i]).all()) for i, p in enumerate(glass_px))
        print(f"{name}: {stopped} of {specular} glass-hitting pixels stop at the first bounce; the reference alone reflects "
              f"{alone} of {len(glass_px)}; {compared} segments compared")
        assert specular == len(glass_px) and specular > 100
        assert alone <= 0.25 * len(glass_px)
        assert stopped <= 0.25 * specular and compared > 100


# ---------------------------------------------------------------- arguments
def test_spec_argument_table(rtlib):
    L = rtlib.lib()
    s = gc.scene("garden_3_bvh")
    soa = s.soa
    r = np.ascontiguousarray(sc.rays("mirror_hall", 5))
    hits, paths = np.zeros(5, rtlib.GUIDE_HIT_DTYPE), np.zeros(5, rtlib.SPEC_PATH_DTYPE)
    keep = np.full(3 * 2 * 3, 7.0, F32)
    ok, aov = rtlib.spec_params(2), rtlib.aov_params(samples=2)
    bad = [dict(max_bounces=-1), dict(max_bounces=17), dict(max_fuzz=-0.5), dict(max_fuzz=1.5), dict(max_fuzz=float("nan")),
           dict(glass=2), dict(glass=-1)]
    params = [rtlib.spec_params(**kw) for kw in bad]
    params.append(rtlib.spec_params())
    params[-1].reserved = 1
    for p in params:
        assert L.rt_spec_cast_host(ctypes.byref(soa), r.ctypes.data, 5, ctypes.byref(p), hits.ctypes.data, paths.ctypes.data) == RT_ERR_ARG
        assert L.rt_spec_render_host(ctypes.byref(soa), 3, 2, None, ctypes.byref(p), keep.ctypes.data, keep.ctypes.data, keep.ctypes.data,
                                     None, keep.ctypes.data) == RT_ERR_ARG
    for kw in bad:
        with pytest.raises(rtlib.RtError) as e:
            rtlib.trace_host(soa, r, **kw)
        assert e.value.status == RT_ERR_ARG
        with pytest.raises(rtlib.RtError) as e:
            rtlib.guide_host(soa, 3, 2, specular=kw)
        assert e.value.status == RT_ERR_ARG
    bad_aov = rtlib.aov_params(samples=4, lens=2)
    assert L.rt_spec_render_host(ctypes.byref(soa), 3, 2, ctypes.byref(bad_aov), ctypes.byref(ok), None, None, keep.ctypes.data, None,
                                 None) == RT_ERR_ARG
    for w, h in [(0, 2), (3, 0), (-1, 2)]:
        assert L.rt_spec_render_host(ctypes.byref(soa), w, h, ctypes.byref(aov), ctypes.byref(ok), None, None, keep.ctypes.data, None,
                                     None) == RT_ERR_ARG
    assert L.rt_spec_render_host(None, 3, 2, None, ctypes.byref(ok), None, None, keep.ctypes.data, None, None) == RT_ERR_ARG
    assert L.rt_spec_cast_host(None, r.ctypes.data, 5, ctypes.byref(ok), hits.ctypes.data, None) == RT_ERR_ARG
    assert L.rt_spec_cast_host(ctypes.byref(soa), None, 5, ctypes.byref(ok), hits.ctypes.data, None) == RT_ERR_ARG
    assert L.rt_spec_cast_host(ctypes.byref(soa), r.ctypes.data, -1, ctypes.byref(ok), hits.ctypes.data, None) == RT_ERR_ARG
    broken = s.soa
    broken.world[0] = 99
    assert L.rt_spec_cast_host(ctypes.byref(broken), r.ctypes.data, 5, ctypes.byref(ok), hits.ctypes.data, None) == RT_ERR_SCENE
    assert L.rt_spec_render_host(ctypes.byref(broken), 3, 2, None, ctypes.byref(ok), None, None, keep.ctypes.data, None, None) == RT_ERR_SCENE
    assert (keep == 7).all() and not hits.tobytes().strip(b"\0") and not paths.tobytes().strip(b"\0")
    # n = 0, null outputs, null parameters for the defaults, null aov parameters for the centre ray
    assert L.rt_spec_cast_host(ctypes.byref(soa), None, 0, None, None, None) == 0
    assert L.rt_spec_cast_host(ctypes.byref(soa), r.ctypes.data, 5, None, None, None) == 0
    assert L.rt_spec_cast_host(ctypes.byref(soa), r.ctypes.data, 5, None, hits.ctypes.data, None) == 0
    assert L.rt_spec_cast_host(ctypes.byref(soa), r.ctypes.data, 5, None, None, paths.ctypes.data) == 0
    want_h, want_p = rtlib.trace_host(soa, r)
    assert hits.tobytes() == want_h.tobytes() and paths.tobytes() == want_p.tobytes()
    dep = np.zeros((2, 3), F32)
    assert L.rt_spec_render_host(ctypes.byref(soa), 3, 2, None, None, None, None, dep.ctypes.data, None, None) == 0
    assert dep.tobytes() == rtlib.guide_host(soa, 3, 2, specular=True)["depth"].tobytes()
    one = rtlib.aov_params(samples=1, lens=0, footprint=0, shutter=0)
    dep2 = np.zeros((2, 3), F32)
    assert L.rt_spec_render_host(ctypes.byref(soa), 3, 2, ctypes.byref(one), None, None, None, dep2.ctypes.data, None, None) == 0
    assert dep.tobytes() == dep2.tobytes()
    assert L.rt_spec_render_host(ctypes.byref(soa), 3, 2, None, None, None, None, None, None, None) == 0
    # without the keyword nothing changes
    assert "coverage" not in rtlib.guide_host(soa, 3, 2) and "coverage" not in rtlib.guide_host(soa, 3, 2, specular=False)
    assert "coverage" in rtlib.guide_host(soa, 3, 2, specular=0)
