"""Ray casts, feature planes and the guided denoise, host side (no GPU): the rt_guide_* ABI is declared, exported
and bound; rt_guide_cast_host gives the oracle's hit points, hit flags and texture values bit for bit on the
oracle's own captured camera rays; normals, centre rays and media behave as include/rt_hip.h says; the host twin
of the guided denoise equals the numpy definition of tests/guide_ref.py byte for byte.

One departure from "the cast hits iff a depth-1 record follows": the built-in cornell holds a diffuse_light, which
does not scatter, so a camera ray that hits it is followed by no depth-1 record (4 of the 340 hits at 24 x 16).
For a hit whose material is a diffuse_light the test asks for no following record instead, and that hit is pinned
by test_hit_flag_and_albedo_of_builtins (the depth-1 pixel is the emitted value, which is not the background)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import flat_cases as fc
import guide_cases as gc
import guide_ref as gr
import noise_ref as nr
from flat_scenes import FlatScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_gpu_amd", "csrc")
F32 = np.float32
RT_ERR_ARG, RT_ERR_STATE, RT_ERR_SCENE = 1, 3, 4
INT_NAMES = ["rt_guide_create", "rt_guide_destroy", "rt_guide_cast", "rt_guide_render", "rt_guide_planes", "rt_guide_image",
             "rt_guide_cast_host", "rt_guide_render_host", "rt_guide_denoise_monitor", "rt_guide_denoise_adaptive",
             "rt_guide_denoise_monitor_blob", "rt_guide_denoise_adaptive_blob"]
FP = 0x0FED_CBA9_8765_4321
NFB = 5
PRM = dict(k=0.45, alpha=1.0, eps=1.0)
GAINS = (4.0, 16.0, 64.0)
MAT_LIGHT = 3


# ---------------------------------------------------------------- ABI and sources
def test_guide_abi_declared_exported_bound(rtlib):
    hdr = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert set(re.findall(r"^\s*int\s+(rt_guide_\w+)\s*\(", hdr, re.M)) == set(INT_NAMES)
    assert re.findall(r"^\s*float\s+(rt_guide_\w+)\s*\(", hdr, re.M) == ["rt_guide_last_ms"]
    assert re.findall(r"^\s*void\s+(rt_guide_\w+)\s*\(", hdr, re.M) == ["rt_guide_params_default"]
    L = rtlib.lib()
    for n in INT_NAMES + ["rt_guide_last_ms", "rt_guide_params_default"]:
        assert hasattr(L, n) and n in rtlib.ABI, n
    assert ctypes.sizeof(rtlib.rt_guide_hit) == 64 and rtlib.GUIDE_HIT_DTYPE.itemsize == 64
    assert ctypes.sizeof(rtlib.rt_guide_params) == 16
    assert ctypes.sizeof(rtlib.rt_denoise_params) == 24  # the denoiser's own parameters are as they were
    d = rtlib.guide_params().as_dict()
    assert all(v >= 0 for v in d.values()) and set(d) == {"normal_gain", "albedo_gain", "depth_gain"}
    with pytest.raises(TypeError):
        rtlib.guide_params(gain=1.0)


def test_guide_sources_share_one_first_hit_and_are_built():
    """The twin is host only (no HIP header), both halves compile rt_first_hit.h and the denoiser's arithmetic."""
    from raytracing_gpu_amd import _build

    twin = open(os.path.join(CSRC, "rt_guide_host.cpp")).read()
    dev = open(os.path.join(CSRC, "rt_guide.hip")).read()
    core = open(os.path.join(CSRC, "rt_first_hit.h")).read()
    assert not re.search(r'#\s*include\s*[<"]hip', twin) and not re.search(r'#\s*include\s*[<"]hip', core)
    for src in (twin, dev):
        assert '#include "rt_first_hit.h"' in src and "rtfh::cast(" in src
    for f in ("rt_denoise.hip", "rt_denoise_blob.cpp"):
        assert "rtdn::feature_x(" in open(os.path.join(CSRC, f)).read()
    assert "rt_guide.hip" in _build.HIP_SOURCES and "rt_guide_host.cpp" in _build.HIP_SOURCES
    assert "rt_first_hit.h" in _build.HIP_DEPS and "-ffp-contract=off" in _build.HIPCC_FLAGS


def test_check_guide_host_program_builds_and_passes(tmp_path):
    """scripts/check_guide_host.cpp: the host twin on the smallest scene of every object kind and on images
    smaller than a tile, in a stand-alone program under the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "check_guide_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "scripts", "check_guide_host.cpp"), os.path.join(CSRC, "rt_guide_host.cpp"),
                    os.path.join(CSRC, "rt_validate.cpp"),
                    *[os.path.join(CSRC, f"rt_{x}_blob.cpp") for x in ("accum", "noise", "adapt", "denoise")], "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_guide_host ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- positions against the oracle
@pytest.mark.parametrize("name", list(gc.SCENES))
def test_hit_points_are_the_oracles(rtlib, oracle, name):
    """Every camera ray of a 24 x 16 render: the cast hits iff a depth-1 record follows it directly (a hit on a
    diffuse_light: iff none does, see the module docstring), and then p is that record's origin bit for bit."""
    rays, follows, origin = gc.camera_rays(name)
    assert len(rays) == gc.W * gc.H
    soa = gc.soa(name)
    h = rtlib.cast_host(soa, rays)
    hit = h["prim"] >= 0
    light = np.zeros(len(h), bool)
    light[hit] = [soa.materials[m].type == MAT_LIGHT for m in h["material"][hit]]
    assert name == "cornell" or not light.any()
    assert np.array_equal(hit & ~light, follows), np.flatnonzero((hit & ~light) != follows)[:8]
    assert 0 < follows.sum() and hit.sum() < len(h) or name in ("cornell", "chain")
    assert h["p"][follows].tobytes() == origin[follows].tobytes()
    # a miss is all zeros but the background
    miss = h[~hit]
    assert (miss["t"] == 0).all() and (miss["n"] == 0).all() and (miss["material"] == -1).all()
    assert (miss["albedo"] == np.array(list(soa.background), F32)).all()
    assert (h["t"][hit] >= F32(0.001)).all()


# ---------------------------------------------------------------- hit flag and albedo against the oracle
def _emissive_two_perlin() -> FlatScene:
    s = FlatScene()
    s.camera((13, 2, 3), (0, 0, 0), 20.0)
    m = s.light(s.noise(4.0, 11))
    s.world = [s.obj_prim(s.sphere((0, -1000, 0), 1000.0, m)), s.obj_prim(s.sphere((0, 2, 0), 2.0, s.light(s.marble(4.0, 12))))]
    return s


def _emissive_earth() -> FlatScene:
    from raytracing_gpu_amd.assets import synthetic_image

    s = FlatScene()
    s.camera((13, 2, 3), (0, 0, 0), 20.0)
    s.world = [s.obj_prim(s.sphere((0, 0, 0), 2.0, s.light(s.image(synthetic_image(64, 32, 3, seed=5)))))]
    return s


LIGHT_SCENES = {f"light_{t}": (lambda t=t: fc.shading(t, "light")) for t in
                ("solid", "checker_solid_noise", "checker_image_solid", "noise", "turbulence_7", "marble", "image_13x7x3",
                 "image_13x7x1", "image_none")}
LIGHT_SCENES["two_perlin_emissive"] = _emissive_two_perlin
LIGHT_SCENES["earth_emissive"] = _emissive_earth


def _flag_and_albedo(rtlib, oracle, soa):
    """On a depth-1 render a pixel is emitted(u, v, p) for a light, 0 for a scattering material and the background
    for a miss: the cast's flag and albedo against it, on the same captured rays."""
    rec, fb = gc.capture(oracle, soa, 1)
    assert len(rec) == gc.W * gc.H and (rec[:, 7] == 0).all()
    px = fb.reshape(-1, 3)
    h = rtlib.cast_host(soa, rec)
    hit = h["prim"] >= 0
    bg = np.array(list(soa.background), F32)
    is_bg = (px == bg).all(1)
    if bg.any():
        assert np.array_equal(~hit, is_bg)
    else:
        assert hit[~is_bg].all()
    light = np.zeros(len(h), bool)
    light[hit] = [soa.materials[m].type == MAT_LIGHT for m in h["material"][hit]]
    assert h["albedo"][light].tobytes() == px[light].tobytes()
    assert (px[hit & ~light] == 0).all()
    return h, light


@pytest.mark.parametrize("name", list(LIGHT_SCENES))
def test_hit_flag_and_albedo_on_lights(rtlib, oracle, name):
    s = LIGHT_SCENES[name]()
    h, light = _flag_and_albedo(rtlib, oracle, s.soa)
    assert light.sum() > 20
    if "solid" != name[6:] and "none" not in name:
        assert len(np.unique(h["albedo"][light], axis=0)) > 3  # a texture, not one colour


@pytest.mark.parametrize("name", ["big1", "cornell", "garden_5_list", "movers"])
def test_hit_flag_and_albedo_of_builtins(rtlib, oracle, name):
    h, light = _flag_and_albedo(rtlib, oracle, gc.soa(name))
    assert light.any() == (name == "cornell")


def test_albedo_of_scattering_materials(rtlib):
    """Lambertian and metal: the texture's value; dielectric: (1, 1, 1)."""
    s = gc.scene("garden_5_bvh")
    soa = s.soa
    rays = gc.camera_rays("garden_5_bvh")[0]
    h = rtlib.cast_host(soa, rays)
    seen = set()
    for k in np.flatnonzero(h["prim"] >= 0):
        m = soa.materials[h["material"][k]]
        t = soa.textures[m.texture] if m.type != 2 else None
        seen.add(m.type)
        if m.type == 2:
            assert (h["albedo"][k] == 1).all()
        elif t.type == 0:
            assert (h["albedo"][k] == np.array(list(t.color), F32)).all()
    assert {0, 1, 2} <= seen


# ---------------------------------------------------------------- normals
@pytest.mark.parametrize("name", ["garden_5_bvh", "garden_4_list", "big1"])
def test_sphere_normals(rtlib, name):
    """n = (p - c) / r against the ray, front = dot(d, outward) < 0, in float32 numpy in the reference's order."""
    soa = gc.soa(name)
    rays = gc.camera_rays(name)[0]
    h = rtlib.cast_host(soa, rays)
    ks = [k for k in np.flatnonzero(h["prim"] >= 0) if soa.prims[h["prim"][k]].type == 0]
    assert len(ks) > 100
    pr = np.array([list(soa.prims[h["prim"][k]].p)[:4] for k in ks], F32)
    p, d = h["p"][ks], rays[ks, 3:6]
    out = (F32(1.0) / pr[:, 3:4]) * (p - pr[:, :3])
    dt = d[:, 0] * out[:, 0] + d[:, 1] * out[:, 1] + d[:, 2] * out[:, 2]
    front = dt < 0
    n = np.where(front[:, None], out, -out)
    assert n.tobytes() == h["n"][ks].tobytes()
    assert np.array_equal(front, h["front"][ks] != 0)
    assert front.any()


# ---------------------------------------------------------------- centre rays
def _centre_rays(cam, Wd, Ht):
    v = lambda a: np.array(list(a), F32)
    i, j = np.meshgrid(np.arange(Wd), np.arange(Ht))
    s = ((i.astype(F32) + F32(0.5)) / F32(Wd))[..., None]
    t = ((j.astype(F32) + F32(0.5)) / F32(Ht))[..., None]
    d = v(cam.lower_left) + s * v(cam.horizontal) + t * v(cam.vertical) - v(cam.origin)
    rays = np.zeros((Ht, Wd, 8), F32)
    rays[..., :3], rays[..., 3:6] = v(cam.origin), d
    rays[..., 6] = F32(cam.time0) + F32(0.5) * (F32(cam.time1) - F32(cam.time0))
    return rays.reshape(-1, 8)


@pytest.mark.parametrize("Wd,Ht", [(7, 5), (33, 17)])
@pytest.mark.parametrize("name", ["movers", "big1", "world_medium_over_xform"])
def test_render_host_is_the_cast_of_centre_rays(rtlib, name, Wd, Ht):
    soa = gc.soa(name)
    pl = rtlib.guide_host(soa, Wd, Ht)
    h = rtlib.cast_host(soa, _centre_rays(soa.camera, Wd, Ht)).reshape(Ht, Wd)
    assert pl["normal"].tobytes() == h["n"].tobytes() and pl["albedo"].tobytes() == h["albedo"].tobytes()
    assert pl["depth"].tobytes() == h["t"].tobytes() and np.array_equal(pl["prim"], h["prim"])
    assert (pl["prim"] >= 0).any() and ((pl["depth"] == 0) == (pl["prim"] < 0)).all()


# ---------------------------------------------------------------- media
def test_medium_is_seen_as_its_boundary(rtlib):
    """cornell_smoke against a twin whose world names the media's boundary objects instead: the same hits, except
    that a smoke box carries the phase material and its texture."""
    sc = rtlib.Scene.builtin("cornell_smoke")
    so = sc.soa
    kinds = [so.objects[so.world[k]].kind for k in range(so.n_world)]
    assert kinds.count(rtlib.OBJ_MEDIUM) == 2
    tw = rtlib.rt_scene_soa()
    ctypes.memmove(ctypes.byref(tw), ctypes.byref(so), ctypes.sizeof(so))
    world = (ctypes.c_int32 * so.n_world)(*[so.objects[so.world[k]].a if kinds[k] == rtlib.OBJ_MEDIUM else so.world[k]
                                            for k in range(so.n_world)])
    tw.world = world
    assert rtlib.validate_scene(tw)[0] == 0
    rays = _centre_rays(so.camera, 24, 24)
    a, b = rtlib.cast_host(so, rays), rtlib.cast_host(tw, rays)
    for f in ("t", "p", "n", "u", "v", "prim", "front"):
        assert a[f].tobytes() == b[f].tobytes(), f
    smoke = a["material"] != b["material"]
    assert smoke.sum() > 20 and not smoke.all()
    phase = {so.objects[so.world[k]].b for k in range(so.n_world) if kinds[k] == rtlib.OBJ_MEDIUM}
    assert set(a["material"][smoke]) <= phase and all(so.materials[m].type == 4 for m in phase)
    for m in phase:
        col = np.array(list(so.textures[so.materials[m].texture].color), F32)
        assert (a["albedo"][a["material"] == m] == col).all()
    assert a[~smoke].tobytes() == b[~smoke].tobytes()


def test_cast_host_arguments(rtlib):
    s = gc.scene("garden_3_bvh")
    L = rtlib.lib()
    out = np.zeros(1, rtlib.GUIDE_HIT_DTYPE)
    ray = np.zeros((1, 8), F32)
    assert L.rt_guide_cast_host(None, ray.ctypes.data, 1, out.ctypes.data) == RT_ERR_ARG
    assert L.rt_guide_cast_host(ctypes.byref(s.soa), None, 1, out.ctypes.data) == RT_ERR_ARG
    assert L.rt_guide_cast_host(ctypes.byref(s.soa), ray.ctypes.data, -1, out.ctypes.data) == RT_ERR_ARG
    assert L.rt_guide_cast_host(ctypes.byref(s.soa), None, 0, None) == 0
    bad = s.soa
    bad.world[0] = 99
    assert L.rt_guide_cast_host(ctypes.byref(bad), ray.ctypes.data, 1, out.ctypes.data) == RT_ERR_SCENE
    assert L.rt_guide_render_host(ctypes.byref(s.soa), 0, 4, None, None, None, None) == RT_ERR_ARG
    # a ray with a zero direction, and one of NaNs, are answered as the reference's float tests answer them (a NaN
    # root passes sphere.h's range test), with indices in range, not a fault
    ray[0, :3] = (0, 1, -5)
    assert -1 <= rtlib.cast_host(s.soa, ray)["prim"][0] < s.soa.n_prims
    ray[:] = np.nan
    assert -1 <= rtlib.cast_host(s.soa, ray)["prim"][0] < s.soa.n_prims


# ---------------------------------------------------------------- guided filter
def _info(rtlib, W, H, k, **kw):
    a = rtlib.make_args(W, H, 3, 2, k, 50, rtlib.RT_CAM_PER_PIXEL, seed=77, **kw)
    return rtlib.rt_accum_info(a, W * H * 3, FP)


def _planes(W, H, seed, miss=True):
    """Feature planes with structure: unit normals of a few directions, albedo in blocks, depth a ramp; miss: a
    corner region of misses (depth 0, normal 0)."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    dirs = g.normal(size=(4, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F32)
    N = dirs[((x // 5) + (y // 4)) % 4].astype(F32)
    A = (g.uniform(0, 1, (3, 3))[(x // 7) % 3] + g.uniform(-0.02, 0.02, (H, W, 3))).astype(F32)
    Z = (3.0 + 0.05 * x + 0.3 * (y // 6) + g.uniform(0, 0.01, (H, W))).astype(F32)
    if miss:
        m = (x + y) < (W + H) // 4
        N[m], Z[m] = 0, 0
        A[m] = (0.7, 0.8, 1.0)
    return np.ascontiguousarray(N), np.ascontiguousarray(A), np.ascontiguousarray(Z)


def _twin(rtlib, fn, blob, prm, gains, planes, W, H, pw=None, ph=None, want_gain=True):
    img = np.full((H, W, 3), 0xAB, np.uint8)
    gain = np.full((H, W), -7.0, F32)
    p = rtlib.denoise_params(prm) if prm is not None else None
    g = rtlib.guide_params(dict(zip(("normal_gain", "albedo_gain", "depth_gain"), gains))) if gains is not None else None
    N, A, Z = planes
    rc = fn(bytes(blob), len(blob), ctypes.byref(p) if p is not None else None, ctypes.byref(g) if g is not None else None,
            N.ctypes.data if N is not None else None, A.ctypes.data if A is not None else None,
            Z.ctypes.data if Z is not None else None, W if pw is None else pw, H if ph is None else ph, img.ctypes.data,
            gain.ctypes.data if want_gain else None)
    return rc, img, gain


def _untouched(img, gain):
    return bool((img == 0xAB).all() and (gain == F32(-7.0)).all())


def _same(img, gain, want_img, want_gain):
    assert np.array_equal(img, want_img), f"image: {int((img != want_img).sum())} bytes differ"
    assert np.array_equal(gain.view(np.uint32), want_gain.view(np.uint32)), "gain bits"


@pytest.fixture(scope="module")
def moments(oracle):
    """{(W, H): (S1, S2)} of random frame buffers with zeros, NaN and infinities."""
    out = {}
    for W, H in [(5, 3), (33, 17), (70, 45)]:
        out[(W, H)] = nr.moments(nr.quantise(oracle, nr.random_fbs(NFB, W * H * 3, 20261020 + W, special=True), W, H))
    return out


@pytest.mark.parametrize("R,f", [(0, 0), (2, 1), (10, 3)])
@pytest.mark.parametrize("W,H", [(5, 3), (33, 17), (70, 45)])
def test_guided_twin_equals_the_definition(rtlib, moments, W, H, R, f):
    S1, S2 = moments[(W, H)]
    blob = nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2)
    planes = _planes(W, H, W)
    prm = dict(PRM, search_radius=R, patch_radius=f)
    rc, img, gain = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, blob, prm, GAINS, planes, W, H)
    assert rc == 0
    want = gr.denoise(S1, S2, NFB, H, W, R, f, prm["k"], prm["alpha"], prm["eps"], *planes, GAINS)
    _same(img, gain, *want)
    plain = dr.denoise(S1, S2, NFB, H, W, R, f, prm["k"], prm["alpha"], prm["eps"])
    assert (gain <= plain[1]).all()  # the feature term only lowers a weight
    if R and W > 5:
        assert (gain < plain[1]).any()
    rc, img2, g2 = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, blob, prm, GAINS, planes, W, H, want_gain=False)
    assert rc == 0 and np.array_equal(img2, img) and (g2 == F32(-7.0)).all()


def test_zero_gains_are_the_unguided_filter(rtlib, moments):
    """With every gain 0 and no pixel a miss (or every pixel one) the bytes are rt_denoise_monitor_blob's."""
    W, H = 33, 17
    S1, S2 = moments[(W, H)]
    blob = nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2)
    prm = dict(PRM, search_radius=4, patch_radius=2)
    img0 = np.zeros((H, W, 3), np.uint8)
    gain0 = np.zeros((H, W), F32)
    p = rtlib.denoise_params(prm)
    assert rtlib.lib().rt_denoise_monitor_blob(blob, len(blob), ctypes.byref(p), img0.ctypes.data, gain0.ctypes.data) == 0
    N, A, Z = _planes(W, H, 3, miss=False)
    for planes in ((N, A, Z), (N, A, np.zeros_like(Z))):
        rc, img, gain = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, blob, prm, (0, 0, 0), planes, W, H)
        assert rc == 0
        _same(img, gain, img0, gain0)
    rc, img, gain = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, blob, prm, GAINS, (N, A, Z), W, H)
    assert rc == 0 and not np.array_equal(gain, gain0)


def test_no_weight_crosses_a_hit_miss_boundary(rtlib):
    """A constant image (every colour weight 1) with misses left of a column: the gain counts the window's pixels
    on the pixel's own side."""
    W, H, n, R = 30, 12, 3, 5
    c = np.full(H * W * 3, 180, np.uint64)
    S1, S2 = np.uint64(n) * c * c, np.uint64(n) * c ** np.uint64(4)
    blob = nr.pack(rtlib, _info(rtlib, W, H, n), S1, S2)
    N = np.zeros((H, W, 3), F32)
    N[..., 2] = 1
    A = np.full((H, W, 3), 0.5, F32)
    Z = np.full((H, W), 2.0, F32)
    Z[:, :W // 2], N[:, :W // 2] = 0, 0
    cy = np.array([min(H - 1, y + R) - max(0, y - R) + 1 for y in range(H)])
    side = np.array([(min(W // 2 - 1, x + R) - max(0, x - R) + 1) if x < W // 2 else
                     (min(W - 1, x + R) - max(W // 2, x - R) + 1) for x in range(W)])
    for f in (0, 3):
        rc, img, gain = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, blob, dict(PRM, search_radius=R, patch_radius=f),
                              (0, 0, 0), (N, A, Z), W, H)
        assert rc == 0 and (img == 180).all()
        assert np.array_equal(gain, (cy[:, None] * side[None, :]).astype(F32))


def test_nan_plane_value_counts_as_64(rtlib):
    """A NaN in a plane: that pixel weighs 0 in every other pixel's window and keeps its own centre weight."""
    W, H, n, R = 15, 9, 3, 10
    c = np.full(H * W * 3, 90, np.uint64)
    S1, S2 = np.uint64(n) * c * c, np.uint64(n) * c ** np.uint64(4)
    blob = nr.pack(rtlib, _info(rtlib, W, H, n), S1, S2)
    for which in range(3):
        N, A, Z = np.zeros((H, W, 3), F32), np.full((H, W, 3), 0.5, F32), np.full((H, W), 2.0, F32)
        (N, A, Z)[which][4, 7] = np.nan
        rc, img, gain = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, blob, dict(PRM, search_radius=R, patch_radius=1),
                              (1, 1, 1), (N, A, Z), W, H)
        assert rc == 0
        want = dr.window_pixels(H, W, R) - F32(1)  # (4, 7) lies in every pixel's window
        want[4, 7] = 1
        assert np.array_equal(gain, want)
        _same(img, gain, *gr.denoise(S1, S2, n, H, W, R, 1, PRM["k"], PRM["alpha"], PRM["eps"], N, A, Z, (1, 1, 1)))


def _mixed_counts(oracle, W, H, counts):
    """(n_t [tiles], n per pixel [H][W], S1, S2): tile t has folded in the first counts[t] of 9 frame buffers."""
    c = nr.quantise(oracle, nr.random_fbs(9, W * H * 3, 424243, special=True), W, H).reshape(9, H, W, 3)
    ty, tx = (H + 15) // 16, (W + 15) // 16
    n_t = np.array(counts, np.int64).reshape(ty, tx)
    n_px = np.repeat(np.repeat(n_t, 16, 0), 16, 1)[:H, :W]
    c2 = c * c
    live = (np.arange(9)[:, None, None] < n_px[None])[..., None]
    return n_t.reshape(-1), n_px, (c2 * live).sum(0, dtype=np.uint64).reshape(-1), (c2 * c2 * live).sum(0, dtype=np.uint64).reshape(-1)


def _adaptive_blob(rtlib, W, H, n_t, S1, S2):
    L = rtlib.lib()
    info = _info(rtlib, W, H, int(np.max(n_t)))
    n_t = np.ascontiguousarray(n_t, np.int32)
    active = np.zeros(n_t.size, np.uint8)
    sums = np.zeros(W * H * 3, np.float32)
    s1, s2 = np.ascontiguousarray(S1, np.uint32), np.ascontiguousarray(S2, np.uint64)
    need = ctypes.c_size_t()
    assert L.rt_adaptive_blob_pack(ctypes.byref(info), None, None, None, None, None, None, 0, ctypes.byref(need)) == 0
    buf = ctypes.create_string_buffer(need.value)
    assert L.rt_adaptive_blob_pack(ctypes.byref(info), n_t.ctypes.data, active.ctypes.data, sums.ctypes.data, s1.ctypes.data,
                                   s2.ctypes.data, buf, need.value, None) == 0
    return buf.raw


def test_guided_adaptive_twin_equals_the_definition(rtlib, oracle):
    W, H = 40, 37
    n_t, n_px, S1, S2 = _mixed_counts(oracle, W, H, [2, 5, 9, 9, 2, 5, 5, 9, 2])
    blob = _adaptive_blob(rtlib, W, H, n_t, S1, S2)
    planes = _planes(W, H, 9)
    for R, f in [(10, 3), (3, 0)]:
        prm = dict(PRM, search_radius=R, patch_radius=f)
        rc, img, gain = _twin(rtlib, rtlib.lib().rt_guide_denoise_adaptive_blob, blob, prm, GAINS, planes, W, H)
        assert rc == 0
        _same(img, gain, *gr.denoise(S1, S2, n_px, H, W, R, f, prm["k"], prm["alpha"], prm["eps"], *planes, GAINS))


def test_guided_argument_table(rtlib, moments):
    W, H = 33, 17
    S1, S2 = moments[(W, H)]
    L = rtlib.lib()
    fn = L.rt_guide_denoise_monitor_blob
    good = nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2)
    small = dict(PRM, search_radius=2, patch_radius=1)
    planes = _planes(W, H, 1)
    assert _twin(rtlib, fn, good, small, GAINS, planes, W, H)[0] == 0
    # plane size, null planes, gains
    for pw, ph in [(W - 1, H), (W, H + 1), (H, W), (0, 0)]:
        rc, img, gain = _twin(rtlib, fn, good, small, GAINS, planes, W, H, pw, ph)
        assert rc == RT_ERR_ARG and _untouched(img, gain), (pw, ph)
    for k in range(3):
        pl = list(planes)
        pl[k] = None
        rc, img, gain = _twin(rtlib, fn, good, small, GAINS, pl, W, H)
        assert rc == RT_ERR_ARG and _untouched(img, gain)
    for bad in [(-1.0, 0, 0), (0, -0.5, 0), (0, 0, -1e-9), (float("nan"), 0, 0), (0, 0, float("nan"))]:
        rc, img, gain = _twin(rtlib, fn, good, small, bad, planes, W, H)
        assert rc == RT_ERR_ARG and _untouched(img, gain), bad
    # the unguided call's errors: parameters, n < 2, a band tiling, a malformed blob
    rc, img, gain = _twin(rtlib, fn, good, dict(small, k=0.0), GAINS, planes, W, H)
    assert rc == RT_ERR_ARG and _untouched(img, gain)
    for n in (0, 1):
        blob = nr.pack(rtlib, _info(rtlib, W, H, n), S1 * np.uint64(0), S2 * np.uint64(0))
        rc, img, gain = _twin(rtlib, fn, blob, small, GAINS, planes, W, H)
        assert rc == RT_ERR_STATE and _untouched(img, gain)
    a = rtlib.make_args(W, H, 3, 2, NFB, 50, rtlib.RT_CAM_PER_PIXEL, seed=77, band_rows=4, band_first=0, band_stride=2)
    nv = len(rtlib.owned_rows(a)) * W * 3
    band = nr.pack(rtlib, rtlib.rt_accum_info(a, nv, FP), S1[:nv], S2[:nv])
    rc, img, gain = _twin(rtlib, fn, band, small, GAINS, planes, W, H)
    assert rc == RT_ERR_ARG and _untouched(img, gain)
    rc, img, gain = _twin(rtlib, fn, good[:-1], small, GAINS, planes, W, H)
    assert rc == RT_ERR_ARG and _untouched(img, gain)
    assert _twin(rtlib, L.rt_guide_denoise_adaptive_blob, good, small, GAINS, planes, W, H)[0] == RT_ERR_ARG
    # null parameters and gains are the defaults
    rc, img, gain = _twin(rtlib, fn, good, None, None, planes, W, H)
    assert rc == 0
    d, g = rtlib.denoise_params().as_dict(), rtlib.guide_params().as_dict()
    _same(img, gain, *gr.denoise(S1, S2, NFB, H, W, d["search_radius"], d["patch_radius"], d["k"], d["alpha"], d["eps"], *planes,
                                 (g["normal_gain"], g["albedo_gain"], g["depth_gain"])))


def test_guided_checkpoint_files(rtlib, moments, tmp_path):
    W, H = 33, 17
    S1, S2 = moments[(W, H)]
    path = tmp_path / "m.noise"
    path.write_bytes(nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2))
    prm = dict(PRM, search_radius=3, patch_radius=1)
    N, A, Z = _planes(W, H, 2)
    guide = {"normal": N, "albedo": A, "depth": Z}
    gains = dict(normal_gain=1.0, albedo_gain=2.0, depth_gain=3.0)
    img, gain = rtlib.denoise_checkpoint(str(path), prm, gain=True, guide=guide, guide_params=gains)
    _same(img, gain, *gr.denoise(S1, S2, NFB, H, W, 3, 1, prm["k"], prm["alpha"], prm["eps"], N, A, Z, (1.0, 2.0, 3.0)))
    # without the keywords: the unguided call, as before
    assert np.array_equal(rtlib.denoise_checkpoint(str(path), prm), dr.denoise(S1, S2, NFB, H, W, 3, 1, prm["k"], prm["alpha"], prm["eps"])[0])
    with pytest.raises(rtlib.RtError) as e:
        rtlib.denoise_checkpoint(str(path), prm, guide=guide, guide_params=dict(depth_gain=-1.0))
    assert e.value.status == RT_ERR_ARG
    with pytest.raises(ValueError):
        rtlib.denoise_checkpoint(str(path), prm, guide={"normal": N, "albedo": A, "depth": Z[:, :-1]})
