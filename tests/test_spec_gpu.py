"""Casts and feature planes that follow mirrors and glass on the GPU (rt_spec_* of include/rt_hip.h): rt_spec_cast's
hits and paths and rt_spec_render's five planes are the host twin's byte for byte, through host, device and null
pointers and in both row orders; max_bounces = 0 is rt_aov_render on the device; the guided denoise on specular
planes equals its host twin fed the host planes and changes no state; rt_main --guide-specular and the Python
drivers give the same bytes."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import aov_ref as ar
import denoise_ref as dr
import guide_cases as gc
import noise_ref as nr
import spec_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
F32 = np.float32
REF, PIX = 0, 1
RT_ERR_ARG, RT_ERR_STATE = 1, 3
NFB = 4
SIZES = [(33, 17), (70, 45)]  # neither a multiple of 16
COUNTS = (1, 63, 65, 397)     # below, beside and above a wave; more than one workgroup
GAINS = dict(normal_gain=2.0, albedo_gain=0.25, depth_gain=1024.0)


# ---------------------------------------------------------------- rt_spec_cast
@pytest.mark.parametrize("name", sc.DEVICE_SCENES)
def test_device_chains_are_the_hosts(rtlib, gpu_ctx, name):
    import torch

    soa = sc.soa(name)
    L = rtlib.lib()
    g = rtlib.Guide(soa)
    try:
        for mb in sc.BOUNCES:
            want_h, want_p = sc.host_trace(name, mb)
            for n in COUNTS:
                hits, paths = g.trace(sc.rays(name, n), max_bounces=mb, max_fuzz=0.25, glass=1)
                assert g.last_spec_ms() > 0.0
                assert gc.same_hits(hits, want_h[:n]), (mb, n, gc.diff_hits(hits, want_h[:n]))
                assert paths.tobytes() == want_p[:n].tobytes(), (mb, n, sc.diff_paths(paths, want_p[:n]))
        # device pointers, either output null, null parameters for the defaults
        n, p = 397, rtlib.spec_params(max_bounces=16, max_fuzz=0.25)
        want_h, want_p = sc.host_trace(name, 16)
        rays = torch.from_numpy(sc.rays(name, n).copy()).cuda()
        dh = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
        dp = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        assert L.rt_spec_cast(g._h, rays.data_ptr(), n, ctypes.byref(p), dh.data_ptr(), None) == 0
        assert L.rt_spec_cast(g._h, rays.data_ptr(), n, ctypes.byref(p), None, dp.data_ptr()) == 0
        assert dh.cpu().numpy().tobytes() == want_h[:n].tobytes() and dp.cpu().numpy().tobytes() == want_p[:n].tobytes()
        hp = np.zeros(n, rtlib.SPEC_PATH_DTYPE)
        assert L.rt_spec_cast(g._h, rays.data_ptr(), n, None, None, hp.ctypes.data) == 0  # a device input, a host output
        assert hp.tobytes() == rtlib.trace_host(soa, sc.rays(name, n))[1].tobytes()  # the defaults on both sides
        assert L.rt_spec_cast(g._h, rays.data_ptr(), n, None, None, None) == 0 and L.rt_spec_cast(g._h, None, 0, None, None, None) == 0
        # the plain cast is untouched by it
        assert gc.same_hits(g.cast(sc.rays(name, n)), sc.host_trace(name, 0)[0][:n])
        # refusals
        for kw in (dict(max_bounces=-1), dict(max_bounces=17), dict(max_fuzz=1.5), dict(max_fuzz=float("nan")), dict(glass=2)):
            bad = rtlib.spec_params(**kw)
            assert L.rt_spec_cast(g._h, rays.data_ptr(), n, ctypes.byref(bad), dh.data_ptr(), None) == RT_ERR_ARG, kw
        assert L.rt_spec_cast(g._h, None, n, None, dh.data_ptr(), None) == RT_ERR_ARG
        assert L.rt_spec_cast(g._h, rays.data_ptr(), -1, None, dh.data_ptr(), None) == RT_ERR_ARG
        assert L.rt_spec_cast(None, rays.data_ptr(), n, None, dh.data_ptr(), None) == RT_ERR_ARG and L.rt_spec_last_ms(None) == 0.0
        assert dh.cpu().numpy().tobytes() == want_h[:n].tobytes()
    finally:
        g.close()


# ---------------------------------------------------------------- rt_spec_render
def _planes(g):
    return dict(g.planes(png_order=False), coverage=g.coverage(png_order=False))


@pytest.mark.parametrize("name", ["mirror_hall", "glass", "moving_mirror", "big1"])
def test_device_planes_are_the_hosts(rtlib, gpu_ctx, name):
    import torch

    soa = sc.soa(name)
    L = rtlib.lib()
    g = rtlib.Guide(soa)
    try:
        for W, H in SIZES:
            for S in (None, 1, 5, 16):
                for mb in sc.BOUNCES:
                    want = sc.host_planes(name, W, H, S, mb)
                    g.render(W, H, samples=S, specular=dict(max_bounces=mb))
                    assert g.last_spec_ms() > 0.0
                    assert not ar.same_planes(_planes(g), want), (W, H, S, mb)
                    if S != 5 or mb != 4:
                        continue
                    top = dict(g.planes(png_order=True), coverage=g.coverage(png_order=True))
                    assert not ar.same_planes(top, {k: want[k][::-1] for k in ar.PLANES}), (W, H)
                    # device pointers, some of them null
                    alb = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
                    dep = torch.zeros(H * W, dtype=torch.float32, device="cuda")
                    cov = torch.zeros(H * W, dtype=torch.float32, device="cuda")
                    assert L.rt_guide_planes(g._h, None, alb.data_ptr(), dep.data_ptr(), None, 0) == 0
                    assert L.rt_aov_coverage(g._h, cov.data_ptr(), 0) == 0
                    assert alb.cpu().numpy().tobytes() == want["albedo"].tobytes() and dep.cpu().numpy().tobytes() == want["depth"].tobytes()
                    assert cov.cpu().numpy().tobytes() == want["coverage"].tobytes()
                    with np.errstate(all="ignore"):  # the 8-bit pictures of specular planes
                        want_n, want_a = dr.quant((want["normal"] + F32(1.0)) / F32(2.0)), dr.quant(want["albedo"])
                    assert np.array_equal(g.image("normal", png_order=False), want_n) and np.array_equal(g.image("albedo"), want_a[::-1])
        # null parameters: the centre ray and the defaults
        W, H = SIZES[0]
        assert L.rt_spec_render(g._h, W, H, None, None) == 0
        g.width, g.height = W, H
        assert not ar.same_planes(_planes(g), sc.host_planes(name, W, H, None, 4))
    finally:
        g.close()


@pytest.mark.parametrize("name", ["mirror_hall", "big1"])
def test_no_bounce_is_the_averaged_pass_on_the_device(rtlib, gpu_ctx, name):
    soa = sc.soa(name)
    L = rtlib.lib()
    g = rtlib.Guide(soa)
    try:
        for W, H in SIZES:
            for S in (1, 5, 16):
                avg = _planes(g.render(W, H, samples=S))
                assert not ar.same_planes(_planes(g.render(W, H, samples=S, specular=0)), avg), (W, H, S)
            centre = g.render(W, H).planes()
            got = g.render(W, H, specular=0).planes()
            assert all(got[k].tobytes() == centre[k].tobytes() for k in centre)
        # the three passes replace each other's planes; a refusal leaves them as they are
        W, H = SIZES[0]
        g.render(W, H, samples=5, specular=4)
        want = sc.host_planes(name, W, H, 5, 4)
        ok = rtlib.spec_params(4)
        for kw in (dict(max_bounces=17), dict(max_fuzz=-1.0), dict(glass=-1)):
            bad = rtlib.spec_params(**kw)
            assert L.rt_spec_render(g._h, W, H, None, ctypes.byref(bad)) == RT_ERR_ARG, kw
        bad_aov = rtlib.aov_params(samples=257)
        assert L.rt_spec_render(g._h, W, H, ctypes.byref(bad_aov), ctypes.byref(ok)) == RT_ERR_ARG
        for w, h in [(0, 4), (4, -1), (1 << 16, 1 << 16)]:
            assert L.rt_spec_render(g._h, w, h, None, ctypes.byref(ok)) == RT_ERR_ARG
        assert L.rt_spec_render(None, W, H, None, ctypes.byref(ok)) == RT_ERR_ARG
        assert not ar.same_planes(_planes(g), want)
        g.render(W, H)  # a centre pass drops the coverage, as after the averaged pass
        with pytest.raises(rtlib.RtError) as e:
            g.coverage()
        assert e.value.status == RT_ERR_STATE
    finally:
        g.close()


# ---------------------------------------------------------------- guided denoise on specular planes
def _twin(rtlib, fn, blob, prm, gains, planes, W, H):
    img = np.zeros((H, W, 3), np.uint8)
    gain = np.zeros((H, W), F32)
    p, g = rtlib.denoise_params(prm), rtlib.guide_params(gains)
    assert fn(blob, len(blob), ctypes.byref(p), ctypes.byref(g), planes["normal"].ctypes.data, planes["albedo"].ctypes.data,
              planes["depth"].ctypes.data, W, H, img.ctypes.data, gain.ctypes.data) == 0
    return img, gain


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: {int((got[0] != want[0]).sum())} image bytes differ"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), f"{what}: gain bits"


@pytest.mark.parametrize("W,H", SIZES)
def test_guided_denoise_on_specular_planes_equals_host_twins(rtlib, gpu_ctx, W, H):
    S, mb = 5, 4
    scene = sc.scene("big1")
    planes = sc.host_planes("big1", W, H, S, mb)
    gpu_ctx.upload(scene)
    n = W * H * 3
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, 1, 0, 1))
    ad = gpu_ctx.adaptive(rtlib.make_args(W, H, 2, 0, 1, cam_mode=PIX), chunk_fbs=3)
    g = rtlib.Guide(scene).render(W, H, samples=S, specular=mb)
    try:
        mon = acc.noise_monitor()
        acc.add_fbs(nr.random_fbs(NFB, n, 9500 + n, special=True).ctypes.data, NFB)
        ad.add(3)
        before = (acc.blob(), mon.blob(), ad.blob())
        first_hit = ar.host_planes("big1", W, H, S)
        for R, f in [(10, 3), (3, 0)]:
            prm = dict(search_radius=R, patch_radius=f, k=0.45, alpha=1.0, eps=1.0)
            want = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, before[1], prm, GAINS, planes, W, H)
            _same(mon.denoise(prm, png_order=False, gain=True, guide=g, guide_params=GAINS), want, f"monitor ({R}, {f})")
            other = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, before[1], prm, GAINS, first_hit, W, H)
            assert not np.array_equal(want[1], other[1])  # not the first-hit planes' weights
            want = _twin(rtlib, rtlib.lib().rt_guide_denoise_adaptive_blob, before[2], prm, GAINS, planes, W, H)
            _same(ad.denoise(prm, png_order=False, gain=True, guide=g, guide_params=GAINS), want, f"adaptive ({R}, {f})")
            _same(ad.denoise(prm, png_order=True, gain=True, guide=g, guide_params=GAINS), (want[0][::-1], want[1][::-1]), "png order")
        assert (acc.blob(), mon.blob(), ad.blob()) == before
        assert not ar.same_planes(_planes(g), planes)  # the guide is read only
    finally:
        g.close()
        ad.close()
        acc.close()


# ---------------------------------------------------------------- rt_main and the Python drivers
def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    W, H = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data[m.end():], np.uint8).reshape(H, W, 3)


def test_rt_main_guide_specular_and_the_drivers(rtlib, gpu_ctx, tmp_path):
    assert os.path.exists(RT_MAIN), "examples/bin/rt_main not built (python -m raytracing_gpu_amd._build)"
    out, den, aov = str(tmp_path / "out.ppm"), str(tmp_path / "den.ppm"), str(tmp_path / "aov")
    den1, aov1 = str(tmp_path / "den1.ppm"), str(tmp_path / "aov1")
    base = [RT_MAIN, "big1", "96", "2", "3", out, "--progressive", "2"]
    p = subprocess.run(base + ["--denoise", den, "--guided", "--aov", aov, "--guide-samples", "8", "--guide-specular", "3"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines[0]["aov"] == aov and lines[0]["guide_samples"] == 8 and lines[0]["guide_specular"] == 3 and lines[0]["guide_ms"] > 0
    p = subprocess.run(base + ["--denoise", den1, "--guided", "--aov", aov1, "--guide-specular", "16"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    first = json.loads(p.stdout.splitlines()[0])
    assert first["aov"] == aov1 and first["guide_specular"] == 16 and "guide_samples" not in first
    assert not os.path.exists(aov1 + "_coverage.ppm")
    for extra in (["--guide-specular", "3"], ["--aov", aov, "--guide-specular", "-1"], ["--aov", aov, "--guide-specular", "17"]):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "--guide-specular" in p.stderr  # alone, or out of range
    H = _read_ppm(out).shape[0]
    scene = rtlib.Scene.builtin("big1")
    gpu_ctx.upload(scene)
    acc = gpu_ctx.accumulator(rtlib.make_args(96, H, 2, 0, 1, 50, REF, seed=1984), 2)
    g = rtlib.Guide(scene)
    try:
        mon = acc.noise_monitor()
        acc.add(3)
        g.render(96, H, specular=16)  # from the centre ray
        want1 = mon.denoise(guide=g)
        assert np.array_equal(_read_ppm(aov1 + "_normal.ppm"), g.image("normal")) and np.array_equal(_read_ppm(aov1 + "_albedo.ppm"), g.image("albedo"))
        assert np.array_equal(_read_ppm(den1), want1)
        first_hit = g.render(96, H).image("albedo")
        assert not np.array_equal(first_hit, _read_ppm(aov1 + "_albedo.ppm"))  # the mirrors show something
        g.render(96, H, samples=8, specular=3)
        want = mon.denoise(guide=g)
        assert np.array_equal(_read_ppm(aov + "_normal.ppm"), g.image("normal")) and np.array_equal(_read_ppm(aov + "_albedo.ppm"), g.image("albedo"))
        grey = dr.quant(g.coverage())
        assert np.array_equal(_read_ppm(aov + "_coverage.ppm"), np.repeat(grey[..., None], 3, axis=2))
        assert np.array_equal(_read_ppm(den), want)
    finally:
        g.close()
        acc.close()
    s = rtlib.render_settings(image_width=96, image_height=H, samples_per_pixel_per_fb=2, no_fb=3)
    img, _ = rtlib.draw_progressive(scene, s, ctx=gpu_ctx, every=2, denoise=dict(guide=True, guide_samples=8, guide_specular=3))
    assert np.array_equal(img, want)
    img, _ = rtlib.draw_progressive(scene, s, ctx=gpu_ctx, every=2, denoise=dict(guide=True, guide_specular=16))
    assert np.array_equal(img, want1)
    prm = dict(search_radius=4, patch_radius=1)
    ck = str(tmp_path / "adaptive.ck")
    img, _, counts = rtlib.draw_adaptive(scene, s, ctx=gpu_ctx, every=1, until_noise=1.0, min_fbs=2, checkpoint=ck,
                                         denoise=dict(prm, guide=True, guide_params=GAINS, guide_samples=8, guide_specular=3))
    assert counts.min() >= 2
    planes = rtlib.guide_host(scene, 96, H, samples=8, specular=3)
    assert np.array_equal(img, rtlib.denoise_adaptive_checkpoint(ck, prm, guide=planes, guide_params=GAINS)[::-1])
    assert not np.array_equal(img, rtlib.denoise_adaptive_checkpoint(ck, prm, guide=rtlib.guide_host(scene, 96, H, samples=8),
                                                                     guide_params=GAINS)[::-1])
