"""Ray casts, feature planes and the guided denoise on the GPU (rt_guide_* of include/rt_hip.h): rt_guide_cast
equals rt_guide_cast_host in every field bit for bit, on the oracle's captured camera rays and on grazing and
axis-aligned ones, through host and device pointers; rt_guide_render's planes are the host's; the guided filter
equals its host twin byte for byte on a monitor and on an adaptive accumulator with mixed counts, changes no
state, refuses a guide of another scene, and leaves the unguided filter's bytes as they were; rt_main --aov and
--guided and the Python drivers give the same bytes."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import guide_cases as gc
import noise_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
F32 = np.float32
REF, PIX = 0, 1
RT_ERR_ARG, RT_ERR_STATE = 1, 3
NFB = 4
GAINS = dict(normal_gain=4.0, albedo_gain=16.0, depth_gain=64.0)


# ---------------------------------------------------------------- rt_guide_cast
@pytest.mark.parametrize("name", list(gc.SCENES) + list(gc.MORE))
def test_cast_equals_the_host_twin(rtlib, gpu_ctx, oracle, name):
    """Counts 1, 63, 65 (one wave, with and without a second) and everything; host and device pointers."""
    import torch

    soa = gc.soa(name)
    rays = np.ascontiguousarray(np.concatenate([gc.camera_rays(name)[0], gc.extra_rays(name)]))
    want = rtlib.cast_host(soa, rays)
    assert (want["prim"] >= 0).any()
    g = rtlib.Guide(soa)
    try:
        for n in (1, 63, 65, len(rays)):
            got = g.cast(rays[:n])
            assert gc.same_hits(got, want[:n]), f"{n} rays, host pointers: {gc.diff_hits(got, want[:n])}"
        assert g.last_ms() > 0.0
        for n in (65, len(rays)):
            r_d = torch.from_numpy(rays[:n].copy()).cuda()
            out_d = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
            g.cast_into(r_d.data_ptr(), n, out_d.data_ptr())
            got = out_d.cpu().numpy().view(rtlib.GUIDE_HIT_DTYPE)
            assert gc.same_hits(got, want[:n]), f"{n} rays, device pointers: {gc.diff_hits(got, want[:n])}"
        assert len(g.cast(rays[:0])) == 0
    finally:
        g.close()


def test_guide_arguments(rtlib, gpu_ctx):
    s = gc.scene("garden_3_bvh")
    L = rtlib.lib()
    h = ctypes.c_void_p()
    assert L.rt_guide_create(None, 0, ctypes.byref(h)) == RT_ERR_ARG
    bad = s.soa
    bad.world[0] = 99
    assert L.rt_guide_create(ctypes.byref(bad), 0, ctypes.byref(h)) == 4 and not h.value  # RT_ERR_SCENE
    g = rtlib.Guide(s)
    try:
        for call in (g.planes, lambda: g.image("normal")):
            g.width, g.height = 4, 4
            with pytest.raises(rtlib.RtError) as e:
                call()
            assert e.value.status == RT_ERR_STATE  # nothing rendered yet
        for w, hgt in [(0, 4), (4, -1)]:
            with pytest.raises(rtlib.RtError) as e:
                g.render(w, hgt)
            assert e.value.status == RT_ERR_ARG
        out = np.zeros(1, rtlib.GUIDE_HIT_DTYPE)
        assert L.rt_guide_cast(g._h, None, 1, out.ctypes.data) == RT_ERR_ARG
        assert L.rt_guide_cast(g._h, out.ctypes.data, -1, out.ctypes.data) == RT_ERR_ARG
    finally:
        g.close()


# ---------------------------------------------------------------- rt_guide_render
@pytest.mark.parametrize("name", ["big1", "world_medium_over_xform", "random_2", "cornell"])
def test_render_planes_are_the_hosts(rtlib, gpu_ctx, name):
    """70 x 45: no multiple of 16, 32 or 64."""
    import torch

    W, H = 70, 45
    soa = gc.soa(name)
    want = rtlib.guide_host(soa, W, H)
    g = rtlib.Guide(soa)
    try:
        g.render(W, H)
        assert g.last_ms() > 0.0
        got = g.planes(png_order=False)
        for k in ("normal", "albedo", "depth", "prim"):
            assert got[k].tobytes() == want[k].tobytes(), k
        top = g.planes(png_order=True)
        for k in ("normal", "albedo", "depth", "prim"):
            assert top[k].tobytes() == want[k][::-1].tobytes(), k
        # device pointers, some of them null
        nrm = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
        prim = torch.zeros(H * W, dtype=torch.int32, device="cuda")
        L = rtlib.lib()
        assert L.rt_guide_planes(g._h, nrm.data_ptr(), None, None, prim.data_ptr(), 0) == 0
        assert nrm.cpu().numpy().tobytes() == want["normal"].tobytes() and prim.cpu().numpy().tobytes() == want["prim"].tobytes()
        assert L.rt_guide_planes(g._h, nrm.data_ptr(), None, None, None, 1) == RT_ERR_ARG
        # the pictures: quant((n + 1) / 2) and quant(albedo)
        with np.errstate(all="ignore"):
            want_n = dr.quant((want["normal"] + F32(1.0)) / F32(2.0))
            want_a = dr.quant(want["albedo"])
        assert np.array_equal(g.image("normal", png_order=False), want_n)
        assert np.array_equal(g.image("normal"), want_n[::-1]) and np.array_equal(g.image("albedo"), want_a[::-1])
        img_d = torch.zeros(H * W * 3, dtype=torch.uint8, device="cuda")
        assert L.rt_guide_image(g._h, 1, img_d.data_ptr(), 0) == 0
        assert np.array_equal(img_d.cpu().numpy().reshape(H, W, 3), want_a)
        # a second render at another size replaces the planes
        g.render(33, 17)
        small = rtlib.guide_host(soa, 33, 17)
        assert g.planes()["depth"].tobytes() == small["depth"].tobytes()
    finally:
        g.close()


# ---------------------------------------------------------------- guided denoise
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


@pytest.mark.parametrize("W,H", [(70, 45), (33, 17)])
def test_guided_monitor_equals_host_twin_and_changes_no_state(rtlib, gpu_ctx, W, H):
    import torch

    n = W * H * 3
    scene = rtlib.Scene.builtin("big1")
    gpu_ctx.upload(scene)
    fbs = nr.random_fbs(NFB, n, 9300 + n, special=True)
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, 1, 0, 1))
    g = rtlib.Guide(scene)
    other = rtlib.Guide(rtlib.Scene.builtin("cornell"))
    try:
        mon = acc.noise_monitor()
        acc.add_fbs(fbs.ctypes.data, NFB)
        before = (acc.blob(), mon.blob())
        prm0 = dict(search_radius=4, patch_radius=1, k=0.45, alpha=1.0, eps=1.0)
        unguided = mon.denoise(prm0, png_order=False, gain=True)  # before any guide was used
        # nothing rendered, another size, another scene: RT_ERR_STATE with the outputs untouched
        img = np.full((H, W, 3), 0xAB, np.uint8)
        gain = np.full((H, W), -7.0, F32)
        p, gp = rtlib.denoise_params(prm0), rtlib.guide_params(GAINS)
        call = lambda guide: rtlib.lib().rt_guide_denoise_monitor(mon._h, guide._h, ctypes.byref(p), ctypes.byref(gp),
                                                                  img.ctypes.data, gain.ctypes.data, 0)
        assert call(g) == RT_ERR_STATE
        g.render(W + 1, H)
        assert call(g) == RT_ERR_STATE
        other.render(W, H)
        assert call(other) == RT_ERR_STATE
        assert (img == 0xAB).all() and (gain == F32(-7.0)).all()
        g.render(W, H)
        planes = g.planes()
        assert (planes["depth"] == 0).any() and (planes["depth"] > 0).any()  # sky and spheres: hit / miss boundaries
        gp.depth_gain = -1.0
        assert call(g) == RT_ERR_ARG and (img == 0xAB).all()
        for R, f in [(10, 3), (10, 0), (3, 3)]:
            prm = dict(prm0, search_radius=R, patch_radius=f)
            want = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, before[1], prm, GAINS, planes, W, H)
            _same(mon.denoise(prm, png_order=False, gain=True, guide=g, guide_params=GAINS), want, f"({R}, {f}) rows ascending")
            assert mon.last_denoise_ms() > 0.0
            _same(mon.denoise(prm, png_order=True, gain=True, guide=g, guide_params=GAINS), (want[0][::-1], want[1][::-1]),
                  f"({R}, {f}) png order")
        assert want[1].max() > 1.0  # something was averaged
        # device pointers
        prm = dict(prm0, search_radius=3, patch_radius=3)
        img_d = torch.zeros(n, dtype=torch.uint8, device="cuda")
        gain_d = torch.zeros(W * H, dtype=torch.float32, device="cuda")
        p, gp = rtlib.denoise_params(prm), rtlib.guide_params(GAINS)
        assert rtlib.lib().rt_guide_denoise_monitor(mon._h, g._h, ctypes.byref(p), ctypes.byref(gp), img_d.data_ptr(),
                                                    gain_d.data_ptr(), 0) == 0
        torch.cuda.synchronize()
        _same((img_d.cpu().numpy().reshape(H, W, 3), gain_d.cpu().numpy().reshape(H, W)), want, "device pointers")
        # no state changed, the guide's planes neither, and the unguided filter gives the bytes it gave before
        assert (acc.blob(), mon.blob()) == before
        again = g.planes()
        assert all(again[k].tobytes() == planes[k].tobytes() for k in planes)
        _same(mon.denoise(prm0, png_order=False, gain=True), unguided, "unguided after guided")
        want0 = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), F32)
        p0 = rtlib.denoise_params(prm0)
        assert rtlib.lib().rt_denoise_monitor_blob(before[1], len(before[1]), ctypes.byref(p0), want0[0].ctypes.data,
                                                   want0[1].ctypes.data) == 0
        _same(unguided, want0, "unguided against its twin")
    finally:
        other.close()
        g.close()
        acc.close()


def test_guided_adaptive_equals_host_twin_and_changes_no_state(rtlib, gpu_ctx):
    W, H = 70, 45
    scene = rtlib.Scene.builtin("cornell_smoke")
    gpu_ctx.upload(scene)
    ad = gpu_ctx.adaptive(rtlib.make_args(W, H, 2, 0, 1, cam_mode=PIX), chunk_fbs=3)
    g = rtlib.Guide(scene).render(W, H)
    try:
        ad.add(2)
        nmap = ad.noise_map()
        thr = float(np.median(nmap[nmap > 0]))
        above = nr.tiles(nmap, thr)[1]
        max_above = int(np.median(above))
        assert above.min() <= max_above < above.max()
        ad.retire(thr, max_above)
        ad.add(3)
        counts = ad.counts()
        assert set(np.unique(counts)) == {2, 5}
        before = ad.blob()
        planes = g.planes()
        for R, f in [(10, 3), (5, 0)]:
            prm = dict(search_radius=R, patch_radius=f)
            want = _twin(rtlib, rtlib.lib().rt_guide_denoise_adaptive_blob, before, prm, GAINS, planes, W, H)
            _same(ad.denoise(prm, png_order=False, gain=True, guide=g, guide_params=GAINS), want, f"adaptive ({R}, {f})")
            _same(ad.denoise(prm, png_order=True, gain=True, guide=g, guide_params=GAINS), (want[0][::-1], want[1][::-1]), "png order")
        assert ad.last_denoise_ms() > 0.0
        assert ad.blob() == before and np.array_equal(ad.counts(), counts)
        other = rtlib.Guide(rtlib.Scene.builtin("cornell")).render(W, H)
        try:
            with pytest.raises(rtlib.RtError) as e:
                ad.denoise(guide=other)
            assert e.value.status == RT_ERR_STATE
        finally:
            other.close()
    finally:
        g.close()
        ad.close()


def _mse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float((d * d).mean())


@pytest.mark.parametrize("scene", ["big1", "cornell_smoke", "cornell"])
def test_guided_image_is_closer_to_the_truth(rtlib, gpu_ctx, scene):
    """tests/test_denoise_gpu.py's protocol -- 192 x 128, 4 samples per frame buffer, the candidates after 16 frame
    buffers against the plain image after 2048, mean squared error in 8-bit levels -- with the shipped gains: the
    guided image is closer than the plain one everywhere, and no farther than the unguided filter's (big1 is the
    narrow one: 23.016 against 23.016, its depth of field blurs what the centre rays' features keep sharp)."""
    W, H = 192, 128
    sc = rtlib.Scene.builtin(scene)
    gpu_ctx.upload(sc)
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, 4, 0, 1), 128)
    g = rtlib.Guide(sc).render(W, H)
    try:
        mon = acc.noise_monitor()
        acc.add(16)
        plain, unguided, guided = acc.image(png_order=True), mon.denoise(), mon.denoise(guide=g)
        acc.add(2048 - 16)
        truth = acc.image(png_order=True)
    finally:
        g.close()
        acc.close()
    m = [_mse(x, truth) for x in (plain, unguided, guided)]
    print(f"{scene}: mse plain {m[0]:.4f}, unguided {m[1]:.4f}, guided {m[2]:.4f}")
    assert m[2] < m[0] and m[2] <= m[1]


# ---------------------------------------------------------------- rt_main and the Python drivers
def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    W, H = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data[m.end():], np.uint8).reshape(H, W, 3)


def test_rt_main_aov_and_guided_and_the_drivers(rtlib, gpu_ctx, tmp_path):
    assert os.path.exists(RT_MAIN), "examples/bin/rt_main not built (python -m raytracing_gpu_amd._build)"
    out, out2, aov = str(tmp_path / "out.ppm"), str(tmp_path / "den.ppm"), str(tmp_path / "aov")
    p = subprocess.run([RT_MAIN, "big1", "96", "2", "3", out, "--progressive", "2", "--denoise", out2, "--guided", "--aov", aov],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines[0]["aov"] == aov and lines[0]["guide_ms"] > 0 and lines[-1]["denoised"] == out2
    den_main, H = _read_ppm(out2), _read_ppm(out).shape[0]
    p = subprocess.run([RT_MAIN, "big1", "96", "2", "3", out, "--guided"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--guided" in p.stderr  # refused without --denoise
    scene = rtlib.Scene.builtin("big1")
    gpu_ctx.upload(scene)
    acc = gpu_ctx.accumulator(rtlib.make_args(96, H, 2, 0, 1, 50, REF, seed=1984), 2)
    g = rtlib.Guide(scene).render(96, H)
    try:
        mon = acc.noise_monitor()
        acc.add(3)
        want, plain_den = mon.denoise(guide=g), mon.denoise()
        assert np.array_equal(_read_ppm(aov + "_normal.ppm"), g.image("normal"))
        assert np.array_equal(_read_ppm(aov + "_albedo.ppm"), g.image("albedo"))
    finally:
        g.close()
        acc.close()
    assert np.array_equal(den_main, want) and not np.array_equal(want, plain_den)
    s = rtlib.render_settings(image_width=96, image_height=H, samples_per_pixel_per_fb=2, no_fb=3)
    img, _ = rtlib.draw_progressive(scene, s, ctx=gpu_ctx, every=2, denoise=dict(guide=True))
    assert np.array_equal(img, want)
    img, _ = rtlib.draw_progressive(scene, s, ctx=gpu_ctx, every=2, denoise=True)  # without the keyword: as before
    assert np.array_equal(img, plain_den)
    prm = dict(search_radius=4, patch_radius=1)
    ck = str(tmp_path / "adaptive.ck")
    img, _, counts = rtlib.draw_adaptive(scene, s, ctx=gpu_ctx, every=1, until_noise=1.0, min_fbs=2, checkpoint=ck,
                                         denoise=dict(prm, guide=True, guide_params=GAINS))
    assert counts.min() >= 2
    planes = rtlib.guide_host(scene, 96, H)
    assert np.array_equal(img, rtlib.denoise_adaptive_checkpoint(ck, prm, guide=planes, guide_params=GAINS)[::-1])
    assert not np.array_equal(img, rtlib.denoise_adaptive_checkpoint(ck, prm)[::-1])
