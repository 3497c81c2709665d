"""Feature planes averaged over lens, footprint and shutter samples on the GPU (rt_aov_* of include/rt_hip.h):
rt_aov_render's five planes are rt_aov_render_host's byte for byte, through host, device and null pointers and in
both row orders; the averaged and the centre pass replace each other's planes; the guided denoise on averaged
planes equals its host twin fed the host planes and changes no state; the guided image stays closer to the truth
than the plain one; rt_main --guide-samples and the Python drivers give the same bytes."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
F32 = np.float32
REF, PIX = 0, 1
RT_ERR_ARG, RT_ERR_STATE = 1, 3
NFB = 4
SIZES = [(33, 17), (70, 45)]  # neither a multiple of 16
GAINS = dict(normal_gain=2.0, albedo_gain=0.25, depth_gain=1024.0)


# ---------------------------------------------------------------- rt_aov_render
@pytest.mark.parametrize("name", ["big1", "cornell", "world_medium_over_xform", "random_2"])
def test_averaged_planes_are_the_hosts(rtlib, gpu_ctx, name):
    import torch

    soa = gc.soa(name)
    L = rtlib.lib()
    g = rtlib.Guide(soa)
    try:
        for W, H in SIZES:
            for S in (1, 2, 5, 16, 64):
                want = ar.host_planes(name, W, H, S)
                g.render(W, H, samples=S)
                assert g.last_aov_ms() > 0.0
                got = dict(g.planes(png_order=False), coverage=g.coverage(png_order=False))
                assert not ar.same_planes(got, want), (W, H, S)
                if S != 5:
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
                assert L.rt_aov_coverage(g._h, cov.data_ptr(), 1) == RT_ERR_ARG and L.rt_aov_coverage(g._h, None, 0) == 0
                assert L.rt_aov_coverage(g._h, cov.data_ptr(), 2) == RT_ERR_ARG
        # a single switch, and null parameters for the defaults
        W, H = SIZES[0]
        for sw in [(True, False, False), (False, True, False), (False, False, True)]:
            g.render(W, H, 5, *sw)
            got = dict(g.planes(png_order=False), coverage=g.coverage(png_order=False))
            assert not ar.same_planes(got, ar.host_planes(name, W, H, 5, *sw)), sw
        assert L.rt_aov_render(g._h, W, H, None) == 0
        got = dict(g.planes(png_order=False), coverage=g.coverage(png_order=False))
        assert not ar.same_planes(got, ar.host_planes(name, W, H, 16))
    finally:
        g.close()


def test_averaged_and_centre_pass_replace_each_other(rtlib, gpu_ctx):
    soa = gc.soa("big1")
    L = rtlib.lib()
    g = rtlib.Guide(soa)
    try:
        with pytest.raises(rtlib.RtError) as e:
            g.width, g.height = 4, 4
            g.coverage()
        assert e.value.status == RT_ERR_STATE  # nothing rendered yet
        (W, H), (W2, H2) = SIZES
        centre, avg = rtlib.guide_host(soa, W, H), ar.host_planes("big1", W2, H2, 5)
        g.render(W, H)
        with pytest.raises(rtlib.RtError) as e:
            g.coverage()
        assert e.value.status == RT_ERR_STATE  # a centre pass keeps no coverage
        g.render(W2, H2, samples=5)  # after a centre pass, at another size
        assert not ar.same_planes(dict(g.planes(), coverage=g.coverage(png_order=False)), avg)
        # the 8-bit pictures of averaged planes
        with np.errstate(all="ignore"):
            want_n, want_a = dr.quant((avg["normal"] + F32(1.0)) / F32(2.0)), dr.quant(avg["albedo"])
        assert np.array_equal(g.image("normal", png_order=False), want_n) and np.array_equal(g.image("albedo"), want_a[::-1])
        g.render(W, H)  # and the reverse: the centre pass's planes, the coverage dropped
        got = g.planes()
        assert all(got[k].tobytes() == centre[k].tobytes() for k in centre)
        with pytest.raises(rtlib.RtError) as e:
            g.coverage()
        assert e.value.status == RT_ERR_STATE
        # refusals leave the planes as they are
        for kw in (dict(samples=0), dict(samples=257), dict(samples=4, lens=2), dict(samples=4, footprint=-1), dict(samples=4, shutter=2)):
            p = rtlib.aov_params(**kw)
            assert L.rt_aov_render(g._h, W, H, ctypes.byref(p)) == RT_ERR_ARG, kw
        ok = rtlib.aov_params(samples=2)
        for w, h in [(0, 4), (4, -1), (1 << 16, 1 << 16)]:
            assert L.rt_aov_render(g._h, w, h, ctypes.byref(ok)) == RT_ERR_ARG
        assert L.rt_aov_render(None, W, H, ctypes.byref(ok)) == RT_ERR_ARG and L.rt_aov_last_ms(None) == 0.0
        got = g.planes()
        assert all(got[k].tobytes() == centre[k].tobytes() for k in centre)
    finally:
        g.close()


# ---------------------------------------------------------------- guided denoise on averaged planes
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
def test_guided_denoise_on_averaged_planes_equals_host_twins(rtlib, gpu_ctx, W, H):
    S = 16
    scene = rtlib.Scene.builtin("big1")
    planes = ar.host_planes("big1", W, H, S)
    assert ((planes["coverage"] > 0) & (planes["coverage"] < 1)).any()
    gpu_ctx.upload(scene)
    n = W * H * 3
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, 1, 0, 1))
    ad = gpu_ctx.adaptive(rtlib.make_args(W, H, 2, 0, 1, cam_mode=PIX), chunk_fbs=3)
    g = rtlib.Guide(scene).render(W, H, samples=S)
    try:
        mon = acc.noise_monitor()
        acc.add_fbs(nr.random_fbs(NFB, n, 9400 + n, special=True).ctypes.data, NFB)
        ad.add(3)
        before = (acc.blob(), mon.blob(), ad.blob())
        centre = rtlib.guide_host(scene, W, H)
        for R, f in [(10, 3), (3, 0)]:
            prm = dict(search_radius=R, patch_radius=f, k=0.45, alpha=1.0, eps=1.0)
            want = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, before[1], prm, GAINS, planes, W, H)
            _same(mon.denoise(prm, png_order=False, gain=True, guide=g, guide_params=GAINS), want, f"monitor ({R}, {f})")
            other = _twin(rtlib, rtlib.lib().rt_guide_denoise_monitor_blob, before[1], prm, GAINS, centre, W, H)
            assert not np.array_equal(want[1], other[1])  # not the centre planes' weights
            want = _twin(rtlib, rtlib.lib().rt_guide_denoise_adaptive_blob, before[2], prm, GAINS, planes, W, H)
            _same(ad.denoise(prm, png_order=False, gain=True, guide=g, guide_params=GAINS), want, f"adaptive ({R}, {f})")
            _same(ad.denoise(prm, png_order=True, gain=True, guide=g, guide_params=GAINS), (want[0][::-1], want[1][::-1]), "png order")
        assert (acc.blob(), mon.blob(), ad.blob()) == before
        got = dict(g.planes(), coverage=g.coverage(png_order=False))
        assert not ar.same_planes(got, planes)  # the guide is read only
    finally:
        g.close()
        ad.close()
        acc.close()


def _mse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float((d * d).mean())


def test_sample_guided_image_is_closer_to_the_truth_than_the_plain_one(rtlib, gpu_ctx):
    """tests/test_denoise_gpu.py's protocol on big1 -- 192 x 128, 4 samples per frame buffer, the candidates after 16
    frame buffers against the plain image after 2048, mean squared error in 8-bit levels -- with the shipped
    parameters and gains: plain, unguided, guided by the centre planes and guided by planes averaged over 16
    samples.  Asserted: sample-guided < plain.  How it compares with centre-guided is a measurement (DESIGN.md 3.9:
    23.7492, 23.0162, 23.0159 and 23.0163 when this was written)."""
    W, H = 192, 128
    sc = rtlib.Scene.builtin("big1")
    gpu_ctx.upload(sc)
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, 4, 0, 1), 128)
    g = rtlib.Guide(sc)
    try:
        mon = acc.noise_monitor()
        acc.add(16)
        plain, unguided = acc.image(png_order=True), mon.denoise()
        centre = mon.denoise(guide=g.render(W, H))
        sampled = mon.denoise(guide=g.render(W, H, samples=16))
        acc.add(2048 - 16)
        truth = acc.image(png_order=True)
    finally:
        g.close()
        acc.close()
    m = [_mse(x, truth) for x in (plain, unguided, centre, sampled)]
    print(f"big1: mse plain {m[0]:.4f}, unguided {m[1]:.4f}, centre-guided {m[2]:.4f}, sample-guided {m[3]:.4f}")
    assert m[3] < m[0]


# ---------------------------------------------------------------- rt_main and the Python drivers
def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    W, H = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data[m.end():], np.uint8).reshape(H, W, 3)


def test_rt_main_guide_samples_and_the_drivers(rtlib, gpu_ctx, tmp_path):
    assert os.path.exists(RT_MAIN), "examples/bin/rt_main not built (python -m raytracing_gpu_amd._build)"
    out, den, aov = str(tmp_path / "out.ppm"), str(tmp_path / "den.ppm"), str(tmp_path / "aov")
    den0, aov0 = str(tmp_path / "den0.ppm"), str(tmp_path / "aov0")
    base = [RT_MAIN, "big1", "96", "2", "3", out, "--progressive", "2"]
    p = subprocess.run(base + ["--denoise", den, "--guided", "--aov", aov, "--guide-samples", "8"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines[0]["aov"] == aov and lines[0]["guide_samples"] == 8 and lines[0]["guide_ms"] > 0
    p = subprocess.run(base + ["--denoise", den0, "--guided", "--aov", aov0], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    first = json.loads(p.stdout.splitlines()[0])
    assert first["aov"] == aov0 and "guide_samples" not in first and not os.path.exists(aov0 + "_coverage.ppm")
    for extra in (["--guide-samples", "8"], ["--aov", aov, "--guide-samples", "0"], ["--aov", aov, "--guide-samples", "257"]):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "--guide-samples" in p.stderr  # alone, or out of range
    H = _read_ppm(out).shape[0]
    scene = rtlib.Scene.builtin("big1")
    gpu_ctx.upload(scene)
    acc = gpu_ctx.accumulator(rtlib.make_args(96, H, 2, 0, 1, 50, REF, seed=1984), 2)
    g = rtlib.Guide(scene)
    try:
        mon = acc.noise_monitor()
        acc.add(3)
        # without the flag: the centre pass, as before
        g.render(96, H)
        want0 = mon.denoise(guide=g)
        assert np.array_equal(_read_ppm(aov0 + "_normal.ppm"), g.image("normal")) and np.array_equal(_read_ppm(aov0 + "_albedo.ppm"), g.image("albedo"))
        assert np.array_equal(_read_ppm(den0), want0)
        g.render(96, H, samples=8)
        want = mon.denoise(guide=g)
        assert np.array_equal(_read_ppm(aov + "_normal.ppm"), g.image("normal")) and np.array_equal(_read_ppm(aov + "_albedo.ppm"), g.image("albedo"))
        grey = dr.quant(g.coverage())
        assert np.array_equal(_read_ppm(aov + "_coverage.ppm"), np.repeat(grey[..., None], 3, axis=2))
        assert np.array_equal(_read_ppm(den), want) and not np.array_equal(g.image("albedo"), _read_ppm(aov0 + "_albedo.ppm"))
    finally:
        g.close()
        acc.close()
    s = rtlib.render_settings(image_width=96, image_height=H, samples_per_pixel_per_fb=2, no_fb=3)
    img, _ = rtlib.draw_progressive(scene, s, ctx=gpu_ctx, every=2, denoise=dict(guide=True, guide_samples=8))
    assert np.array_equal(img, want)
    img, _ = rtlib.draw_progressive(scene, s, ctx=gpu_ctx, every=2, denoise=dict(guide=True))  # without the key: as before
    assert np.array_equal(img, want0)
    prm = dict(search_radius=4, patch_radius=1)
    ck = str(tmp_path / "adaptive.ck")
    img, _, counts = rtlib.draw_adaptive(scene, s, ctx=gpu_ctx, every=1, until_noise=1.0, min_fbs=2, checkpoint=ck,
                                         denoise=dict(prm, guide=True, guide_params=GAINS, guide_samples=8))
    assert counts.min() >= 2
    planes = rtlib.guide_host(scene, 96, H, samples=8)
    assert np.array_equal(img, rtlib.denoise_adaptive_checkpoint(ck, prm, guide=planes, guide_params=GAINS)[::-1])
    assert not np.array_equal(img, rtlib.denoise_adaptive_checkpoint(ck, prm, guide=rtlib.guide_host(scene, 96, H), guide_params=GAINS)[::-1])
