"""Denoiser on the GPU (rt_denoise_* of include/rt_hip.h): the device kernels of csrc/rt_denoise.hip equal the
host-only twin on the saved state byte for byte -- the image and the gain as float bits -- for a monitor and for
an adaptive accumulator with mixed counts; denoising changes no state and a monitor that is never denoised
changes nothing; with the shipped parameters the denoised image after 16 frame buffers is closer to the image
after 2048 than the plain one is; draw_progressive(denoise=True) and rt_main --denoise give the same bytes."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import noise_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
REF, PIX = 0, 1
RT_ERR_ARG, RT_ERR_STATE = 1, 3
NFB = 4


def _twin(rtlib, fn, blob, params, W, H):
    img = np.zeros((H, W, 3), np.uint8)
    gain = np.zeros((H, W), np.float32)
    p = rtlib.denoise_params(params)
    assert fn(blob, len(blob), ctypes.byref(p), img.ctypes.data, gain.ctypes.data) == 0
    return img, gain


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: {int((got[0] != want[0]).sum())} image bytes differ"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), f"{what}: gain bits"


# The filter's output tile is 32 x 32.  5 x 3: smaller than the window and than a tile; 16 x 16 and 32 x 32:
# exactly one noise tile, exactly one output tile; 37 x 21: partial tiles on the right edge; 50 x 35 and 65 x 33
# at the largest radii: halos span several tiles, the latter with one-pixel tiles on both edges; 130 x 3: wide and
# thin.  Every patch radius (a kernel instance each) occurs.
@pytest.mark.parametrize("W,H,R,f", [(5, 3, 10, 3), (16, 16, 4, 2), (32, 32, 2, 1), (37, 21, 3, 1), (50, 35, 10, 3),
                                     (65, 33, 10, 3), (130, 3, 5, 0)])
def test_device_equals_host_twin(rtlib, gpu_ctx, W, H, R, f):
    import torch

    n = W * H * 3
    fbs = nr.random_fbs(NFB, n, 9100 + n, special=True)
    gpu_ctx.upload(rtlib.Scene.builtin("basic"))
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, 1, 0, 1))
    try:
        mon = acc.noise_monitor()
        acc.add_fbs(fbs.ctypes.data, NFB)
        before = (acc.blob(), mon.blob())
        prm = dict(search_radius=R, patch_radius=f, k=0.45, alpha=1.0, eps=1.0)
        want = _twin(rtlib, rtlib.lib().rt_denoise_monitor_blob, before[1], prm, W, H)
        assert want[1].max() > 1.0  # something was averaged
        # host pointers, both row orders
        _same(mon.denoise(prm, png_order=False, gain=True), want, "host, rows ascending")
        assert mon.last_denoise_ms() > 0.0
        _same(mon.denoise(prm, png_order=True, gain=True), (want[0][::-1], want[1][::-1]), "host, png order")
        assert np.array_equal(mon.denoise(prm, png_order=False), want[0])  # the gain is optional
        # device pointers
        img_d = torch.zeros(n, dtype=torch.uint8, device="cuda")
        gain_d = torch.zeros(W * H, dtype=torch.float32, device="cuda")
        mon.denoise_into(img_d.data_ptr(), gain_d.data_ptr(), prm)
        torch.cuda.synchronize()
        _same((img_d.cpu().numpy().reshape(H, W, 3), gain_d.cpu().numpy().reshape(H, W)), want, "device")
        # png order needs host memory; nothing is written
        with pytest.raises(rtlib.RtError) as e:
            mon.denoise_into(img_d.data_ptr(), 0, prm, png_order=True)
        assert e.value.status == RT_ERR_ARG
        with pytest.raises(rtlib.RtError) as e:
            mon.denoise(dict(prm, k=0.0))
        assert e.value.status == RT_ERR_ARG
        # no state changed
        assert (acc.blob(), mon.blob()) == before
    finally:
        acc.close()


def test_denoise_needs_two_frame_buffers_and_the_whole_image(rtlib, gpu_ctx):
    W, H = 20, 12
    fbs = nr.random_fbs(2, W * H * 3, 5)
    gpu_ctx.upload(rtlib.Scene.builtin("basic"))
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, 1, 0, 1))
    try:
        mon = acc.noise_monitor()
        acc.add_fbs(fbs.ctypes.data, 1)
        with pytest.raises(rtlib.RtError) as e:
            mon.denoise()
        assert e.value.status == RT_ERR_STATE
        acc.add_fbs(fbs[1:].ctypes.data, 1)
        assert mon.denoise().shape == (H, W, 3)
    finally:
        acc.close()
    band = gpu_ctx.accumulator(rtlib.make_args(W, H, 1, 0, 1, band_rows=4, band_first=0, band_stride=2))
    try:
        mon = band.noise_monitor()
        rows = len(rtlib.owned_rows(rtlib.make_args(W, H, 1, 0, 1, band_rows=4, band_first=0, band_stride=2)))
        band.add_fbs(nr.random_fbs(2, rows * W * 3, 6).ctypes.data, 2)
        with pytest.raises(rtlib.RtError) as e:
            mon.denoise(png_order=False)
        assert e.value.status == RT_ERR_ARG
    finally:
        band.close()


@pytest.mark.parametrize("scene", ["cornell_smoke"])
def test_adaptive_device_equals_host_twin_and_changes_no_state(rtlib, gpu_ctx, scene):
    W, H = 64, 48
    gpu_ctx.upload(rtlib.Scene.builtin(scene))
    ad = gpu_ctx.adaptive(rtlib.make_args(W, H, 2, 0, 1, cam_mode=PIX), chunk_fbs=3)
    try:
        ad.add(2)
        nmap = ad.noise_map()
        thr = float(np.median(nmap[nmap > 0]))
        above = nr.tiles(nmap, thr)[1]
        max_above = int(np.median(above))
        assert above.min() <= max_above < above.max()
        ad.retire(thr, max_above)  # the tiles with fewer noisy pixels stop at 2
        ad.add(3)
        counts = ad.counts()
        assert set(np.unique(counts)) == {2, 5}
        before = ad.blob()
        for R, f in [(10, 3), (3, 1)]:
            prm = dict(search_radius=R, patch_radius=f)
            want = _twin(rtlib, rtlib.lib().rt_denoise_adaptive_blob, before, prm, W, H)
            _same(ad.denoise(prm, png_order=False, gain=True), want, f"adaptive ({R}, {f})")
            _same(ad.denoise(prm, png_order=True, gain=True), (want[0][::-1], want[1][::-1]), "adaptive, png order")
        assert ad.last_denoise_ms() > 0.0
        assert ad.blob() == before  # the checkpoint after denoising is the one before
        assert np.array_equal(ad.counts(), counts)
    finally:
        ad.close()


def test_monitor_never_denoised_and_denoise_in_between_change_nothing(rtlib, gpu_ctx):
    """A 64 x 48 progressive draw with a denoise between its steps: image, checkpoint and monitor file are those
    of the draw without that call."""
    W, H = 64, 48
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    args = rtlib.make_args(W, H, 2, 0, 1)
    out = []
    for denoise in (False, True):
        acc = gpu_ctx.accumulator(args, 2)
        try:
            mon = acc.noise_monitor()
            acc.add(2)
            if denoise:
                mon.denoise()
                mon.denoise(dict(search_radius=2, patch_radius=0), gain=True)
            acc.add(2)
            out.append((acc.image(png_order=True).tobytes(), acc.blob(), mon.blob()))
        finally:
            acc.close()
    assert out[0] == out[1]


def _mse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float((d * d).mean())


@pytest.mark.parametrize("scene", ["big1", "cornell_smoke"])
def test_denoised_image_is_closer_to_the_truth(rtlib, gpu_ctx, scene):
    """192 x 128 at 4 samples per frame buffer: the mean squared error in 8-bit levels against the plain image
    after 2048 frame buffers, of the plain and of the denoised image after 16, with the shipped parameters."""
    W, H = 192, 128
    gpu_ctx.upload(rtlib.Scene.builtin(scene))
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, 4, 0, 1), 128)
    try:
        mon = acc.noise_monitor()
        acc.add(16)
        plain = acc.image(png_order=True)
        denoised, gain = mon.denoise(gain=True)
        acc.add(2048 - 16)
        truth = acc.image(png_order=True)
    finally:
        acc.close()
    mse_plain, mse_denoised = _mse(plain, truth), _mse(denoised, truth)
    print(f"{scene}: mse plain {mse_plain:.3f}, denoised {mse_denoised:.3f}, ratio {mse_denoised / mse_plain:.4f}, "
          f"mean gain {float(gain.mean()):.2f}")
    assert mse_denoised < mse_plain


def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    W, H = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data[m.end():], np.uint8).reshape(H, W, 3)


def test_draw_progressive_and_rt_main_denoise(rtlib, gpu_ctx, tmp_path):
    assert os.path.exists(RT_MAIN), "examples/bin/rt_main not built (python -m raytracing_gpu_amd._build)"
    out, out2 = str(tmp_path / "out.ppm"), str(tmp_path / "den.ppm")
    p = subprocess.run([RT_MAIN, "big1", "96", "2", "3", out, "--progressive", "2", "--denoise", out2], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert [x["fbs_done"] for x in lines if "fbs_done" in x] == [2, 3] and not [x for x in lines if "noise_max" in x]
    assert lines[-1]["denoised"] == out2 and lines[-1]["fbs"] == 3 and lines[-1]["denoise_ms"] > 0
    plain_main, den_main = _read_ppm(out), _read_ppm(out2)
    H = plain_main.shape[0]
    # the same state by hand
    scene = rtlib.Scene.builtin("big1")
    gpu_ctx.upload(scene)
    acc = gpu_ctx.accumulator(rtlib.make_args(96, H, 2, 0, 1, 50, REF, seed=1984), 2)
    try:
        mon = acc.noise_monitor()
        acc.add(3)
        plain, want = acc.image(png_order=True), mon.denoise()
    finally:
        acc.close()
    assert np.array_equal(plain_main, plain) and np.array_equal(den_main, want)
    assert not np.array_equal(want, plain)
    s = rtlib.render_settings(image_width=96, image_height=H, samples_per_pixel_per_fb=2, no_fb=3)
    seen = []
    img, _ = rtlib.draw_progressive(scene, s, ctx=gpu_ctx, every=2, denoise=True, on_image=lambda im, k: seen.append(im.copy()))
    assert np.array_equal(img, want) and np.array_equal(seen[-1], plain)
    img, _ = rtlib.draw_progressive(scene, s, ctx=gpu_ctx, every=2)  # the default: the plain image
    assert np.array_equal(img, plain)
    # the adaptive driver: the denoised image of its final state, which its checkpoint holds
    prm = dict(search_radius=4, patch_radius=1)
    ck = str(tmp_path / "adaptive.ck")
    img, _, counts = rtlib.draw_adaptive(scene, s, ctx=gpu_ctx, every=1, until_noise=1.0, min_fbs=2, checkpoint=ck, denoise=prm)
    assert counts.min() >= 2
    assert np.array_equal(img, rtlib.denoise_adaptive_checkpoint(ck, prm)[::-1])
    assert not np.array_equal(img, rtlib.read_adaptive_checkpoint(ck)[1][::-1])
