"""Progressive accumulator on the GPU (rt_accum_* of include/rt_hip.h): draw() cut after any frame
buffer is byte-identical to the one-shot rt_draw, to rt_render + rt_resolve of the same prefix and to
the CPU oracle's draw(); checkpoints continue bit-identically; examples/rt_main --progressive /
--checkpoint."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
REF, PIX = 0, 1
RT_ERR_ARG, RT_ERR_STATE = 1, 3

_oracle_draws = {}


def _oracle_prefix_images(oracle, scene, W, H, spp, nfb, cam=REF):
    """[image of the first k frame buffers for k = 1..nfb] (PNG order) and the total counters: one
    oracle.draw of nfb frame buffers, its prefixes folded as oracle.draw folds them."""
    key = (scene, W, H, spp, nfb, cam)
    if key not in _oracle_draws:
        img, fbs, tot = oracle.draw(scene, W, H, spp, nfb, cam_mode=cam)
        qs = [oracle.quantize_fb(fb, W, H) for fb in fbs]
        pre = [oracle.average(qs[:k], W, H) for k in range(1, nfb + 1)]
        assert np.array_equal(pre[-1], img)
        _oracle_draws[key] = (pre, tot)
    return _oracle_draws[key]


def _status(rtlib, fn):
    with pytest.raises(rtlib.RtError) as e:
        fn()
    return e.value.status


# ---------------------------------------------------------------- the kernels alone (add_fbs)
def _random_fbs(nfb, n, special=False):
    rng = np.random.default_rng(1000 + n + nfb)
    fbs = rng.uniform(-0.3, 1.3, (nfb, n)).astype(np.float32)
    fbs[rng.random(fbs.shape) < 0.05] = 0.0
    if special:
        for v in (np.nan, np.inf, -np.inf, -1.0, -0.0, 1e30, 1e-30):
            fbs[rng.random(fbs.shape) < 0.03] = v
    return fbs


@pytest.mark.parametrize("W,H,groups,mode", [
    (17, 9, (2, 1, 2), "device"),     # per_fb = 459, odd: the scalar kernel
    (64, 36, (2, 1, 1), "device"),    # per_fb % 4 == 0, aligned: the 16-byte kernel
    (64, 36, (2, 1, 1), "offset"),    # the same at a pointer one float off: the scalar kernel again
    (64, 36, (2, 1, 1), "host"),      # staged from host memory
    (17, 9, (2, 1, 2), "host"),
    (64, 36, (2, 1, 1), "special"),   # NaN, +-inf, negatives (against rt_resolve only)
    (17, 9, (2, 1, 2), "special"),
    (66, 2, (1, 3), "device"),        # per_fb = 396 = 4 x 99: 16-byte kernel, lanes of a wave past the end
    (300, 7, (3, 2), "device"),       # per_fb = 6300: several blocks, the last one part full
])
def test_add_fbs_matches_resolve_and_oracle(rtlib, gpu_ctx, oracle, W, H, groups, mode):
    import torch

    nfb, n = sum(groups), W * H * 3
    fbs = _random_fbs(nfb, n, special=mode == "special")
    gpu_ctx.upload(rtlib.Scene.builtin("basic"))
    args = rtlib.make_args(W, H, 1, 0, 1)
    off = 1 if mode == "offset" else 0
    dev = torch.zeros(nfb * n + off, dtype=torch.float32, device="cuda")
    dev[off:] = torch.from_numpy(fbs.reshape(-1)).cuda()
    base = dev.data_ptr() + 4 * off
    assert base % 16 == (4 if off else 0)
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    qs = [oracle.quantize_fb(f, W, H) for f in fbs] if mode != "special" else None
    acc = gpu_ctx.accumulator(args)
    try:
        done = 0
        for g in groups:
            if mode == "host":
                acc.add_fbs(fbs[done:done + g].ctypes.data, g)
            else:
                acc.add_fbs(base + 4 * n * done, g)
            done += g
            assert acc.done == done
            got = acc.image()
            r = rtlib.make_args(W, H, 1, 0, done)
            gpu_ctx.resolve(r, base, out.data_ptr())
            want = out.cpu().numpy().reshape(H, W, 3)
            assert np.array_equal(got, want), f"after {done} frame buffers: differs from rt_resolve"
            if qs is not None:
                assert np.array_equal(got[::-1], oracle.average(qs[:done], W, H)), f"after {done}: differs from the oracle"
            # the image into device memory (4-byte aligned and not) is the same image
            o2 = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
            for o in (0, 1):
                acc.image_into(o2.data_ptr() + o)
                torch.cuda.synchronize()
                assert np.array_equal(o2.cpu().numpy()[o:o + n].reshape(H, W, 3), want)
    finally:
        acc.close()


# ---------------------------------------------------------------- progressive == one-shot
PROG = [("big1", 96, 54, 2, 5, REF), ("cornell_smoke", 48, 48, 3, 4, PIX)]
_gpu_draws = {}


def _gpu_draw(rtlib, ctx, scene, W, H, spp, nfb, cam):
    key = (scene, W, H, spp, nfb, cam)
    if key not in _gpu_draws:
        ctx.upload(rtlib.Scene.builtin(scene))
        _gpu_draws[key] = ctx.draw_args(rtlib.make_args(W, H, spp, 0, nfb, 50, cam))
    return _gpu_draws[key]


@pytest.mark.parametrize("chunk,step", [(1, 1), (2, 1), (8, 1), (2, 0)], ids=["chunk1", "chunk2", "chunk8", "one_call_chunk2"])
@pytest.mark.parametrize("scene,W,H,spp,nfb,cam", PROG)
def test_progressive_equals_one_shot(rtlib, gpu_ctx, oracle, scene, W, H, spp, nfb, cam, chunk, step):
    one, cnt1 = _gpu_draw(rtlib, gpu_ctx, scene, W, H, spp, nfb, cam)
    pre, tot = _oracle_prefix_images(oracle, scene, W, H, spp, nfb, cam)
    gpu_ctx.upload(rtlib.Scene.builtin(scene))
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, spp, 0, 1, 50, cam), chunk_fbs=chunk)
    try:
        segs = samples = 0
        while acc.done < nfb:
            c = acc.add(step or nfb)  # step 0: every frame buffer in one call, ceil(nfb / chunk) launches
            segs += c["segments"]
            samples += c["samples"]
            assert np.array_equal(acc.image(png_order=True), pre[acc.done - 1]), f"preview {acc.done}"
        final = acc.image(png_order=True)
        assert np.array_equal(final, one) and np.array_equal(final, pre[-1])
        assert np.array_equal(acc.image()[::-1], final)
        assert segs == cnt1["segments"] == tot["segments"]
        assert samples == cnt1["samples"] == W * H * spp * nfb
        i = acc.info()
        assert (i["fb_count"], i["fb_first"], i["n_values"], i["width"], i["spp"]) == (nfb, 0, W * H * 3, W, spp)
    finally:
        acc.close()


def test_nonzero_fb_first(rtlib, gpu_ctx):
    import torch

    W, H, spp, first, nfb = 80, 45, 2, 4, 2
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    gpu_ctx.render_init(W, H, 1984)
    args = rtlib.make_args(W, H, spp, first, nfb)
    fb = torch.zeros(nfb * H * W * 3, dtype=torch.float32, device="cuda")
    out = torch.zeros(H * W * 3, dtype=torch.uint8, device="cuda")
    cnt = gpu_ctx.render(args, fb.data_ptr())
    gpu_ctx.resolve(args, fb.data_ptr(), out.data_ptr())
    want = out.cpu().numpy().reshape(H, W, 3)
    acc = gpu_ctx.accumulator(rtlib.make_args(W, H, spp, first, 99))  # fb_count is ignored
    try:
        c = acc.add(nfb)
        assert np.array_equal(acc.image(), want)
        assert c["segments"] == cnt["segments"] and acc.info()["fb_first"] == first and acc.done == nfb
    finally:
        acc.close()


def test_band_tiling_two_accumulators(rtlib, gpu_ctx):
    W, H, spp, nfb = 80, 45, 2, 3
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    one, cnt1 = gpu_ctx.draw_args(rtlib.make_args(W, H, spp, 0, nfb))
    parts = [rtlib.make_args(W, H, spp, 0, 1, band_rows=4, band_first=b, band_stride=2) for b in (0, 1)]
    accs = [gpu_ctx.accumulator(a, chunk_fbs=2) for a in parts]
    try:
        whole = np.zeros((H, W, 3), np.uint8)
        segs = 0
        for a, acc in zip(parts, accs):
            segs += acc.add(nfb)["segments"]
        for a, acc in zip(parts, accs):
            rows = rtlib.owned_rows(a)
            img = acc.image()
            assert img.shape == (len(rows), W, 3) and acc.info()["n_values"] == len(rows) * W * 3
            whole[rows] = img
            assert _status(rtlib, lambda: acc.image(png_order=True)) == RT_ERR_ARG
        assert sorted(np.concatenate([rtlib.owned_rows(a) for a in parts])) == list(range(H))
        assert len(rtlib.owned_rows(parts[1])) == 21  # five whole bands and row 44, the short last band
        assert np.array_equal(whole[::-1], one)
        assert segs == cnt1["segments"]
    finally:
        for acc in accs:
            acc.close()


# ---------------------------------------------------------------- checkpoints and errors
def test_checkpoint_resume_and_errors(rtlib, gpu_ctx, oracle, tmp_path):
    import torch

    scene, W, H, spp, nfb = "big1", 96, 54, 2, 5
    pre, _ = _oracle_prefix_images(oracle, scene, W, H, spp, nfb, REF)
    gpu_ctx.upload(rtlib.Scene.builtin(scene))
    args = rtlib.make_args(W, H, spp, 0, 1)
    assert _status(rtlib, lambda: gpu_ctx.accumulator(args, chunk_fbs=0)) == RT_ERR_ARG
    acc = gpu_ctx.accumulator(args, chunk_fbs=2)
    ck = str(tmp_path / "ck.bin")
    try:
        assert _status(rtlib, acc.image) == RT_ERR_STATE  # nothing folded in yet
        assert _status(rtlib, lambda: acc.add(0)) == RT_ERR_ARG
        assert _status(rtlib, lambda: acc.add_fbs(0, 1)) == RT_ERR_ARG
        dev = torch.zeros(16, dtype=torch.uint8, device="cuda")
        acc.add(2)
        assert _status(rtlib, lambda: acc.image_into(dev.data_ptr(), png_order=True)) == RT_ERR_ARG  # device + png order
        preview2 = acc.image(png_order=True)
        assert np.array_equal(preview2, pre[1])
        acc.save(ck)
        fp = acc.info()["scene_fp"]
    finally:
        acc.close()
    assert [p.name for p in tmp_path.iterdir()] == ["ck.bin"]  # the temporary name is gone
    # the file alone, without a context: the host-only functions
    info, img = rtlib.read_checkpoint(ck)
    assert info["fb_count"] == 2 and info["scene_fp"] == fp and np.array_equal(img[::-1], preview2)
    # the same scene uploaded again (another generation, same fingerprint): load and continue
    gpu_ctx.upload(rtlib.Scene.builtin(scene))
    acc = rtlib.Accumulator.load(gpu_ctx, ck, chunk_fbs=2)
    try:
        assert acc.done == 2 and acc.info() == info
        assert np.array_equal(acc.image(png_order=True), preview2)
        acc.add(3)
        assert np.array_equal(acc.image(png_order=True), pre[4])
        # the scene uploaded once more: this accumulator's scene is gone
        gpu_ctx.upload(rtlib.Scene.builtin(scene))
        assert _status(rtlib, lambda: acc.add(1)) == RT_ERR_STATE
        assert acc.done == 5
    finally:
        acc.close()
    # another scene: the checkpoint does not belong to it
    gpu_ctx.upload(rtlib.Scene.builtin("basic"))
    assert _status(rtlib, lambda: rtlib.Accumulator.load(gpu_ctx, ck)) == RT_ERR_STATE
    bad = tmp_path / "bad.bin"
    bad.write_bytes(open(ck, "rb").read()[:-4])
    assert _status(rtlib, lambda: rtlib.Accumulator.load(gpu_ctx, str(bad))) == RT_ERR_ARG


def test_draw_progressive_python(rtlib, gpu_ctx, oracle, tmp_path):
    """draw_progressive: a callback per step, the checkpoint rewritten per step, and a second call
    that continues from it."""
    scene, W, H, spp, nfb = "big1", 96, 54, 2, 5
    pre, tot = _oracle_prefix_images(oracle, scene, W, H, spp, nfb, REF)
    ck = str(tmp_path / "draw.ck")
    seen = []
    s = rtlib.render_settings(image_width=W, image_height=H, samples_per_pixel_per_fb=spp, no_fb=3)
    img, _ = rtlib.draw_progressive(rtlib.Scene.builtin(scene), s, ctx=gpu_ctx, every=2, checkpoint=ck,
                                    on_image=lambda im, k: seen.append((k, im.copy())))
    assert [k for k, _ in seen] == [2, 3]
    assert all(np.array_equal(im, pre[k - 1]) for k, im in seen) and np.array_equal(img, pre[2])
    assert rtlib.read_checkpoint(ck)[0]["fb_count"] == 3
    s.no_fb = nfb
    seen.clear()
    img, cnt = rtlib.draw_progressive(rtlib.Scene.builtin(scene), s, ctx=gpu_ctx, every=2, checkpoint=ck,
                                      on_image=lambda im, k: seen.append((k, im.copy())))
    assert [k for k, _ in seen] == [5] and np.array_equal(img, pre[4])
    assert cnt["samples"] == W * H * spp * 2  # only frame buffers 3 and 4 were rendered by this call
    s.samples_per_pixel_per_fb = spp + 1  # other settings: the checkpoint is refused
    with pytest.raises(rtlib.RtError):
        rtlib.draw_progressive(rtlib.Scene.builtin(scene), s, ctx=gpu_ctx, checkpoint=ck)


# ---------------------------------------------------------------- examples/rt_main
def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    W, H = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data[m.end():], np.uint8).reshape(H, W, 3)


def _rt_main(tmp_path, *args):
    out = str(tmp_path / "out.ppm")
    p = subprocess.run([RT_MAIN, *map(str, args[:4]), out, *map(str, args[4:])], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    return _read_ppm(out), [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]


def test_rt_main_progressive_and_resume(oracle, tmp_path):
    assert os.path.exists(RT_MAIN), "examples/bin/rt_main not built (python -m raytracing_gpu_amd._build)"
    ck = str(tmp_path / "ck.bin")
    img, lines = _rt_main(tmp_path, "big1", 96, 2, 3, "--progressive", 1, "--checkpoint", ck)
    H = img.shape[0]  # rt_main's own calc_all(): int(96 / aspect)
    pre, tot = _oracle_prefix_images(oracle, "big1", 96, H, 2, 5, REF)
    assert img.shape == (H, 96, 3) and np.array_equal(img, pre[2])
    assert [x["fbs_done"] for x in lines if "fbs_done" in x] == [1, 2, 3]
    assert not [x for x in lines if "resumed_from" in x]
    img, lines = _rt_main(tmp_path, "big1", 96, 2, 5, "--progressive", 1, "--checkpoint", ck)
    assert [x["resumed_from"] for x in lines if "resumed_from" in x] == [3]
    assert [x["fbs_done"] for x in lines if "fbs_done" in x] == [4, 5]
    assert np.array_equal(img, pre[4])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ck.bin", "out.ppm"]  # temporaries renamed away
    # without the two options the program is the one-shot draw it was
    one, l1 = _rt_main(tmp_path, "big1", 96, 2, 5)
    assert np.array_equal(one, img) and l1[-1]["segments"] == tot["segments"] and "fbs_done" not in l1[-1]
