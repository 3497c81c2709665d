"""Tile launches and the adaptive accumulator on the GPU (rt_render_tiles, rt_adapt_* of
include/rt_hip.h): a tile launch writes rt_render's floats into the listed tiles and nothing else, its
counters partition rt_render's, it leaves the context's item schedule alone; the adaptive accumulator's
tiles are the oracle's draw() at their own frame-buffer counts, it equals the numpy model of
tests/adapt_ref.py in every integer, and its results do not depend on how the adds were grouped."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import adapt_ref as ar
import noise_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
REF, PIX = 0, 1
RT_ERR_ARG, RT_ERR_STATE = 1, 3
SPP = 2
SMALL, WHOLE = (70, 37), (80, 48)  # 5 x 3 tiles partial in both directions (per_fb = 7770, no multiple of 4); whole tiles
SCENES = ["big1", "cornell_smoke", "triangles"]  # stepwise kernel with the scene in LDS; list world; mesh variant
BAND = dict(band_rows=4, band_stride=2, band_first=1)  # 17 of 37 rows: 5 x 2 tiles
SENTINEL = 0x7FC0BEEF  # a NaN bit pattern no render writes


def _status(rtlib, fn):
    with pytest.raises(rtlib.RtError) as e:
        fn()
    return e.value.status


def _grid(rows, width):
    return (rows + 15) // 16, (width + 15) // 16


def _tile_sets(rows, width):
    ty, tx = _grid(rows, width)
    n = ty * tx
    return {"one": [min(1, ty - 1) * tx + min(2, tx - 1)], "corner": [n - 1], "every_other": list(range(0, n, 2)),
            "all": list(range(n - 1, -1, -1))}  # "all" in descending order: the list's order changes no pixel


def _mask(tiles, rows, width):
    return np.isin(ar.pixel_tiles(rows, width), tiles)


_scene_of = {}


def _upload(rtlib, ctx, scene):
    """Upload scene unless the session context holds it already (an upload drops the schedule)."""
    if _scene_of.get(id(ctx)) != scene:
        ctx.upload(rtlib.Scene.builtin(scene))
        _scene_of[id(ctx)] = scene


@pytest.fixture(autouse=True)
def _forget_scene():
    """Other test modules upload into the session context: never trust the note across tests."""
    _scene_of.clear()
    yield
    _scene_of.clear()


def _render(rtlib, ctx, args):
    """(float frame buffers as uint32 [fb_count][rows][W][3], counters) of plain rt_render."""
    import torch

    rows = len(rtlib.owned_rows(args))
    fb = torch.zeros(args.fb_count * rows * args.width * 3, dtype=torch.float32, device="cuda")
    cnt = ctx.render(args, fb.data_ptr())
    return fb.cpu().numpy().view(np.uint32).reshape(args.fb_count, rows, args.width, 3), cnt


def _sentinel_fb(n):
    import torch

    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")


def _check_tiles(rtlib, ctx, args, ref, host, what):
    rows, W, nfb = ref.shape[1], args.width, args.fb_count
    for name, tiles in _tile_sets(rows, W).items():
        if host:
            buf = np.full(ref.size, SENTINEL, np.int32)
            cnt = ctx.render_tiles(args, tiles, buf.ctypes.data)
            got = buf.view(np.uint32).reshape(ref.shape)
        else:
            dev = _sentinel_fb(ref.size)
            cnt = ctx.render_tiles(args, tiles, dev.data_ptr())
            got = dev.cpu().numpy().view(np.uint32).reshape(ref.shape)
        m = _mask(tiles, rows, W)
        want = np.full(ref.shape, SENTINEL, np.int32).view(np.uint32)
        want[:, m] = ref[:, m]
        assert np.array_equal(got[:, m], ref[:, m]), f"{what} {name}: listed pixels differ from rt_render"
        assert np.array_equal(got, want), f"{what} {name}: floats outside the listed tiles were written"
        assert cnt["samples"] == int(m.sum()) * nfb * args.spp, f"{what} {name}"
        assert ctx.last_render_schedule() == 0 and ctx.last_kernel_ms() > 0.0
        assert ctx.last_render_kernel().startswith("render_")


# ---------------------------------------------------------------- 1. tile launches against rt_render
@pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "pix"])
@pytest.mark.parametrize("nfb,first", [(1, 0), (1, 5), (3, 0), (3, 5)])
@pytest.mark.parametrize("size", [SMALL, WHOLE], ids=["70x37", "80x48"])
@pytest.mark.parametrize("scene", SCENES)
def test_tile_launch_equals_render(rtlib, gpu_ctx, scene, size, nfb, first, cam):
    W, H = size
    _upload(rtlib, gpu_ctx, scene)
    gpu_ctx.render_init(W, H, 1984)
    args = rtlib.make_args(W, H, SPP, first, nfb, 50, cam)
    ref, _ = _render(rtlib, gpu_ctx, args)
    kernel = gpu_ctx.last_render_kernel()
    _check_tiles(rtlib, gpu_ctx, args, ref, False, f"{scene} {W}x{H}")
    assert gpu_ctx.last_render_kernel() == kernel  # the variant rt_render picks


@pytest.mark.parametrize("how", ["host", "band", "band_host"])
@pytest.mark.parametrize("scene", SCENES)
def test_tile_launch_host_fb_and_band_tiling(rtlib, gpu_ctx, scene, how):
    W, H = SMALL
    _upload(rtlib, gpu_ctx, scene)
    gpu_ctx.render_init(W, H, 1984)
    args = rtlib.make_args(W, H, SPP, 5, 3, 50, PIX, **(BAND if "band" in how else {}))
    ref, _ = _render(rtlib, gpu_ctx, args)
    assert ref.shape[1] == (17 if "band" in how else 37)
    _check_tiles(rtlib, gpu_ctx, args, ref, "host" in how, f"{scene} {how}")


def test_tile_launch_flags_and_stats(rtlib, gpu_ctx):
    """The schedule flags have no effect; stats and the other flags behave as in rt_render."""
    W, H = SMALL
    _upload(rtlib, gpu_ctx, "big1")
    gpu_ctx.render_init(W, H, 1984)
    base = rtlib.make_args(W, H, SPP, 1, 2, 50, REF)
    ref, _ = _render(rtlib, gpu_ctx, base)
    tiles = _tile_sets(H, W)["every_other"]
    m = _mask(tiles, H, W)
    for kw in (dict(schedule=False), dict(split=False), dict(fresh=True), dict(stats=True), dict(lds=False),
               dict(step=False), dict(bins=False), dict(exact=True)):
        args = rtlib.make_args(W, H, SPP, 1, 2, 50, REF, **kw)
        dev = _sentinel_fb(ref.size)
        cnt = gpu_ctx.render_tiles(args, tiles, dev.data_ptr())
        got = dev.cpu().numpy().view(np.uint32).reshape(ref.shape)
        assert np.array_equal(got[:, m], ref[:, m]) and (got[:, ~m] == np.uint32(SENTINEL)).all(), kw
        assert cnt["samples"] == int(m.sum()) * 2 * SPP and gpu_ctx.last_render_schedule() == 0, kw
        if kw.get("stats"):
            assert cnt["node_tests"] > 0 and cnt["prim_tests"] > 0


# ---------------------------------------------------------------- 2. counters partition
@pytest.mark.parametrize("scene", SCENES)
def test_tile_counters_partition_render(rtlib, gpu_ctx, scene):
    import torch

    W, H = SMALL
    _upload(rtlib, gpu_ctx, scene)
    gpu_ctx.render_init(W, H, 1984)
    args = rtlib.make_args(W, H, SPP, 2, 3, 50, REF)
    _, whole = _render(rtlib, gpu_ctx, args)
    part = _tile_sets(H, W)["every_other"]
    rest = sorted(set(range(15)) - set(part))
    fb = torch.zeros(3 * H * W * 3, dtype=torch.float32, device="cuda")
    a, b = gpu_ctx.render_tiles(args, part, fb.data_ptr()), gpu_ctx.render_tiles(args, rest, fb.data_ptr())
    assert a["segments"] > 0 and b["segments"] > 0
    for k in ("segments", "samples"):
        assert a[k] + b[k] == whole[k], k


# ---------------------------------------------------------------- 3. schedule isolation
@pytest.mark.parametrize("tile_first", [0, 5], ids=["same_fbs", "other_fbs"])
def test_tile_launch_leaves_the_schedule_alone(rtlib, gpu_ctx, tile_first):
    W, H, nfb = SMALL[0], SMALL[1], 2
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))  # a fresh upload: A's first launch is cold
    gpu_ctx.render_init(W, H, 1984)
    A = rtlib.make_args(W, H, SPP, 0, nfb, 50, REF)
    fb1, _ = _render(rtlib, gpu_ctx, A)
    assert not gpu_ctx.last_render_schedule() & rtlib.RT_SCHED_PREVIOUS
    fb2, _ = _render(rtlib, gpu_ctx, A)
    assert gpu_ctx.last_render_schedule() & rtlib.RT_SCHED_PREVIOUS
    T = rtlib.make_args(W, H, SPP, tile_first, nfb, 50, REF)
    half = _tile_sets(H, W)["every_other"]
    dev = _sentinel_fb(fb1.size)
    gpu_ctx.render_tiles(T, half, dev.data_ptr())
    assert gpu_ctx.last_render_schedule() == 0
    if tile_first == 0:
        m = _mask(half, H, W)
        assert np.array_equal(dev.cpu().numpy().view(np.uint32).reshape(fb1.shape)[:, m], fb1[:, m])
    fb3, _ = _render(rtlib, gpu_ctx, A)
    assert gpu_ctx.last_render_schedule() & rtlib.RT_SCHED_PREVIOUS, "the tile launch dropped A's schedule"
    assert np.array_equal(fb1, fb2) and np.array_equal(fb1, fb3)


# ---------------------------------------------------------------- 4. argument errors
def test_tile_launch_argument_errors(rtlib, gpu_ctx):
    W, H = SMALL
    _upload(rtlib, gpu_ctx, "big1")
    gpu_ctx.render_init(W, H, 1984)
    args = rtlib.make_args(W, H, SPP, 0, 1, 50, REF)
    dev = _sentinel_fb(H * W * 3)
    for tiles in ([], [15], [-1], [3, 7, 3], list(range(15)) + [0]):
        assert _status(rtlib, lambda: gpu_ctx.render_tiles(args, tiles, dev.data_ptr())) == RT_ERR_ARG, tiles
        assert (dev.cpu().numpy() == SENTINEL).all(), tiles
    # fb_count x owned_rows x width > 2^31: refused before fb is looked at (one float of fb exists)
    big = rtlib.make_args(W, H, SPP, 0, (1 << 31) // (W * H) + 1, 50, REF)
    assert _status(rtlib, lambda: gpu_ctx.render_tiles(big, [0], dev.data_ptr())) == RT_ERR_ARG
    assert (dev.cpu().numpy() == SENTINEL).all()


# ---------------------------------------------------------------- the adaptive accumulator
NFB = 8
# Test 5's thresholds, chosen on the CPU: the oracle's 8 frame buffers of each scene at 70 x 37 x 2 spp
# (REF camera) through tests/adapt_ref.py with steps (add 2, retire T, 0) x 4, for T = 0.5 .. 128.  big1
# retires its three sky tiles at 2 for every T up to 64 and at T = 32 the others at 4, 6 and 8 (counts
# 2 / 4 / 6 / 8 in 3 / 1 / 7 / 4 tiles); cornell_smoke's tiles all stay active up to T = 40 and at T = 56
# retire at 4 (1 tile) and 6 (14).  No reference noise value of any step lies within 2000 float32 ulp
# of either threshold, so one ulp of the device's double divide and sqrt cannot move a decision.
ORACLE_T = {"big1": 32.0, "cornell_smoke": 56.0}
# Test 6: the first of these with no reference noise value of any step within 2 ulp of it
PARITY_T = {"big1": [32.0, 28.0, 40.0, 24.0], "cornell_smoke": [56.0, 48.0, 80.0, 52.0], "triangles": [32.0, 16.0, 8.0, 48.0]}


def _settings(rtlib, W, H, no_fb=NFB):
    return rtlib.render_settings(image_width=W, image_height=H, samples_per_pixel_per_fb=SPP, no_fb=no_fb, max_depth=50)


_planes = {}


def _gpu_planes(rtlib, ctx, scene, W, H, cam, band=None):
    """[NFB][rows*W*3] uint8: the 8-bit plane of every single frame buffer, by plain rt_render + rt_resolve
    (the resolve of one frame buffer is quant(float(c * c) / 65025 / 1) = c)."""
    import torch

    key = (scene, W, H, cam, bool(band))
    if key not in _planes:
        _upload(rtlib, ctx, scene)
        ctx.render_init(W, H, 1984)
        out = []
        for f in range(NFB):
            args = rtlib.make_args(W, H, SPP, f, 1, 50, cam, **(band or {}))
            n = len(rtlib.owned_rows(args)) * W * 3
            fb = torch.zeros(n, dtype=torch.float32, device="cuda")
            img = torch.zeros(n, dtype=torch.uint8, device="cuda")
            ctx.render(args, fb.data_ptr())
            ctx.resolve(args, fb.data_ptr(), img.data_ptr())
            out.append(img.cpu().numpy())
        _planes[key] = np.stack(out)
    return _planes[key]


def _run_steps(ad, steps):
    reports = []
    for s in steps:
        if s[0] == "add":
            ad.add(s[1])
        else:
            reports.append(ad.retire(s[1], s[2]))
    return reports


# ---------------------------------------------------------------- 5. the guarantee against the oracle
@pytest.mark.parametrize("scene", ["big1", "cornell_smoke"])
def test_adaptive_tiles_are_the_oracles_draws(rtlib, gpu_ctx, oracle, scene):
    W, H = SMALL
    seen = []
    img, total, counts = rtlib.draw_adaptive(rtlib.Scene.builtin(scene), _settings(rtlib, W, H), ctx=gpu_ctx, every=2,
                                             until_noise=ORACLE_T[scene], max_above=0, min_fbs=2,
                                             on_step=lambda rep, done: seen.append((done, rep)))
    distinct = sorted(set(counts.reshape(-1).tolist()))
    print(scene, "counts", distinct, "pixel_fbs", seen[-1][1]["pixel_fbs"], "of", W * H * seen[-1][0])
    assert len(distinct) >= 2, "nothing retired early: the test would show nothing"
    assert all(2 <= n <= NFB and n % 2 == 0 for n in distinct)
    ref = oracle.RefScene(scene)
    qs, ref_segments = [], 0
    for f in range(NFB):
        fb, c, _ = ref.render(W, H, SPP, f, 50, REF)
        qs.append(oracle.quantize_fb(fb, W, H))
        ref_segments += c["segments"]
    tid = ar.pixel_tiles(H, W)[::-1]  # tiles count rows from the bottom, the PNG-order image from the top
    for n in distinct:
        want = oracle.average(qs[:n], W, H)
        sel = np.isin(tid, np.flatnonzero(counts.reshape(-1) == n))
        assert np.array_equal(img[sel], want[sel]), f"{scene}: tiles with n_t = {n} differ from the oracle's draw(no_fb={n})"
    px = np.bincount(ar.pixel_tiles(H, W).reshape(-1))
    assert seen[-1][1]["pixel_fbs"] == int((px * counts.reshape(-1)).sum())
    assert total["samples"] == seen[-1][1]["pixel_fbs"] * SPP and total["segments"] < ref_segments
    assert [d for d, _ in seen] == list(range(2, seen[-1][0] + 1, 2))


# ---------------------------------------------------------------- 6. model parity
@pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "pix"])
@pytest.mark.parametrize("scene,size,band", [("big1", SMALL, None), ("cornell_smoke", SMALL, None), ("triangles", SMALL, None),
                                             ("big1", WHOLE, None), ("cornell_smoke", SMALL, BAND)],
                         ids=["big1", "smoke", "triangles", "big1_80x48", "smoke_band"])
def test_adaptive_equals_the_model(rtlib, gpu_ctx, scene, size, band, cam):
    W, H = size
    planes = _gpu_planes(rtlib, gpu_ctx, scene, W, H, cam, band)
    args = rtlib.make_args(W, H, SPP, 0, 1, 50, cam, **(band or {}))
    rows = len(rtlib.owned_rows(args))
    thr = None
    for T in PARITY_T[scene]:
        steps = [("add", 2), ("retire", T, 0), ("add", 2), ("retire", T, 1), ("add", 3), ("retire", T, 0), ("add", 1),
                 ("retire", T, 2)]
        model = ar.run(planes, rows, W, steps)
        near = min(int(np.abs(nr.ulps(m) - nr.ulps(np.float32(T))).min()) for m in model["maps"] + [model["noise"]])
        if near > 2:
            thr = T
            break
    assert thr is not None, "every threshold of the list has a reference noise value within 2 ulp"
    _upload(rtlib, gpu_ctx, scene)
    ad = gpu_ctx.adaptive(args, chunk_fbs=2)
    try:
        assert _status(rtlib, ad.image) == RT_ERR_STATE
        ad.add(1)
        assert _status(rtlib, lambda: ad.retire(thr, 0)) == RT_ERR_STATE  # needs two frame buffers
        assert _status(rtlib, ad.noise_map) == RT_ERR_STATE
        ad.add(1)
        reports = _run_steps(ad, steps[1:])
        print(scene, size, "threshold", thr, "counts", np.unique(model["counts"], return_counts=True))
        assert np.array_equal(ad.counts(), model["counts"])
        assert np.array_equal(ad.image(), model["image"])
        if size == SMALL:  # rt_adapt_image's other outputs, through the C ABI
            import torch

            img = ad.image()
            dev = torch.zeros(img.size + 1, dtype=torch.uint8, device="cuda")
            assert dev.data_ptr() % 4 == 0
            gpu_ctx._after_torch()
            for o in (0, 1):  # into device memory, 4-byte aligned and one byte off it: the same image
                assert rtlib.lib().rt_adapt_image(ad._h, ctypes.c_void_p(dev.data_ptr() + o), 0) == 0
                assert np.array_equal(dev.cpu().numpy()[o:o + img.size].reshape(img.shape), img)
            assert rtlib.lib().rt_adapt_image(ad._h, ctypes.c_void_p(dev.data_ptr()), 1) == RT_ERR_ARG  # png order + device
            if band:  # png order needs the whole-image tiling
                assert _status(rtlib, lambda: ad.image(png_order=True)) == RT_ERR_ARG
        for got, want in zip(reports, model["reports"]):
            for k in want:
                if k == "max_noise":
                    assert abs(int(nr.ulps(np.float32(got[k]))) - int(nr.ulps(np.float32(want[k])))) <= 1
                else:
                    assert got[k] == want[k], (k, got, want)
        assert ad.report(thr) == reports[-1]
        nmap = ad.noise_map()
        assert (np.abs(nr.ulps(nmap) - nr.ulps(model["noise"])) <= 1).all()
        assert np.float32(reports[-1]["max_noise"]) == nmap.max()
        assert ad.last_add_ms() > 0.0 and ad.last_retire_ms() > 0.0
    finally:
        ad.close()


# ---------------------------------------------------------------- 7. independence of grouping
@pytest.mark.parametrize("scene", ["big1", "cornell_smoke"])
def test_adaptive_does_not_depend_on_grouping(rtlib, gpu_ctx, scene):
    W, H = SMALL
    T = ORACLE_T[scene]
    _upload(rtlib, gpu_ctx, scene)
    args = rtlib.make_args(W, H, SPP, 0, 1, 50, REF)
    runs = {"chunk1": (1, [("add", 4), ("retire", T, 0), ("add", 4), ("retire", T, 0)]),
            "chunk3": (3, [("add", 4), ("retire", T, 0), ("add", 4), ("retire", T, 0)]),
            "ones": (3, [("add", 1)] * 4 + [("retire", T, 0)] + [("add", 1)] * 4 + [("retire", T, 0)])}
    got = {}
    for name, (chunk, steps) in runs.items():
        ad = gpu_ctx.adaptive(args, chunk_fbs=chunk)
        try:
            reports = _run_steps(ad, steps)
            got[name] = (ad.image(), ad.counts(), ad.noise_map().view(np.uint32), reports)
        finally:
            ad.close()
    assert len(np.unique(got["chunk1"][1])) >= 2, "nothing retired at the first retire"
    for name in ("chunk3", "ones"):
        for k in range(3):
            assert np.array_equal(got[name][k], got["chunk1"][k]), (name, k)
        assert got[name][3] == got["chunk1"][3], name


# ---------------------------------------------------------------- 8. nothing retired
@pytest.mark.parametrize("size", [SMALL, WHOLE], ids=["70x37", "80x48"])
def test_adaptive_with_nothing_retired_is_the_plain_accumulator(rtlib, gpu_ctx, size):
    W, H = size
    _upload(rtlib, gpu_ctx, "cornell_smoke")
    args = rtlib.make_args(W, H, SPP, 3, 1, 50, PIX)
    ad, acc = gpu_ctx.adaptive(args, chunk_fbs=2), gpu_ctx.accumulator(args, 2)
    try:
        mon = acc.noise_monitor()
        for k in (2, 3):
            ad.add(k)
            acc.add(k)
            rep = ad.retire(-1.0, 0)  # every pixel's noise is above a negative threshold: no tile retires
            assert rep["tiles_active"] == rep["tiles_x"] * rep["tiles_y"] and rep["pixels_above"] == rep["pixels"] == W * H
            assert rep["pixel_fbs"] == W * H * rep["fbs"]
            assert np.array_equal(ad.image(), acc.image())
            assert np.array_equal(ad.noise_map().view(np.uint32), mon.map().view(np.uint32))
            assert np.float32(rep["max_noise"]) == np.float32(mon.measure(-1.0)[0]["max_noise"])
        assert (ad.counts() == 5).all()
        assert np.array_equal(ad.image(png_order=True), acc.image(png_order=True))
    finally:
        ad.close()
        acc.close()


# ---------------------------------------------------------------- 9. everything retired
def test_adaptive_with_everything_retired_renders_nothing(rtlib, gpu_ctx):
    W, H = SMALL
    _upload(rtlib, gpu_ctx, "big1")
    args = rtlib.make_args(W, H, SPP, 0, 1, 50, REF)
    ad = gpu_ctx.adaptive(args)
    try:
        first = ad.add(2)
        assert first["samples"] == 2 * W * H * SPP
        rep = ad.retire(1e9, 0)
        assert rep["tiles_active"] == 0 and rep["pixels_active"] == 0 and rep["fbs"] == 2 and rep["pixels_above"] == 0
        img, nmap = ad.image(), ad.noise_map()
        assert ad.add(3) == {k: 0 for k in first}
        assert ad.report(1e9) == rep and ad.retire(1e9, 0) == rep
        assert np.array_equal(ad.image(), img) and np.array_equal(ad.noise_map(), nmap) and (ad.counts() == 2).all()
        # the cap of the noise monitor, before anything is rendered
        assert _status(rtlib, lambda: ad.add(nr.MAX_FBS - 1)) == RT_ERR_ARG
        gpu_ctx.upload(rtlib.Scene.builtin("big1"))
        fresh = gpu_ctx.adaptive(args)
        try:
            gpu_ctx.upload(rtlib.Scene.builtin("big1"))
            assert _status(rtlib, lambda: fresh.add(1)) == RT_ERR_STATE  # another upload since it was created
        finally:
            fresh.close()
    finally:
        ad.close()


# ---------------------------------------------------------------- 10. rt_main --adaptive
def test_rt_main_adaptive_writes_draw_adaptives_image(rtlib, gpu_ctx, tmp_path):
    W, H = SMALL
    out = str(tmp_path / "a.ppm")
    T = ORACLE_T["big1"]
    r = subprocess.run([RT_MAIN, "big1", str(W), str(SPP), str(NFB), out, "--height", str(H), "--adaptive", "2",
                        "--until-noise", str(T), "--max-above", "1", "--min-fbs", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    seen = []
    img, _, counts = rtlib.draw_adaptive(rtlib.Scene.builtin("big1"), _settings(rtlib, W, H), ctx=gpu_ctx, every=2,
                                         until_noise=T, max_above=1, min_fbs=2, on_step=lambda rep, done: seen.append(rep))
    data = open(out, "rb").read()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(head) and data[len(head):] == img.tobytes()
    steps, last = lines[:-1], lines[-1]
    assert len(steps) == len(seen)
    for line, rep in zip(steps, seen):
        assert (line["fbs"], line["tiles_active"], line["pixel_fbs"]) == (rep["fbs"], rep["tiles_active"], rep["pixel_fbs"])
        assert np.float32(line["noise_max"]) == np.float32(rep["max_noise"])
    assert last["stopped_at"] == seen[-1]["fbs"] and last["pixel_fbs"] == seen[-1]["pixel_fbs"]
    for extra in (["--progressive", "2"], ["--checkpoint", str(tmp_path / "c.bin")]):
        r = subprocess.run([RT_MAIN, "big1", str(W), str(SPP), str(NFB), out, "--adaptive", "2", "--until-noise", "1"] + extra,
                           capture_output=True, text=True)
        assert r.returncode == 99 and "cannot be combined" in r.stderr
