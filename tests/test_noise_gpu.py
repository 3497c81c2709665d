"""Noise monitor on the GPU (rt_noise_* of include/rt_hip.h): the fused accumulate kernel leaves the
image and the checkpoint byte-identical and its integer moments equal the numpy reference of
tests/noise_ref.py whatever the grouping, chunking, band tiling or checkpointing; the measure kernel's
counts are exact and its floats within one float32 ulp of the reference (the device's double divide
and sqrt are not assumed correctly rounded: fewer than ten roundings at 2^-53 in the double chain can
move the float result across at most one rounding boundary); draw_progressive(until_noise=...) and
rt_main --until-noise stop where a manual run says they must."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import noise_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
REF, PIX = 0, 1
RT_ERR_ARG, RT_ERR_STATE = 1, 3


def _status(rtlib, fn):
    with pytest.raises(rtlib.RtError) as e:
        fn()
    return e.value.status


def _within_one_ulp(got, want):
    return bool((np.abs(nr.ulps(got) - nr.ulps(want)) <= 1).all())


def _check_measure(rtlib, mon, S1, S2, n, rows, width, what):
    """measure() and map() of a monitor against the reference of its moments and against the host-only
    rt_noise_blob_measure of its own blob."""
    want = nr.noise_map(S1, S2, n, rows, width)
    thr = nr.pick_threshold(want)  # asserts that no reference value lies within 2 ulp of it
    wmax, wabove = nr.tiles(want, thr)
    rep, tmax, tabove = mon.measure(thr)
    nmap = mon.map()
    brc, brep, bmax, babove, bmap = nr.blob_measure(rtlib, mon.blob(), thr, rows, width)
    assert brc == 0
    assert np.array_equal(bmap.view(np.uint32), want.view(np.uint32)), what  # host: bit for bit
    assert rep["pixels_above"] == int((want > np.float32(thr)).sum()) == brep["pixels_above"], what
    assert np.array_equal(tabove, wabove) and np.array_equal(babove, wabove), what
    assert (rep["fbs"], rep["pixels"], rep["tiles_x"], rep["tiles_y"]) == (n, rows * width, (width + 15) // 16, (rows + 15) // 16)
    assert nmap.shape == want.shape and tmax.shape == wmax.shape
    assert _within_one_ulp(nmap, want) and _within_one_ulp(nmap, bmap), what
    assert _within_one_ulp(tmax, wmax) and _within_one_ulp(tmax, bmax), what
    assert _within_one_ulp(np.float32(rep["max_noise"]), want.max()), what
    # what the device reports is consistent with its own map
    dmax, dabove = nr.tiles(nmap, thr)
    assert np.array_equal(tmax.view(np.uint32), dmax.view(np.uint32)) and np.array_equal(tabove, dabove), what
    assert np.float32(rep["max_noise"]) == nmap.max()
    assert mon.last_measure_ms() > 0.0


# ---------------------------------------------------------------- the kernels alone (add_fbs)
@pytest.mark.parametrize("groups", [(1, 1, 1, 1, 1), (2, 3), (5,)], ids=["1x5", "2+3", "5"])
@pytest.mark.parametrize("W,H,mode", [
    (17, 9, "device"),   # per_fb = 459, odd: the one-by-one kernel
    (36, 9, "device"),   # per_fb = 972 = 4 x 243: the 16-byte kernel, 3 x 1 tiles with a partial edge tile
    (36, 9, "offset"),   # the same 4 bytes off: the one-by-one kernel again
    (40, 20, "host"),    # staged from host memory; 3 x 2 tiles, partial in both directions, 3 blocks
])
def test_add_fbs_moments_and_measure(rtlib, gpu_ctx, oracle, W, H, mode, groups):
    import torch

    nfb, n = sum(groups), W * H * 3
    fbs = nr.random_fbs(nfb, n, 7000 + n, special=True)
    assert np.isnan(fbs).any() and np.isinf(fbs).any()
    c = nr.quantise(oracle, fbs, W, H)
    gpu_ctx.upload(rtlib.Scene.builtin("basic"))
    args = rtlib.make_args(W, H, 1, 0, 1)
    off = 1 if mode == "offset" else 0
    dev = torch.zeros(nfb * n + off, dtype=torch.float32, device="cuda")
    dev[off:] = torch.from_numpy(fbs.reshape(-1)).cuda()
    base = dev.data_ptr() + 4 * off
    assert base % 16 == (4 if off else 0)
    acc, plain = gpu_ctx.accumulator(args), gpu_ctx.accumulator(args)
    try:
        mon = acc.noise_monitor()
        done = 0
        for g in groups:
            for a in (acc, plain):
                if mode == "host":
                    a.add_fbs(fbs[done:done + g].ctypes.data, g)
                else:
                    a.add_fbs(base + 4 * n * done, g)
            done += g
            # the monitor changes no pixel and no checkpoint byte
            assert np.array_equal(acc.image(), plain.image()), f"after {done}: image"
            assert acc.blob() == plain.blob(), f"after {done}: accumulator blob"
            assert acc.last_add_ms() > 0.0
            # integer moments: equal to the reference whatever the grouping
            blob = mon.blob()
            info = rtlib.rt_accum_info()
            assert rtlib.lib().rt_noise_blob_info(blob, len(blob), ctypes.byref(info)) == 0
            assert info.as_dict() == acc.info() and info.as_dict()["fb_count"] == done
            S1, S2 = nr.moments(c[:done])
            g1, g2 = nr.split_blob(blob, n)
            assert np.array_equal(g1, S1) and np.array_equal(g2, S2), f"after {done}: moments"
            if done >= 2:
                _check_measure(rtlib, mon, S1, S2, done, H, W, f"after {done}")
            else:
                assert _status(rtlib, lambda: mon.measure(1.0)) == RT_ERR_STATE
                assert _status(rtlib, mon.map) == RT_ERR_STATE
        # the map into device memory is the same map
        out = torch.zeros(H * W, dtype=torch.float32, device="cuda")
        mon.map_into(out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(H, W).view(np.uint32), mon.map().view(np.uint32))
    finally:
        acc.close()
        plain.close()


# ---------------------------------------------------------------- rendered frame buffers
W2, H2, SPP2, NFB2 = 40, 24, 2, 6
_renders = {}


def _rendered(rtlib, ctx, oracle, scene, cam):
    """(quantised frame buffers [NFB2][n] uint64, rt_draw's image) of scene at W2 x H2, rendered on the GPU."""
    import torch

    key = (scene, cam)
    if key not in _renders:
        ctx.upload(rtlib.Scene.builtin(scene))
        ctx.render_init(W2, H2, 1984)
        n = W2 * H2 * 3
        fb = torch.zeros(NFB2 * n, dtype=torch.float32, device="cuda")
        args = rtlib.make_args(W2, H2, SPP2, 0, NFB2, 50, cam)
        ctx.render(args, fb.data_ptr())
        fbs = fb.cpu().numpy().reshape(NFB2, n)
        img, _ = ctx.draw_args(args)
        _renders[key] = (nr.quantise(oracle, fbs, W2, H2), img)
    return _renders[key]


@pytest.mark.parametrize("chunk", [1, 4])
@pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "pix"])
@pytest.mark.parametrize("scene", ["first", "cornell_smoke"])
def test_rendered_moments(rtlib, gpu_ctx, oracle, scene, cam, chunk):
    c, one = _rendered(rtlib, gpu_ctx, oracle, scene, cam)
    gpu_ctx.upload(rtlib.Scene.builtin(scene))
    acc = gpu_ctx.accumulator(rtlib.make_args(W2, H2, SPP2, 0, 1, 50, cam), chunk_fbs=chunk)
    try:
        mon = acc.noise_monitor()
        acc.add(NFB2)  # chunk 4: launches of 4 and 2 frame buffers
        assert acc.done == NFB2
        assert np.array_equal(acc.image(png_order=True), one)
        S1, S2 = nr.moments(c)
        g1, g2 = nr.split_blob(mon.blob(), W2 * H2 * 3)
        assert np.array_equal(g1, S1) and np.array_equal(g2, S2)
        _check_measure(rtlib, mon, S1, S2, NFB2, H2, W2, f"{scene} chunk {chunk}")
    finally:
        acc.close()


def test_band_tiling_maps_interleave(rtlib, gpu_ctx):
    W, H, spp, nfb = 40, 26, 2, 3  # bands of 4 rows: share 0 owns 14 rows (the short last band), share 1 owns 12
    gpu_ctx.upload(rtlib.Scene.builtin("first"))
    whole_acc = gpu_ctx.accumulator(rtlib.make_args(W, H, spp, 0, 1), chunk_fbs=3)
    parts = [rtlib.make_args(W, H, spp, 0, 1, band_rows=4, band_first=b, band_stride=2) for b in (0, 1)]
    accs = [gpu_ctx.accumulator(a, chunk_fbs=2) for a in parts]
    try:
        whole_mon = whole_acc.noise_monitor()
        mons = [a.noise_monitor() for a in accs]
        for a in [whole_acc] + accs:
            a.add(nfb)
        whole = whole_mon.map()
        w1, w2 = nr.split_blob(whole_mon.blob(), W * H * 3)
        thr = nr.pick_threshold(whole)
        assert whole.shape == (H, W)
        seen = []
        for a, mon in zip(parts, mons):
            rows = rtlib.owned_rows(a)
            seen += list(rows)
            m = mon.map()
            assert m.shape == (len(rows), W)
            assert np.array_equal(m.view(np.uint32), whole[rows].view(np.uint32))  # exactly: the same integers
            s1, s2 = nr.split_blob(mon.blob(), len(rows) * W * 3)
            assert np.array_equal(s1, w1.reshape(H, W * 3)[rows].reshape(-1))
            assert np.array_equal(s2, w2.reshape(H, W * 3)[rows].reshape(-1))
            # tiles run over (position in the owned-row list, column)
            rep, tmax, tabove = mon.measure(thr)
            wmax, wabove = nr.tiles(whole[rows], thr)
            assert np.array_equal(tmax.view(np.uint32), wmax.view(np.uint32)) and np.array_equal(tabove, wabove)
            assert (rep["tiles_x"], rep["tiles_y"], rep["pixels"]) == (3, 1, len(rows) * W)
            assert rep["pixels_above"] == int((whole[rows] > np.float32(thr)).sum())
        assert sorted(seen) == list(range(H)) and [len(rtlib.owned_rows(a)) for a in parts] == [14, 12]
        rep = whole_mon.measure(thr)[0]
        assert (rep["tiles_x"], rep["tiles_y"]) == (3, 2) and rep["pixels_above"] == int((whole > np.float32(thr)).sum())
    finally:
        for a in [whole_acc] + accs:
            a.close()


# ---------------------------------------------------------------- side file and errors
def test_save_load_and_errors(rtlib, gpu_ctx, tmp_path):
    W, H, n = 36, 9, 36 * 9 * 3
    fbs = nr.random_fbs(6, n, 4242, special=True)
    p = fbs.ctypes.data
    gpu_ctx.upload(rtlib.Scene.builtin("basic"))
    args = rtlib.make_args(W, H, 1, 0, 1)
    side, ck = str(tmp_path / "ck.bin.noise"), str(tmp_path / "ck.bin")
    L = rtlib.lib()
    opened = []

    def new_acc():
        opened.append(gpu_ctx.accumulator(args))
        return opened[-1]

    try:
        a = new_acc()
        mon = a.noise_monitor()
        assert _status(rtlib, a.noise_monitor) == RT_ERR_STATE            # a second monitor
        # more than 32768 frame buffers: refused before anything is read, rendered or written
        assert _status(rtlib, lambda: a.add_fbs(p, nr.MAX_FBS + 1)) == RT_ERR_ARG
        assert _status(rtlib, lambda: a.add(nr.MAX_FBS + 1)) == RT_ERR_ARG
        assert a.done == 0
        a.add_fbs(p, 3)
        mon.save(side)
        a.save(ck)
        assert sorted(x.name for x in tmp_path.iterdir()) == ["ck.bin", "ck.bin.noise"]  # temporaries renamed away
        a.add_fbs(p + 4 * n * 3, 3)
        straight, straight_acc = mon.blob(), a.blob()

        b = new_acc()
        b.add_fbs(p, 1)
        assert _status(rtlib, b.noise_monitor) == RT_ERR_STATE            # create on a non-empty accumulator
        assert _status(rtlib, lambda: rtlib.NoiseMonitor.load(b, side)) == RT_ERR_STATE  # another fb_count
        assert _status(rtlib, lambda: rtlib.NoiseMonitor.load(a, side)) == RT_ERR_STATE  # 6 done, and a has one

        c = rtlib.Accumulator.load(gpu_ctx, ck)
        opened.append(c)
        bad = tmp_path / "bad.noise"
        bad.write_bytes(open(side, "rb").read()[:-4])
        assert _status(rtlib, lambda: rtlib.NoiseMonitor.load(c, str(bad))) == RT_ERR_ARG
        bad.write_bytes(open(ck, "rb").read())                            # an accumulator checkpoint is no side file
        assert _status(rtlib, lambda: rtlib.NoiseMonitor.load(c, str(bad))) == RT_ERR_ARG
        mc = rtlib.NoiseMonitor.load(c, side)
        assert _status(rtlib, lambda: rtlib.NoiseMonitor.load(c, side)) == RT_ERR_STATE  # c has a monitor now
        assert mc.blob() == open(side, "rb").read()
        c.add_fbs(p + 4 * n * 3, 3)
        assert mc.blob() == straight and c.blob() == straight_acc         # 3 + load + 3 == 6 straight
        rep, _, _, nmap = rtlib.read_noise(side, 1.0)
        assert rep["fb_count"] == 3 and nmap.shape == (H, W)

        # closing the monitor: the accumulator goes on without one
        mc.close()
        c.add_fbs(p, 1)
        assert c.done == 7

        # another scene, an accumulator in the same state otherwise
        gpu_ctx.upload(rtlib.Scene.builtin("first"))
        d = new_acc()
        d.add_fbs(p, 3)
        assert d.info()["scene_fp"] != a.info()["scene_fp"]
        assert _status(rtlib, lambda: rtlib.NoiseMonitor.load(d, side)) == RT_ERR_STATE

        # the accumulator destroyed first (C ABI): the monitor is detached, its calls fail, destroy frees it
        ha, hn = ctypes.c_void_p(), ctypes.c_void_p()
        assert L.rt_accum_create(gpu_ctx._c, ctypes.byref(args), 1, ctypes.byref(ha)) == 0
        assert L.rt_noise_create(ha, ctypes.byref(hn)) == 0
        assert L.rt_accum_add_fbs(ha, p, 2) == 0
        rep = rtlib.rt_noise_report()
        assert L.rt_noise_measure(hn, 1.0, ctypes.byref(rep), None, None) == 0 and rep.fbs == 2
        assert L.rt_accum_destroy(ha) == 0
        out = np.zeros((H, W), np.float32)
        need = ctypes.c_size_t()
        assert L.rt_noise_measure(hn, 1.0, ctypes.byref(rep), None, None) == RT_ERR_STATE
        assert L.rt_noise_map(hn, out.ctypes.data) == RT_ERR_STATE
        assert L.rt_noise_save(hn, None, 0, ctypes.byref(need)) == RT_ERR_STATE
        assert L.rt_noise_destroy(hn) == 0
    finally:
        for x in opened:
            x.close()


# ---------------------------------------------------------------- stop when converged
EVERY, NO_FB, FRACTION = 2, 12, 0.1
_manual = {}


def _manual_run(rtlib, ctx, scene, W, H, spp):
    """An accumulator and a monitor driven by hand over all NO_FB frame buffers, EVERY per step:
    {done: map}, {done: image}, the final monitor blob; then a threshold for which the stopping rule
    (pixels above <= floor(FRACTION x pixels)) first holds strictly between the first and the last step,
    and that step, from the maps alone."""
    key = (scene, W, H, spp)
    if key in _manual:
        return _manual[key]
    ctx.upload(rtlib.Scene.builtin(scene))
    acc = ctx.accumulator(rtlib.make_args(W, H, spp, 0, 1), chunk_fbs=EVERY)
    try:
        mon = acc.noise_monitor()
        maps, images = {}, {}
        while acc.done < NO_FB:
            acc.add(EVERY)
            maps[acc.done] = mon.map()
            images[acc.done] = acc.image(png_order=True)
        blob = mon.blob()
    finally:
        acc.close()
    limit = math.floor(FRACTION * W * H)
    # q[k]: the smallest threshold at which step k satisfies the rule (the (limit+1)-th largest value)
    q = {k: float(np.sort(m.reshape(-1))[::-1][limit]) for k, m in maps.items()}
    steps = sorted(maps)
    thr = stop = None
    for s in steps[1:-1]:
        lo, hi = q[s], min(q[k] for k in steps if k < s)
        if lo < hi:
            t = np.float32((lo + hi) / 2)
            every = np.concatenate([m.reshape(-1) for m in maps.values()])
            if lo < t < hi and np.abs(nr.ulps(every) - nr.ulps(t)).min() > 2:
                thr, stop = float(t), s
                break
    assert thr is not None, f"no threshold stops strictly inside the draw: {q}"
    above = {k: int((m > np.float32(thr)).sum()) for k, m in maps.items()}
    assert [k for k in steps if above[k] <= limit][0] == stop and steps[0] < stop < steps[-1]
    _manual[key] = (maps, images, blob, thr, stop, above)
    return _manual[key]


def test_draw_progressive_until_noise(rtlib, gpu_ctx, tmp_path):
    scene, W, H, spp = "first", 40, 24, 2
    maps, images, blob12, thr, stop, above = _manual_run(rtlib, gpu_ctx, scene, W, H, spp)
    s = rtlib.render_settings(image_width=W, image_height=H, samples_per_pixel_per_fb=spp, no_fb=NO_FB)
    ck = str(tmp_path / "draw.ck")
    noise_calls, image_calls = [], []

    def run(**kw):
        noise_calls.clear()
        image_calls.clear()
        return rtlib.draw_progressive(rtlib.Scene.builtin(scene), s, ctx=gpu_ctx, every=EVERY, checkpoint=ck,
                                      on_noise=lambda r, k: noise_calls.append((k, r)),
                                      on_image=lambda im, k: image_calls.append(k), **kw)

    img, cnt = run(until_noise=thr, noisy_fraction=FRACTION)
    steps = list(range(EVERY, stop + 1, EVERY))
    assert [k for k, _ in noise_calls] == steps == image_calls                 # the stop step
    assert [r["pixels_above"] for _, r in noise_calls] == [above[k] for k in steps]
    assert all(r["fbs"] == k and r["pixels"] == W * H for k, r in noise_calls)
    assert cnt["samples"] == W * H * spp * stop
    s_stop = rtlib.render_settings(image_width=W, image_height=H, samples_per_pixel_per_fb=spp, no_fb=stop)
    one, _ = rtlib.draw(rtlib.Scene.builtin(scene), s_stop, ctx=gpu_ctx)
    assert np.array_equal(img, one) and np.array_equal(img, images[stop])      # == draw(no_fb = stop)
    assert rtlib.read_checkpoint(ck)[0]["fb_count"] == stop
    assert rtlib.read_noise(ck + ".noise", thr)[0]["fb_count"] == stop
    assert sorted(x.name for x in tmp_path.iterdir()) == ["draw.ck", "draw.ck.noise"]
    stop_side = str(tmp_path / "stop.noise")
    shutil.copy(ck + ".noise", stop_side)
    # min_fbs postpones the first measure, and with it the stop
    limit = math.floor(FRACTION * W * H)
    late = next((k for k in sorted(above) if k > stop and above[k] <= limit), NO_FB)
    ck = str(tmp_path / "late.ck")
    img, _ = run(until_noise=thr, noisy_fraction=FRACTION, min_fbs=stop + 1)
    assert [k for k, _ in noise_calls] == list(range(stop + EVERY, late + 1, EVERY)) and image_calls[-1] == late
    assert np.array_equal(img, images[late])
    ck = str(tmp_path / "draw.ck")
    # resumed with the same rule: measured before anything is rendered, and still converged
    img, cnt = run(until_noise=thr, noisy_fraction=FRACTION)
    assert [k for k, _ in noise_calls] == [stop] and image_calls == [] and cnt["samples"] == 0
    assert np.array_equal(img, one)
    # resumed with a rule that never holds: the side file continues, to the same moments as 12 straight
    img, cnt = run(until_noise=0.0, noisy_fraction=0.0)
    assert [k for k, _ in noise_calls] == list(range(stop, NO_FB + 1, EVERY)) and cnt["samples"] == W * H * spp * (NO_FB - stop)
    assert np.array_equal(img, images[NO_FB])
    assert open(ck + ".noise", "rb").read() == blob12
    # without until_noise nothing changes: no monitor, no side file written, the same image
    ck3 = str(tmp_path / "plain.ck")
    plain, _ = rtlib.draw_progressive(rtlib.Scene.builtin(scene), s, ctx=gpu_ctx, every=EVERY, checkpoint=ck3)
    assert np.array_equal(plain, images[NO_FB]) and not os.path.exists(ck3 + ".noise")
    # a checkpoint without its side file, or with one of another frame-buffer count: no silent restart
    with pytest.raises(rtlib.RtError):
        rtlib.draw_progressive(rtlib.Scene.builtin(scene), s, ctx=gpu_ctx, every=EVERY, checkpoint=ck3, until_noise=thr)
    shutil.copy(stop_side, ck3 + ".noise")
    with pytest.raises(rtlib.RtError) as e:
        rtlib.draw_progressive(rtlib.Scene.builtin(scene), s, ctx=gpu_ctx, every=EVERY, checkpoint=ck3, until_noise=thr)
    assert e.value.status == RT_ERR_STATE


# ---------------------------------------------------------------- examples/rt_main
def _read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    W, H = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data[m.end():], np.uint8).reshape(H, W, 3)


def _rt_main(tmp_path, *args, ok=True):
    out = str(tmp_path / "out.ppm")
    p = subprocess.run([RT_MAIN, *map(str, args[:4]), out, *map(str, args[4:])], capture_output=True, text=True,
                       timeout=120)
    if not ok:
        return p
    assert p.returncode == 0, p.stderr
    return _read_ppm(out), [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]


def test_rt_main_until_noise(rtlib, gpu_ctx, tmp_path):
    assert os.path.exists(RT_MAIN), "examples/bin/rt_main not built (python -m raytracing_gpu_amd._build)"
    scene, W, spp = "first", 40, 2
    s = rtlib.render_settings(image_width=W)
    s.aspect_ratio = rtlib.Scene.builtin(scene).aspect
    s.calc_all()  # rt_main's own height
    H = s.image_height
    maps, images, blob12, thr, stop, above = _manual_run(rtlib, gpu_ctx, scene, W, H, spp)
    ck = str(tmp_path / "ck.bin")
    t = f"{np.float32(thr):.9g}"
    assert np.float32(float(t)) == np.float32(thr)
    img, lines = _rt_main(tmp_path, scene, W, spp, NO_FB, "--progressive", EVERY, "--until-noise", t,
                          "--noisy-fraction", FRACTION, "--checkpoint", ck)
    steps = list(range(EVERY, stop + 1, EVERY))
    per_step = [x for x in lines if "fbs_done" in x]
    assert [x["fbs_done"] for x in per_step] == steps
    assert [x["pixels_above"] for x in per_step] == [above[k] for k in steps]
    assert [np.float32(x["noise_max"]) for x in per_step] == [maps[k].max() for k in steps]
    assert "stopped_at" in lines[-1] and lines[-1]["stopped_at"] == stop and lines[-1]["converged"] is True
    assert img.shape == (H, W, 3) and np.array_equal(img, images[stop])
    assert sorted(x.name for x in tmp_path.iterdir()) == ["ck.bin", "ck.bin.noise", "out.ppm"]
    assert rtlib.read_noise(ck + ".noise", thr)[0]["fb_count"] == stop
    # resume with a rule that never holds: to NO_FB, the side file as 12 straight
    img, lines = _rt_main(tmp_path, scene, W, spp, NO_FB, "--progressive", EVERY, "--until-noise", 0,
                          "--noisy-fraction", 0, "--checkpoint", ck)
    assert [x["resumed_from"] for x in lines if "resumed_from" in x] == [stop]
    assert [x["fbs_done"] for x in lines if "fbs_done" in x] == list(range(stop + EVERY, NO_FB + 1, EVERY))
    assert lines[-1]["stopped_at"] == NO_FB and lines[-1]["converged"] is False
    assert np.array_equal(img, images[NO_FB]) and open(ck + ".noise", "rb").read() == blob12
    # the side file gone: refused; the option without --progressive: refused; without the option: no new keys
    os.remove(ck + ".noise")
    assert _rt_main(tmp_path, scene, W, spp, NO_FB, "--progressive", EVERY, "--until-noise", t, "--checkpoint", ck,
                    ok=False).returncode != 0
    assert _rt_main(tmp_path, scene, W, spp, NO_FB, "--until-noise", t, ok=False).returncode != 0
    img, lines = _rt_main(tmp_path, scene, W, spp, 4, "--progressive", EVERY)
    assert np.array_equal(img, images[4])
    assert not [x for x in lines if "noise_max" in x or "pixels_above" in x or "stopped_at" in x]
