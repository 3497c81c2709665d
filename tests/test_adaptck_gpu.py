"""Checkpoint and resume, reopening and dilation of the adaptive accumulator on the GPU (rt_adaptive_* of
include/rt_hip.h): a draw that is saved, destroyed and loaded continues byte-identically to one that never
stopped; reopened tiles continue from their own frame-buffer count and every tile stays the oracle's draw()
at that count; the device equals the numpy model of tests/adaptck_ref.py in every integer; the grouping of
adds, the chunk size and the limit change nothing they should not; the drivers resume.

Thresholds come from the model's own tile maxima over rt_render's planes: midpoints between adjacent
distinct values, with no reference noise value of any decision within 2 ulp of them (the device's double
divide and square root may differ from numpy's by an ulp, which then cannot move a decision)."""
import json
import os
import subprocess

import numpy as np
import pytest

import adapt_ref as ar
import adaptck_ref as am
import noise_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
REF, PIX = 0, 1
RT_ERR_ARG, RT_ERR_STATE = 1, 3
SPP, NFB = 2, 8
W, H = 70, 37  # 5 x 3 tiles, partial in both directions
BAND = dict(band_rows=4, band_stride=2, band_first=1)  # 17 of 37 rows: 5 x 2 tiles
CONFIGS = {"big1": ("big1", REF, None), "smoke_pix": ("cornell_smoke", PIX, None), "triangles": ("triangles", REF, None),
           "smoke_band": ("cornell_smoke", REF, BAND), "smoke": ("cornell_smoke", REF, None)}


def _status(rtlib, fn):
    with pytest.raises(rtlib.RtError) as e:
        fn()
    return e.value.status


def _args(rtlib, cam, band, first=0):
    return rtlib.make_args(W, H, SPP, first, 1, 50, cam, **(band or {}))


_planes, _plans, _oracle = {}, {}, {}


def _gpu_planes(rtlib, ctx, name):
    """[NFB][rows*W*3] uint8: the 8-bit plane of every single frame buffer, by plain rt_render + rt_resolve
    (the resolve of one frame buffer is c itself); computed once per configuration."""
    import torch

    if name not in _planes:
        scene, cam, band = CONFIGS[name]
        ctx.upload(rtlib.Scene.builtin(scene))
        ctx.render_init(W, H, 1984)
        out = []
        for f in range(NFB):
            args = _args(rtlib, cam, band, f)
            n = len(rtlib.owned_rows(args)) * W * 3
            fb = torch.zeros(n, dtype=torch.float32, device="cuda")
            img = torch.zeros(n, dtype=torch.uint8, device="cuda")
            ctx.render(args, fb.data_ptr())
            ctx.resolve(args, fb.data_ptr(), img.data_ptr())
            out.append(img.cpu().numpy())
        _planes[name] = np.stack(out)
    return _planes[name]


def _rows(rtlib, name):
    return len(rtlib.owned_rows(_args(rtlib, CONFIGS[name][1], CONFIGS[name][2])))


def _script(loose, tight, r=0):
    """The steps every test here is a part of: three rounds of add 2 / retire at the loose threshold, a
    reopen at the tight one, an add of 3 limited to 7 frame buffers, a last retire."""
    return [("add", 2, None), ("retire", loose, 0, r), ("add", 2, None), ("retire", loose, 0, r), ("add", 2, None),
            ("retire", loose, 0, r), ("reopen", tight, 0, r), ("add", 3, 7), ("retire", tight, 0, r)]


def _model_run(planes, rows, steps):
    """(model, reports, maps at every decision, active flags before and after the reopen)."""
    m = am.Model(planes, rows, W)
    reports, maps, around = [], [], []
    for s in steps:
        if s[0] == "add":
            m.add(s[1], s[2] if s[2] is not None else am.MAX_FBS)
        else:
            maps.append(m.noise())
            if s[0] == "reopen":
                around.append(m.flags())
            reports.append(getattr(m, s[0])(s[1], s[2], s[3]))
            if s[0] == "reopen":
                around.append(m.flags())
    return m, reports, maps, around


def _plan(rtlib, ctx, name):
    """(loose, tight): thresholds for _script, both midpoints between adjacent tile maxima of the model (loose:
    of a draw that retires nothing, at 2, 4 and 6 frame buffers, at most 17 of them evenly spread).
    loose: the one after whose three retires the model holds the most distinct retire times (two at least),
    then the most tiles still active; tight: the one below it whose reopen leaves the most distinct n_t at
    the end of the script (two at least), then reopens the most tiles (one at least).  No noise value of
    any decision lies within 2 ulp of either."""
    if name not in _plans:
        planes, rows = _gpu_planes(rtlib, ctx, name), _rows(rtlib, name)
        plain, maxima = am.Model(planes, rows, W), []
        for _ in range(3):  # the tile maxima of a draw that retires nothing, at 2, 4 and 6 frame buffers
            plain.add(2)
            maxima.append(plain.tile_max().reshape(-1))
        cands = am.midpoints(np.concatenate(maxima))
        best = None
        for loose in cands[::max(1, len(cands) // 16)]:
            before, maps = am.Model(planes, rows, W), []
            for s in _script(loose, loose)[:6]:
                if s[0] == "add":
                    before.add(s[1])
                else:
                    maps.append(before.noise())
                    before.retire(s[1], s[2])
            score = (len(set(before.n_t[~before.active].tolist())), int(before.active.sum()))
            if score[0] >= 2 and am.clear_of(loose, maps) and (best is None or score > best[0]):
                best = (score, loose, before)
        assert best, f"{name}: no threshold retires tiles at two distinct times"
        _, loose, before = best
        found = None
        for tight in [t for t in am.midpoints(before.tile_max()) if t < loose]:
            m, _, maps, around = _model_run(planes, rows, _script(loose, tight))
            score = (len(set(m.n_t.tolist())), int((around[1] & ~around[0]).sum()))
            if score[0] >= 2 and score[1] >= 1 and am.clear_of(tight, maps[3:]) and (found is None or score > found[0]):
                found = (score, tight)
        assert found, f"{name}: no tighter threshold reopens a tile"
        _plans[name] = (loose, found[1])
    return _plans[name]


def _run(ad, steps):
    """The reports and counters of the steps on an accumulator."""
    out = []
    for s in steps:
        if s[0] == "add":
            out.append(ad.add(s[1]) if s[2] is None else ad.add(s[1], limit=s[2]))
        else:
            out.append(getattr(ad, s[0])(s[1], s[2], s[3]))
    return out


def _state(ad):
    return ad.counts(), ad.active(), ad.image(), ad.noise_map().view(np.uint32)


def _same_report(got, want):
    for k in want:
        if k == "max_noise":
            assert abs(int(nr.ulps(np.float32(got[k]))) - int(nr.ulps(np.float32(want[k])))) <= 1, (got, want)
        else:
            assert got[k] == want[k], (k, got, want)


# ---------------------------------------------------------------- 1. resume equals never stopping
@pytest.mark.parametrize("name", ["big1", "smoke_pix", "triangles", "smoke_band"])
def test_resume_equals_never_stopping(rtlib, gpu_ctx, name):
    scene, cam, band = CONFIGS[name]
    loose, tight = _plan(rtlib, gpu_ctx, name)
    steps = _script(loose, tight, 1)
    gpu_ctx.upload(rtlib.Scene.builtin(scene))
    args = _args(rtlib, cam, band)
    whole = gpu_ctx.adaptive(args, chunk_fbs=2)
    try:
        empty = whole.blob()  # the empty state can be saved and loaded too
        want_out, want_blobs = [], []
        for s in steps:
            want_out += _run(whole, [s])
            want_blobs.append(whole.blob())
        want = _state(whole)
    finally:
        whole.close()
    part = rtlib.AdaptiveAccumulator.from_blob(gpu_ctx, empty, chunk_fbs=3)
    try:
        assert (part.counts() == 0).all() and part.active().all()
        for k, s in enumerate(steps):
            got = _run(part, [s])[0]
            assert got == want_out[k], (k, s, got, want_out[k])
            blob = part.blob()
            assert blob == want_blobs[k], f"{name}: the save after step {k} differs"
            part.close()  # destroyed, then continued from the bytes with another chunk size
            part = rtlib.AdaptiveAccumulator.from_blob(gpu_ctx, blob, chunk_fbs=1 + 2 * (k % 2))
        for g, w in zip(_state(part), want):
            assert np.array_equal(g, w)
        assert part.report(tight) == want_out[-1]
    finally:
        part.close()


# ---------------------------------------------------------------- 2. reopen against the model and the oracle
def _oracle_fbs(oracle, scene):
    if scene not in _oracle:
        ref = oracle.RefScene(scene)
        _oracle[scene] = [oracle.quantize_fb(ref.render(W, H, SPP, f, 50, REF)[0], W, H) for f in range(NFB)]
    return _oracle[scene]


@pytest.mark.parametrize("name", ["big1", "smoke", "triangles", "smoke_band"])
def test_reopen_equals_the_model_and_the_oracle(rtlib, gpu_ctx, oracle, name):
    scene, cam, band = CONFIGS[name]
    loose, tight = _plan(rtlib, gpu_ctx, name)
    steps = _script(loose, tight)
    rows = _rows(rtlib, name)
    model, want_reports, _, around = _model_run(_gpu_planes(rtlib, gpu_ctx, name), rows, steps)
    gpu_ctx.upload(rtlib.Scene.builtin(scene))
    ad = gpu_ctx.adaptive(_args(rtlib, cam, band), chunk_fbs=2)
    try:
        out = _run(ad, steps[:6])
        counts6, flags6 = ad.counts(), ad.active()
        assert len(set(counts6[~flags6].tolist())) >= 2, "the steps do not retire tiles at two distinct times"
        out += _run(ad, steps[6:7])
        assert np.array_equal(ad.counts(), counts6), "a reopen changes no count"
        reopened = ad.active() & ~flags6
        assert reopened.any() and (ad.active() | ~flags6).all(), "the steps reopen no tile, or the reopen retired one"
        assert np.array_equal(flags6, around[0]) and np.array_equal(ad.active(), around[1])
        counters = _run(ad, steps[7:8])[0]
        px = model.px.reshape(counts6.shape)
        grown = ad.counts() - counts6
        assert counters["samples"] == int((px * grown).sum()) * SPP
        assert (grown[reopened] > 0).all() and (ad.counts() <= 7).all()
        assert np.array_equal(grown, np.where(ad.active(), np.minimum(3, 7 - counts6), 0))
        out += [counters] + _run(ad, steps[8:])
        print(name, "thresholds", loose, tight, "counts", np.unique(ad.counts(), return_counts=True), "reopened", int(reopened.sum()))
        assert np.array_equal(ad.counts(), model.counts()) and np.array_equal(ad.active(), model.flags())
        assert np.array_equal(ad.image(), model.image())
        for got, ref in zip([o for o, s in zip(out, steps) if s[0] != "add"], want_reports):
            _same_report(got, ref)
        assert (np.abs(nr.ulps(ad.noise_map()) - nr.ulps(model.noise())) <= 1).all()
        if name in ("big1", "smoke"):  # the guarantee, with mixed n_t: every tile is the oracle's draw(no_fb = n_t)
            qs = _oracle_fbs(oracle, scene)
            img, counts = ad.image(png_order=True), ad.counts().reshape(-1)
            tid = ar.pixel_tiles(H, W)[::-1]  # tiles count rows from the bottom, the PNG-order image from the top
            assert len(set(counts.tolist())) >= 2
            for n in sorted(set(counts.tolist())):
                ref_img = oracle.average(qs[:n], W, H)
                sel = np.isin(tid, np.flatnonzero(counts == n))
                assert np.array_equal(img[sel], ref_img[sel]), f"{name}: tiles with n_t = {n} differ from the oracle's draw(no_fb={n})"
    finally:
        ad.close()


# ---------------------------------------------------------------- 3. grouping, 4. the limit
def _reopened_blob(rtlib, ctx, name):
    """The checkpoint after the reopen of _script (tiles at 2, 4 and 6 active together)."""
    scene, cam, band = CONFIGS[name]
    loose, tight = _plan(rtlib, ctx, name)
    ctx.upload(rtlib.Scene.builtin(scene))
    ad = ctx.adaptive(_args(rtlib, cam, band), chunk_fbs=2)
    try:
        _run(ad, _script(loose, tight)[:7])
        assert len(set(ad.counts()[ad.active()].tolist())) >= 2, "one group only: the test would show nothing"
        return ad.blob()
    finally:
        ad.close()


def test_grouping_of_adds_does_not_matter_after_a_reopen(rtlib, gpu_ctx):
    blob = _reopened_blob(rtlib, gpu_ctx, "big1")
    got = {}
    for how, chunk, adds in (("ones", 1, [1, 1, 1]), ("three", 1, [3]), ("three_chunk3", 3, [3]), ("two_one", 2, [2, 1])):
        ad = rtlib.AdaptiveAccumulator.from_blob(gpu_ctx, blob, chunk_fbs=chunk)
        try:
            total = {}
            for n in adds:
                for k, v in ad.add(n, limit=8).items():
                    total[k] = total.get(k, 0) + v
            got[how] = (ad.blob(), total["samples"], total["segments"])
        finally:
            ad.close()
    for how in got:
        assert got[how] == got["ones"], how


def test_limit_holds_and_tiles_at_it_stay_active(rtlib, gpu_ctx):
    blob = _reopened_blob(rtlib, gpu_ctx, "big1")
    ad = rtlib.AdaptiveAccumulator.from_blob(gpu_ctx, blob, chunk_fbs=2)
    try:
        before, flags = ad.counts(), ad.active()
        assert (before[flags] >= 5).any() and (before[flags] < 5).any()
        cnt = ad.add(4, limit=5)
        after = ad.counts()
        assert np.array_equal(after, np.where(flags & (before < 5), 5, before))  # none beyond it, none at it moved
        assert np.array_equal(ad.active(), flags)
        px = np.bincount(ar.pixel_tiles(H, W).reshape(-1)).reshape(before.shape)
        assert cnt["samples"] == int((px * (after - before)).sum()) * SPP > 0
        state = ad.blob()
        assert ad.add(4, limit=5) == {k: 0 for k in cnt}  # nobody receives anything
        assert ad.blob() == state and ad.report(1.0)["fbs"] == int(after.max())
    finally:
        ad.close()


# ---------------------------------------------------------------- 5. dilation
def _dilation_threshold(planes, rows):
    """A midpoint between adjacent tile maxima at 2 frame buffers under which the model's retire keeps the
    fewest tiles (one at least) with r = 0 and more with r = 1; no noise value within 2 ulp of it."""
    m = am.Model(planes, rows, W)
    m.add(2)
    best = None
    for T in am.midpoints(m.tile_max()):
        kept = []
        for r in (0, 1):
            k = am.Model(planes, rows, W)
            k.add(2)
            k.retire(T, 0, r)
            kept.append(int(k.active.sum()))
        if 0 < kept[0] < kept[1] and am.clear_of(T, [m.noise()]) and (best is None or kept[0] < best[0]):
            best = (kept[0], T)
    assert best, "no threshold at which a passing tile has a failing neighbour"
    return best[1]


@pytest.mark.parametrize("name", ["big1", "smoke_band"])
def test_dilation_on_the_device_equals_the_model(rtlib, gpu_ctx, name):
    import ctypes

    scene, cam, band = CONFIGS[name]
    planes, rows = _gpu_planes(rtlib, gpu_ctx, name), _rows(rtlib, name)
    loose = _dilation_threshold(planes, rows)
    gpu_ctx.upload(rtlib.Scene.builtin(scene))
    ad = gpu_ctx.adaptive(_args(rtlib, cam, band), chunk_fbs=2)
    try:
        ad.add(2)
        blob = ad.blob()
        rep = rtlib.rt_adapt_report()  # the entry point of old
        gpu_ctx._check(rtlib.lib().rt_adapt_retire(ad._h, loose, 0, ctypes.byref(rep)), "rt_adapt_retire")
        old = (rep.as_dict(), ad.active())
    finally:
        ad.close()
    flags = {}
    for r in (0, 1, 2):
        m = am.Model(planes, rows, W)
        m.add(2)
        want = m.retire(loose, 0, r)
        ad = rtlib.AdaptiveAccumulator.from_blob(gpu_ctx, blob, chunk_fbs=1)
        try:
            got = ad.retire(loose, 0, r)
            flags[r] = ad.active()
            _same_report(got, want)
            assert np.array_equal(flags[r], m.flags()), r
            if r == 0:
                assert got == old[0] and np.array_equal(flags[0], old[1])
        finally:
            ad.close()
    print(name, "threshold", loose, "active with r = 0, 1, 2:", [int(flags[r].sum()) for r in (0, 1, 2)])
    assert 0 < flags[0].sum() < flags[1].sum()  # the radius kept passing tiles
    assert (flags[1] | ~flags[0]).all() and (flags[2] | ~flags[1]).all()
    assert np.array_equal(flags[1], am.dilate(flags[0], 1)) and np.array_equal(flags[2], am.dilate(flags[0], 2))


# ---------------------------------------------------------------- 6. errors
def test_errors(rtlib, gpu_ctx):
    gpu_ctx.upload(rtlib.Scene.builtin("big1"))
    ad = gpu_ctx.adaptive(_args(rtlib, REF, None))
    try:
        ad.add(1)
        assert _status(rtlib, lambda: ad.reopen(1.0)) == RT_ERR_STATE  # needs two frame buffers
        assert _status(rtlib, lambda: ad.retire(1.0, 0, 1)) == RT_ERR_STATE
        ad.add(1)
        before = ad.blob()
        assert _status(rtlib, lambda: ad.retire(1.0, 0, -1)) == RT_ERR_ARG
        assert _status(rtlib, lambda: ad.reopen(1.0, 0, -1)) == RT_ERR_ARG
        assert _status(rtlib, lambda: ad.reopen(1.0, -1, 0)) == RT_ERR_ARG
        assert _status(rtlib, lambda: ad.add(1, limit=0)) == RT_ERR_ARG
        assert _status(rtlib, lambda: ad.add(0, limit=4)) == RT_ERR_ARG
        assert _status(rtlib, lambda: ad.add(nr.MAX_FBS, limit=nr.MAX_FBS + 5)) == RT_ERR_ARG  # would pass 32768
        assert ad.blob() == before  # nothing was rendered or retired
        for bad in (before[:-1], before[:200], before[:96] + bytes([before[96] ^ 1]) + before[97:], b"RTACCUM1" + before[8:]):
            assert _status(rtlib, lambda: rtlib.AdaptiveAccumulator.from_blob(gpu_ctx, bad)) == RT_ERR_ARG
        gpu_ctx.upload(rtlib.Scene.builtin("cornell_smoke"))
        assert _status(rtlib, lambda: rtlib.AdaptiveAccumulator.from_blob(gpu_ctx, before)) == RT_ERR_STATE
    finally:
        ad.close()


# ---------------------------------------------------------------- 7. the drivers
class _Stop(Exception):
    pass


def _settings(rtlib, no_fb=NFB):
    return rtlib.render_settings(image_width=W, image_height=H, samples_per_pixel_per_fb=SPP, no_fb=no_fb, max_depth=50)


def test_draw_adaptive_resumes_from_its_checkpoint(rtlib, gpu_ctx, tmp_path):
    loose, tight = _plan(rtlib, gpu_ctx, "big1")
    scene = rtlib.Scene.builtin("big1")
    kw = dict(ctx=gpu_ctx, every=2, until_noise=loose, max_above=0, min_fbs=2)
    want_img, want_total, want_counts = rtlib.draw_adaptive(scene, _settings(rtlib), **kw)
    assert len(set(want_counts.reshape(-1).tolist())) >= 2 and want_counts.max() > 4  # the draw goes on after the interruption
    path = str(tmp_path / "draw.ckpt")
    seen = []

    def stop_after_two(rep, done):
        seen.append(done)
        if len(seen) == 2:
            raise _Stop

    with pytest.raises(_Stop):
        rtlib.draw_adaptive(scene, _settings(rtlib), checkpoint=path, on_step=stop_after_two, **kw)
    info, _, counts, _ = rtlib.read_adaptive_checkpoint(path)
    assert seen == [2, 4] and info["fb_count"] == 4 and counts.max() == 4
    img, total, counts = rtlib.draw_adaptive(scene, _settings(rtlib), checkpoint=path, on_step=lambda rep, done: seen.append(done), **kw)
    assert np.array_equal(img, want_img) and np.array_equal(counts, want_counts)
    assert seen[2:] == list(range(6, int(want_counts.max()) + 1, 2)) and 0 < total["samples"] < want_total["samples"]
    _, ck_img, ck_counts, _ = rtlib.read_adaptive_checkpoint(path)
    assert np.array_equal(ck_img[::-1], img) and np.array_equal(ck_counts, counts)
    # a finished draw refined: reopen at the tighter threshold, every tile continuing from its own count
    img2, total2, counts2 = rtlib.draw_adaptive(scene, _settings(rtlib), checkpoint=path, reopen=True,
                                                **dict(kw, until_noise=tight, dilate=1))
    assert (counts2 >= counts).all() and (counts2 > counts).any() and counts2.max() <= NFB
    px = np.bincount(ar.pixel_tiles(H, W).reshape(-1)).reshape(counts.shape)
    assert total2["samples"] == int((px * (counts2 - counts)).sum()) * SPP
    # other settings, or more frame buffers than the draw may have
    assert _status(rtlib, lambda: rtlib.draw_adaptive(scene, _settings(rtlib, 2), checkpoint=path, **kw)) is None
    with pytest.raises(rtlib.RtError):
        rtlib.draw_adaptive(scene, _settings(rtlib), checkpoint=path, **dict(kw, cam_mode=PIX))
    assert _status(rtlib, lambda: rtlib.draw_adaptive(rtlib.Scene.builtin("cornell_smoke"), _settings(rtlib), checkpoint=path,
                                                     **kw)) == RT_ERR_STATE


def test_rt_main_adaptive_checkpoint_run_twice(rtlib, gpu_ctx, tmp_path):
    loose, tight = _plan(rtlib, gpu_ctx, "big1")
    out, ckpt = str(tmp_path / "a.ppm"), str(tmp_path / "a.ckpt")

    def main(no_fb, T, *extra):
        r = subprocess.run([RT_MAIN, "big1", str(W), str(SPP), str(no_fb), out, "--height", str(H), "--adaptive", "2",
                            "--until-noise", repr(float(T)), "--min-fbs", "2", "--adaptive-checkpoint", ckpt,
                            *extra], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [json.loads(x) for x in r.stdout.splitlines()]

    first = main(4, loose)
    assert "resumed_from" not in first[0] and first[-1]["stopped_at"] == 4
    second = main(NFB, loose)
    assert second[0] == {"resumed_from": 4, "checkpoint": ckpt}
    img, _, counts = rtlib.draw_adaptive(rtlib.Scene.builtin("big1"), _settings(rtlib), ctx=gpu_ctx, every=2, until_noise=loose,
                                         max_above=0, min_fbs=2)
    data = open(out, "rb").read()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(head) and data[len(head):] == img.tobytes()
    assert second[-1]["stopped_at"] == int(counts.max())
    assert np.array_equal(rtlib.read_adaptive_checkpoint(ckpt)[2], counts)
    third = main(NFB, tight, "--reopen", "--dilate", "1")
    assert third[0]["resumed_from"] == int(counts.max()) and third[1]["reopened"] > 0
    assert (rtlib.read_adaptive_checkpoint(ckpt)[2] >= counts).all()
