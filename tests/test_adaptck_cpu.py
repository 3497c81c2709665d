"""Checkpoint, reopen and dilation of the adaptive accumulator, host side (no GPU): the rt_adaptive_* ABI is
declared, exported and bound; the host-only blob tools of csrc/rt_adapt_blob.cpp equal the numpy model of
tests/adaptck_ref.py byte for byte and bit for bit on a hand-made state with three distinct n_t; malformed
blobs are refused; the model's dilation and reopen behave as include/rt_hip.h says; rt_main refuses the new
options without --adaptive."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import adaptck_ref as am
import noise_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_gpu_amd", "csrc")
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
RT_ERR_ARG, RT_ERR_STATE = 1, 3
DEVICE_NAMES = ["rt_adaptive_add", "rt_adaptive_retire", "rt_adaptive_reopen", "rt_adaptive_active", "rt_adaptive_save",
                "rt_adaptive_load"]
BLOB_NAMES = ["rt_adaptive_blob_info", "rt_adaptive_blob_tiles", "rt_adaptive_blob_image", "rt_adaptive_blob_measure",
              "rt_adaptive_blob_pack"]


def test_adaptive_abi_declared_exported_bound(rtlib):
    hdr = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert set(re.findall(r"^\s*int\s+(rt_adaptive_\w+)\s*\(", hdr, re.M)) == set(DEVICE_NAMES + BLOB_NAMES)
    L = rtlib.lib()
    for n in DEVICE_NAMES + BLOB_NAMES:
        assert hasattr(L, n) and n in rtlib.ABI, n
    for n in ("add", "retire", "reopen", "active", "blob", "save", "load"):
        assert callable(getattr(rtlib.AdaptiveAccumulator, n)), n
    assert callable(rtlib.read_adaptive_checkpoint)


def test_blob_source_is_host_only_and_built():
    from raytracing_gpu_amd import _build

    src = open(os.path.join(CSRC, "rt_adapt_blob.cpp")).read()
    assert not re.search(r'#\s*include\s*[<"]hip', src)
    assert "rt_adapt_blob.cpp" in _build.HIP_SOURCES and "rt_adapt_blob.cpp" in _build.HIP_DEPS


# ---------------------------------------------------------------- a hand-made state with three distinct n_t
ROWS, WIDTH, NFB = 20, 40, 8  # 2 x 3 tiles, partial in both directions
INFO = dict(width=WIDTH, height=ROWS, spp=3, fb_first=2, max_depth=50, cam_mode=1, band_rows=ROWS, band_first=0,
            band_stride=1, stats=0, flags=0, seed=77, scene_fp=0x123456789ABCDEF0)
AMPLITUDE = [2, 40, 10, 90, 4, 20]  # per tile: the spread of its planes around 128


def _planes():
    rng = np.random.default_rng(11)
    ty, tx = (ROWS + 15) // 16, (WIDTH + 15) // 16
    amp = np.repeat(np.repeat(np.array(AMPLITUDE).reshape(ty, tx), 16, 0), 16, 1)[:ROWS, :WIDTH]
    p = 128 + rng.integers(-1, 2, (NFB, ROWS, WIDTH, 3)) * amp[None, :, :, None]
    return p.astype(np.uint8).reshape(NFB, -1)


def _between(values, lo_count):
    """A threshold from am.midpoints with exactly lo_count of the distinct tile maxima below it."""
    v = np.unique(np.asarray(values, np.float32))
    for t in am.midpoints(v):
        if int((v < np.float32(t)).sum()) == lo_count:
            return t
    raise AssertionError("no such threshold")


_cache = {}


def _state():
    """(model, thresholds, reports): add 2, retire loosely (two tiles stop at 2), add 2, retire (two more stop
    at 4), add 2 (6), reopen tightly (every tile but the quietest), add 1 up to a limit of 6."""
    if not _cache:
        m = am.Model(_planes(), ROWS, WIDTH)
        reports = []
        m.add(2)
        t_loose = _between(m.tile_max(), 2)
        reports.append(m.retire(t_loose, 0))
        assert reports[-1]["tiles_active"] == 4
        m.add(2)
        t_mid = _between(m.tile_max().reshape(-1)[m.active], 2)
        reports.append(m.retire(t_mid, 0))
        assert reports[-1]["tiles_active"] == 2
        m.add(2)
        t_tight = _between(m.tile_max(), 1)
        reports.append(m.reopen(t_tight, 0))
        assert reports[-1]["tiles_active"] == 5
        before = m.counts().copy()
        m.add(1, limit=6)
        assert sorted(set(m.counts().reshape(-1).tolist())) == [2, 3, 5, 6]
        assert np.array_equal(m.counts() - before, (before < 6) & m.flags())  # from their own n_t, none beyond 6
        _cache["s"] = (m, (t_loose, t_mid, t_tight), reports)
    return _cache["s"]


def _c_info(rtlib, fb_count):
    args = rtlib.rt_render_args(*[dict(INFO, fb_count=fb_count)[k] for k in am.ARG_FIELDS], INFO["seed"])
    return rtlib.rt_accum_info(args, ROWS * WIDTH * 3, INFO["scene_fp"])


def _c_pack(rtlib, info, n_t, active, sums, S1, S2):
    """(status, blob) of rt_adaptive_blob_pack."""
    L = rtlib.lib()
    n_t = np.ascontiguousarray(n_t, np.int32)
    active = np.ascontiguousarray(active, np.uint8)
    sums = np.ascontiguousarray(sums, np.float32)
    s1, s2 = np.ascontiguousarray(S1, np.uint32), np.ascontiguousarray(S2, np.uint64)
    need = ctypes.c_size_t()
    rc = L.rt_adaptive_blob_pack(ctypes.byref(info), None, None, None, None, None, None, 0, ctypes.byref(need))
    if rc:
        return rc, b""
    buf = ctypes.create_string_buffer(need.value)
    rc = L.rt_adaptive_blob_pack(ctypes.byref(info), n_t.ctypes.data, active.ctypes.data, sums.ctypes.data, s1.ctypes.data,
                                 s2.ctypes.data, buf, need.value, None)
    return rc, buf.raw


def _blob_info(rtlib, blob):
    i = rtlib.rt_accum_info()
    return rtlib.lib().rt_adaptive_blob_info(bytes(blob), len(blob), ctypes.byref(i)), i


def test_both_writers_produce_the_same_bytes(rtlib):
    m, _, _ = _state()
    blob = m.pack(INFO)
    lay = am.layout(ROWS * WIDTH * 3, 6)
    assert len(blob) == lay["total"] == 128 + 16 * ROWS * WIDTH * 3 and lay["pad0"] == 126 and lay["sums"] == 128
    rc, cblob = _c_pack(rtlib, _c_info(rtlib, m.fbs), m.n_t, m.active, m.sums, m.S1, m.S2)
    assert rc == 0 and cblob == blob
    rc, i = _blob_info(rtlib, blob)
    assert rc == 0 and i.as_dict() == dict(INFO, fb_count=6, n_values=ROWS * WIDTH * 3)
    back = am.unpack(blob, ROWS * WIDTH * 3, 6)
    assert np.array_equal(back["n_t"], m.n_t) and np.array_equal(back["active"], m.active)
    assert np.array_equal(back["sums"].view(np.uint32), m.sums.reshape(-1).view(np.uint32))
    assert np.array_equal(back["S1"], m.S1.reshape(-1)) and np.array_equal(back["S2"], m.S2.reshape(-1))


def test_blob_tools_equal_the_model(rtlib, tmp_path):
    m, (_, _, t_tight), _ = _state()
    blob = m.pack(INFO)
    L = rtlib.lib()
    counts, flags = np.zeros((2, 3), np.int32), np.zeros((2, 3), np.uint8)
    assert L.rt_adaptive_blob_tiles(blob, len(blob), counts.ctypes.data, flags.ctypes.data) == 0
    assert np.array_equal(counts, m.counts()) and np.array_equal(flags.astype(bool), m.flags())
    img = np.zeros((ROWS, WIDTH, 3), np.uint8)
    assert L.rt_adaptive_blob_image(blob, len(blob), img.ctypes.data) == 0
    assert np.array_equal(img, m.image())
    # the measure: host double arithmetic is correctly rounded, so the map equals the model's bit for bit
    for T in (t_tight, 0.0):
        rep = rtlib.rt_adapt_report()
        tmax, tabove = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32)
        nmap = np.zeros((ROWS, WIDTH), np.float32)
        assert L.rt_adaptive_blob_measure(blob, len(blob), T, ctypes.byref(rep), tmax.ctypes.data, tabove.ctypes.data,
                                          nmap.ctypes.data) == 0
        want = m.noise()
        assert np.array_equal(nmap.view(np.uint32), want.view(np.uint32))
        wmax, wabove = nr.tiles(want, T)
        assert np.array_equal(tmax.view(np.uint32), wmax.view(np.uint32)) and np.array_equal(tabove, wabove)
        got, ref = rep.as_dict(), m.report(T)
        assert np.float32(got.pop("max_noise")) == np.float32(ref.pop("max_noise")) and got == ref
        assert L.rt_adaptive_blob_measure(blob, len(blob), T, None, None, None, None) == 0
    # the reader of the Python package
    path = str(tmp_path / "a.ckpt")
    open(path, "wb").write(blob)
    info, image, cnt, act = rtlib.read_adaptive_checkpoint(path)
    assert info["fb_count"] == 6 and np.array_equal(image, m.image()) and np.array_equal(cnt, m.counts())
    assert act.dtype == bool and np.array_equal(act, m.flags())
    full = rtlib.read_adaptive_checkpoint(path, threshold=t_tight)
    assert full[4]["pixels_above"] == m.report(t_tight)["pixels_above"]
    assert np.array_equal(full[5].view(np.uint32), m.noise().view(np.uint32))


# ---------------------------------------------------------------- malformed blobs
def test_check_adapt_blob_program_builds_and_passes(tmp_path):
    """scripts/check_adapt_blob.cpp: every truncation length, a flipped byte in each region and each
    violated invariant, in a stand-alone program (the one a sanitizer build runs)."""
    exe = tmp_path / "check_adapt_blob"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "scripts", "check_adapt_blob.cpp"), os.path.join(CSRC, "rt_adapt_blob.cpp"),
                    os.path.join(CSRC, "rt_accum_blob.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_adapt_blob ok" in r.stdout, r.stdout + r.stderr


def test_malformed_blobs_are_refused(rtlib):
    m, _, _ = _state()
    blob = m.pack(INFO)
    nv, tiles = ROWS * WIDTH * 3, 6
    lay = am.layout(nv, tiles)
    assert _blob_info(rtlib, blob)[0] == 0 and _blob_info(rtlib, am.rehash(blob))[0] == 0

    def put(at, data, fix=True):
        b = blob[:at] + data + blob[at + len(data):]
        return am.rehash(b) if fix else b

    i32 = lambda v: struct.pack("<i", v)  # noqa: E731
    retired = int(np.flatnonzero(~m.active)[0])
    at_max = np.flatnonzero(m.n_t == 6)
    lowered = blob
    for t in at_max:  # no tile at fb_count
        lowered = lowered[:lay["n_t"] + 4 * int(t)] + i32(5) + lowered[lay["n_t"] + 4 * int(t) + 4:]
    table = {
        "truncated": blob[:-1], "header only": blob[:96], "half a header": blob[:40], "empty": b"", "a byte more": blob + b"\0",
        "magic": put(0, b"RTNOISE1", False), "version": put(8, struct.pack("<I", 2), False),
        "header size": put(12, struct.pack("<I", 100), False), "hash": put(88, struct.pack("<Q", 1), False),
        "flipped sum": put(lay["sums"] + 9, bytes([blob[lay["sums"] + 9] ^ 1]), False),
        "flipped S2": put(lay["S2"] + 9, bytes([blob[lay["S2"] + 9] ^ 1]), False),
        "flipped S1": put(len(blob) - 1, bytes([blob[-1] ^ 1]), False),
        "n_values": put(72, struct.pack("<q", nv + 3), False), "width": put(16, i32(WIDTH + 16), False),
        "fb_count > 32768": put(32, i32(32769), False), "fb_count below a tile": put(32, i32(5), False),
        "fb_count above every tile": put(32, i32(7), False), "fb_count 0": put(32, i32(0), False),
        "n_t < 0": put(lay["n_t"], i32(-1)), "n_t > fb_count": put(lay["n_t"], i32(7)), "no tile at fb_count": am.rehash(lowered),
        "retired below 2": put(lay["n_t"] + 4 * retired, i32(1)), "flag 2": put(lay["active"], b"\2"),
        "padding": put(lay["pad0"], b"\1"), "padding, second byte": put(lay["pad0"] + 1, b"\x80"),
    }
    for name, b in table.items():
        assert _blob_info(rtlib, b)[0] == RT_ERR_ARG, name
        L = rtlib.lib()
        assert L.rt_adaptive_blob_tiles(b, len(b), None, None) == RT_ERR_ARG, name
        assert L.rt_adaptive_blob_measure(b, len(b), 1.0, None, None, None, None) == RT_ERR_ARG, name
    # an active tile may hold fewer than two frame buffers; it cannot be measured then
    active = int(np.flatnonzero(m.active & (m.n_t < 6))[0])
    odd = put(lay["n_t"] + 4 * active, i32(1))
    assert _blob_info(rtlib, odd)[0] == 0
    assert rtlib.lib().rt_adaptive_blob_measure(odd, len(odd), 1.0, None, None, None, None) == RT_ERR_STATE
    # pack refuses the same states
    assert _c_pack(rtlib, _c_info(rtlib, 7), m.n_t, m.active, m.sums, m.S1, m.S2)[0] == RT_ERR_ARG
    assert _c_pack(rtlib, _c_info(rtlib, 32769), m.n_t, m.active, m.sums, m.S1, m.S2)[0] == RT_ERR_ARG
    bad = m.n_t.copy()
    bad[retired] = 1
    assert _c_pack(rtlib, _c_info(rtlib, 6), bad, m.active, m.sums, m.S1, m.S2)[0] == RT_ERR_ARG
    # the empty state is valid, and has neither image nor measure
    z = np.zeros(nv)
    rc, empty = _c_pack(rtlib, _c_info(rtlib, 0), np.zeros(tiles), np.ones(tiles), z, z, z)
    assert rc == 0 and empty == am.pack(INFO, np.zeros(tiles, np.int64), np.ones(tiles, bool), z, z, z)
    assert _blob_info(rtlib, empty)[0] == 0
    img = np.zeros(nv, np.uint8)
    assert rtlib.lib().rt_adaptive_blob_image(empty, len(empty), img.ctypes.data) == RT_ERR_STATE
    assert _c_pack(rtlib, _c_info(rtlib, 0), np.zeros(tiles), m.active, z, z, z)[0] == RT_ERR_ARG


# ---------------------------------------------------------------- the model: dilation
def test_dilate_is_a_chebyshev_box():
    f = np.zeros((4, 5), bool)
    f[1, 3] = True
    assert np.array_equal(am.dilate(f, 0), f)
    one = am.dilate(f, 1)
    assert one.sum() == 9 and one[0:3, 2:5].all()
    two = am.dilate(f, 2)
    assert two.sum() == 16 and two[0:4, 1:5].all()  # clipped at the grid's edges
    assert am.dilate(f, 7).all() and not am.dilate(np.zeros((4, 5), bool), 3).any()


def _quiet_but_one(noisy_tile_px=(3, 17)):
    """Constant planes but one alternating pixel (tile 1)."""
    p = np.full((NFB, ROWS, WIDTH, 3), 100, np.uint8)
    p[0::2, noisy_tile_px[0], noisy_tile_px[1]] = 10
    p[1::2, noisy_tile_px[0], noisy_tile_px[1]] = 250
    return p.reshape(NFB, -1)


def test_model_passing_neighbour_stays_active_with_r1_and_retires_with_r0():
    flags = {}
    for r in (0, 1, 2):
        m = am.Model(_quiet_but_one(), ROWS, WIDTH)
        m.add(2)
        rep = m.retire(0.5, 0, r)
        flags[r] = m.flags()
        assert rep["tiles_active"] == int(flags[r].sum()) and rep["pixels_above"] == 1
    assert np.array_equal(flags[0], [[False, True, False], [False, False, False]])
    assert flags[1].all()  # every tile of the 2 x 3 grid is within 1 of tile 1, the partial edge tiles included
    assert flags[2].all()
    # a failing tile in a corner: r = 1 reaches the partial tiles beside it and no further
    m = am.Model(_quiet_but_one((18, 1)), ROWS, WIDTH)  # tile 3: 16 x 4 pixels
    m.add(2)
    m.retire(0.5, 0, 1)
    assert np.array_equal(m.flags(), [[True, True, False], [True, True, False]])
    m.add(2)
    assert np.array_equal(m.counts(), [[4, 4, 2], [4, 4, 2]])
    m.retire(0.5, 0, 2)  # the retired tiles are not brought back by a wider radius
    assert np.array_equal(m.flags(), [[True, True, False], [True, True, False]])


def test_model_everything_retires_when_no_active_tile_fails():
    m = am.Model(_quiet_but_one(), ROWS, WIDTH)
    m.add(2)
    rep = m.retire(1e9, 0, 2)
    assert rep["tiles_active"] == 0 and m.add(3) == 0 and (m.counts() == 2).all()


# ---------------------------------------------------------------- the model: reopen, limit
def test_model_reopen_retires_nothing_and_tiles_continue_from_their_own_count():
    m, (t_loose, t_mid, t_tight), reports = _state()
    assert t_tight < t_mid and t_tight < t_loose
    assert [r["tiles_active"] for r in reports] == [4, 2, 5] and [r["fbs"] for r in reports] == [2, 4, 6]
    # replayed: the flags before the reopen are a subset of those after it
    r = am.Model(_planes(), ROWS, WIDTH)
    r.add(2), r.retire(t_loose), r.add(2), r.retire(t_mid), r.add(2)
    before, counts = r.flags(), r.counts().copy()
    rep = r.reopen(t_tight)
    assert (r.flags() | ~before).all() and r.flags().sum() > before.sum() and np.array_equal(r.counts(), counts)
    assert rep["pixel_fbs"] == int((r.px * counts.reshape(-1)).sum())
    # a reopened tile at n_t = 2 receives planes 2, 3, ...: its sums equal a tile that never stopped
    work = r.add(2)
    assert work == int((r.px * (r.counts() - counts).reshape(-1)).sum())
    never = am.Model(_planes(), ROWS, WIDTH)
    never.add(4)
    sel = (r.n_t == 4)[r.tid] & (counts.reshape(-1) == 2)[r.tid]
    assert sel.any()
    assert np.array_equal(r.sums[sel].view(np.uint32), never.sums[sel].view(np.uint32))
    assert np.array_equal(r.S1[sel], never.S1[sel]) and np.array_equal(r.S2[sel], never.S2[sel])
    assert np.array_equal(r.image()[sel], never.image()[sel])


def test_model_limit_holds_and_tiles_at_it_stay_active():
    m = am.Model(_planes(), ROWS, WIDTH)
    assert m.add(5, limit=3) == 3 * ROWS * WIDTH and (m.counts() == 3).all()
    assert m.add(2, limit=3) == 0 and m.flags().all() and (m.counts() == 3).all()
    # the grouping of adds does not matter after a reopen either
    a, (t_loose, t_mid, t_tight), _ = _state()
    b = am.Model(_planes(), ROWS, WIDTH)
    b.add(1), b.add(1), b.retire(t_loose), b.add(2), b.retire(t_mid), b.add(1), b.add(1), b.reopen(t_tight), b.add(1, limit=6)
    assert b.pack(INFO) == a.pack(INFO)


# ---------------------------------------------------------------- rt_main's option checks (before any GPU call)
@pytest.mark.parametrize("extra", [["--adaptive-checkpoint", "c.bin"], ["--dilate", "1"], ["--reopen"]],
                         ids=["checkpoint", "dilate", "reopen"])
def test_rt_main_refuses_the_new_options_without_adaptive(rtlib, tmp_path, extra):
    from raytracing_gpu_amd import _build

    _build.build_examples()
    out = str(tmp_path / "o.ppm")
    r = subprocess.run([RT_MAIN, "big1", "70", "2", "8", out] + extra, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 99 and "need --adaptive" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "c.bin")
    r = subprocess.run([RT_MAIN, "big1", "70", "2", "8", out, "--adaptive", "2", "--until-noise", "1", "--dilate", "-1"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 99 and "--dilate" in r.stderr
