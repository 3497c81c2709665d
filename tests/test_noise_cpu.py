"""Noise monitor, host side (no GPU): the rt_noise_* ABI is declared, exported and bound, and the
host-only functions of csrc/rt_noise_blob.cpp pack, validate and measure a side file bit for bit like
the numpy reference of tests/noise_ref.py (host double division and sqrt are correctly rounded, as
numpy's are)."""
import ctypes
import math
import os
import re
import struct

import numpy as np
import pytest

import noise_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_noise_create", "rt_noise_measure", "rt_noise_map", "rt_noise_save", "rt_noise_load",
         "rt_noise_destroy", "rt_noise_blob_info", "rt_noise_blob_pack", "rt_noise_blob_measure"]
SHAPES = [(17, 9), (36, 9)]  # per_fb 459 (odd) and 972 (a multiple of 4); partial edge tiles
NFB = 5
HEADER = nr.HEADER
RT_ERR_ARG, RT_ERR_STATE = 1, 3
FP = 0x1234_5678_9ABC_DEF0


def test_noise_abi_declared_exported_bound(rtlib):
    hdr = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(rt_noise_\w+)\s*\(", hdr, re.M))
    assert declared == set(NAMES)
    assert set(re.findall(r"^\s*float\s+(rt_noise_\w+)\s*\(", hdr, re.M)) == {"rt_noise_last_measure_ms"}
    L = rtlib.lib()
    for n in NAMES + ["rt_noise_last_measure_ms"]:
        assert hasattr(L, n) and n in rtlib.ABI, n
    assert ctypes.sizeof(rtlib.rt_noise_report) == 40
    # the accumulator's own names are as they were
    assert not [n for n in rtlib.ABI if n.startswith("rt_accum_") and "noise" in n]


def test_noise_blob_file_has_no_hip_include_and_is_built():
    """The host-only functions link into a stand-alone program: no HIP header in their file."""
    from raytracing_gpu_amd import _build

    src = open(os.path.join(ROOT, "raytracing_gpu_amd", "csrc", "rt_noise_blob.cpp")).read()
    assert "rt_noise_blob_measure" in src and not re.search(r'#\s*include\s*[<"]hip', src)
    assert "rt_noise_blob.cpp" in _build.HIP_SOURCES


def _info(rtlib, W, H, k, n_values=None, **kw):
    a = rtlib.make_args(W, H, 3, 2, k, 50, rtlib.RT_CAM_PER_PIXEL, seed=77, **kw)
    return rtlib.rt_accum_info(a, W * H * 3 if n_values is None else n_values, FP)


@pytest.fixture(scope="module")
def quantised(oracle):
    """{(W, H): c [NFB][H*W*3] uint64}: random frame buffers in [-0.3, 1.3] with exact zeros, quantised
    by the oracle; pixel 3 of each is constant over the frame buffers."""
    out = {}
    for W, H in SHAPES:
        fbs = nr.random_fbs(NFB, W * H * 3, 20240607 + W)
        fbs[:, 9:12] = fbs[0, 9:12]
        fbs[:, 9] = 0.5  # not all three channels black
        out[(W, H)] = nr.quantise(oracle, fbs, W, H)
    return out


@pytest.mark.parametrize("W,H", SHAPES)
def test_blob_measure_matches_reference_bit_for_bit(rtlib, quantised, W, H):
    c = quantised[(W, H)]
    L = rtlib.lib()
    for k in range(2, NFB + 1):
        S1, S2 = nr.moments(c[:k])
        info = _info(rtlib, W, H, k)
        blob = nr.pack(rtlib, info, S1, S2)
        got = rtlib.rt_accum_info()
        assert L.rt_noise_blob_info(blob, len(blob), ctypes.byref(got)) == 0
        assert got.as_dict() == info.as_dict() and got.as_dict()["fb_count"] == k
        want = nr.noise_map(S1, S2, k, H, W)
        thr = nr.pick_threshold(want)
        rc, rep, tmax, tabove, nmap = nr.blob_measure(rtlib, blob, thr, H, W)
        assert rc == 0
        assert np.array_equal(nmap.view(np.uint32), want.view(np.uint32)), f"prefix {k}: map"
        wmax, wabove = nr.tiles(want, thr)
        assert np.array_equal(tmax.view(np.uint32), wmax.view(np.uint32)), f"prefix {k}: tile_max"
        assert np.array_equal(tabove, wabove), f"prefix {k}: tile_above"
        assert rep["pixels"] == W * H and rep["pixels_above"] == int((want > np.float32(thr)).sum()) == int(wabove.sum())
        assert 0 < rep["pixels_above"] < W * H
        assert np.float32(rep["max_noise"]).view(np.uint32) == want.max().view(np.uint32)
        assert (rep["fbs"], rep["tiles_x"], rep["tiles_y"]) == (k, (W + 15) // 16, 1)
        assert np.float32(rep["threshold"]) == np.float32(thr)
        # every output is optional
        assert L.rt_noise_blob_measure(blob, len(blob), thr, None, None, None, None) == 0


def test_one_frame_buffer_is_a_state_error(rtlib, quantised):
    W, H = SHAPES[0]
    S1, S2 = nr.moments(quantised[(W, H)][:1])
    blob = nr.pack(rtlib, _info(rtlib, W, H, 1), S1, S2)
    assert nr.blob_measure(rtlib, blob, 0.5, H, W)[0] == RT_ERR_STATE
    blob0 = nr.pack(rtlib, _info(rtlib, W, H, 0), S1 * 0, S2 * 0)
    assert nr.blob_measure(rtlib, blob0, 0.5, H, W)[0] == RT_ERR_STATE


def test_constant_pixel_has_no_noise(rtlib, quantised):
    W, H = SHAPES[0]
    c = quantised[(W, H)]
    same = np.flatnonzero((c == c[0]).all(0).reshape(H * W, 3).all(1))
    assert len(same) >= 1 and c[0].reshape(H * W, 3)[same[0]].max() > 0
    S1, S2 = nr.moments(c)
    rc, _, _, _, nmap = nr.blob_measure(rtlib, nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2), 0.5, H, W)
    assert rc == 0 and nmap.reshape(-1)[same[0]] == 0.0
    # an all-black pixel: m is clamped to 2^-16, the noise is 0 and not NaN
    S1[:3] = 0
    S2[:3] = 0
    rc, _, _, _, nmap = nr.blob_measure(rtlib, nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2), 0.5, H, W)
    assert rc == 0 and nmap.reshape(-1)[0] == 0.0 and np.isfinite(nmap).all()


def test_largest_monitor_does_not_overflow(rtlib):
    """n = 32768, half the frame buffers at c = 255 and half at 0: the largest D; against Python's
    unbounded integers.  One frame buffer more is refused."""
    W, H, n = 17, 1, nr.MAX_FBS
    half = n // 2
    s1, s2 = half * 65025, half * 65025 ** 2
    D = 3 * (n * s2 - s1 * s1)
    assert n * n * 65025 ** 2 < 4.6e18 < 2 ** 63 and 3 * n * n * 65025 ** 2 < 1.4e19 < 2 ** 64 and D < 2 ** 64
    S1 = np.full(W * H * 3, s1, np.uint64)
    S2 = np.full(W * H * 3, s2, np.uint64)
    # pixel 1: one channel only alternates, the others stay at 255 (largest n S2 and S1^2: D small)
    S1[3:6] = [s1, n * 65025, n * 65025]
    S2[3:6] = [s2, n * 65025 ** 2, n * 65025 ** 2]
    blob = nr.pack(rtlib, _info(rtlib, W, H, n), S1, S2)
    rc, rep, _, _, nmap = nr.blob_measure(rtlib, blob, 0.25, H, W)
    assert rc == 0

    def expect(D, S):
        a = float(D) / (3.0 * n * n * (n - 1) * 4228250625.0)
        m = float(S) / (3.0 * n * 65025.0)
        return np.float32(128.0 * math.sqrt(a / m))

    assert nmap[0, 0].view(np.uint32) == expect(D, 3 * s1).view(np.uint32)
    assert nmap[0, 1].view(np.uint32) == expect(D // 3, s1 + 2 * n * 65025).view(np.uint32)
    assert np.array_equal(nmap.view(np.uint32), nr.noise_map(S1, S2, n, H, W).view(np.uint32))
    # sd of x is 1/2, so the standard error of m = 1/2 is 0.5 / sqrt(n) and of the level 128 x that / sqrt(1/2)
    assert abs(float(nmap[0, 0]) - 128 * 0.5 / math.sqrt(n - 1) / math.sqrt(0.5)) < 1e-4
    assert rep["pixels_above"] == W - 1 and rep["fbs"] == n  # pixel 1 is at 0.2236
    # 32769 frame buffers: pack refuses, and so does a header that says so
    L = rtlib.lib()
    over = _info(rtlib, W, H, n + 1)
    buf = ctypes.create_string_buffer(len(blob))
    assert L.rt_noise_blob_pack(ctypes.byref(over), S1.astype(np.uint32).ctypes.data, S2.ctypes.data, buf, len(blob),
                                None) == RT_ERR_ARG
    forged = bytearray(blob)
    struct.pack_into("<i", forged, 16 + 4 * 4, n + 1)
    info = rtlib.rt_accum_info()
    assert L.rt_noise_blob_info(bytes(forged), len(forged), ctypes.byref(info)) == RT_ERR_ARG
    assert nr.blob_measure(rtlib, forged, 0.25, H, W)[0] == RT_ERR_ARG


def test_noise_blob_header_layout(rtlib, quantised):
    """The documented little-endian header, field by field, then S2 (u64) and S1 (u32)."""
    W, H = SHAPES[0]
    S1, S2 = nr.moments(quantised[(W, H)][:4])
    blob = nr.pack(rtlib, _info(rtlib, W, H, 4), S1, S2)
    n = W * H * 3
    assert len(blob) == HEADER + 12 * n
    assert blob[:8] == b"RTNOISE1"
    assert struct.unpack_from("<II", blob, 8) == (1, HEADER)
    assert struct.unpack_from("<12i", blob, 16) == (W, H, 3, 2, 4, 50, 1, H, 0, 1, 0, 0)
    assert struct.unpack_from("<QqQ", blob, 64) == (77, n, FP)
    h = 0xCBF29CE484222325
    for b in blob[HEADER:]:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    assert struct.unpack_from("<Q", blob, 88)[0] == h
    assert np.array_equal(np.frombuffer(blob, "<u8", n, HEADER), S2)
    assert np.array_equal(np.frombuffer(blob, "<u4", n, HEADER + 8 * n), S1)
    g1, g2 = nr.split_blob(blob, n)
    assert np.array_equal(g1, S1) and np.array_equal(g2, S2)


def test_noise_blob_rejection(rtlib, quantised):
    W, H = SHAPES[0]
    S1, S2 = nr.moments(quantised[(W, H)][:3])
    L = rtlib.lib()
    good = nr.pack(rtlib, _info(rtlib, W, H, 3), S1, S2)
    info = rtlib.rt_accum_info()

    def rc(b):
        return L.rt_noise_blob_info(bytes(b), len(b), ctypes.byref(info))

    assert rc(good) == 0
    assert rc(good[:-1]) == RT_ERR_ARG and rc(good[:HEADER]) == RT_ERR_ARG and rc(good[:40]) == RT_ERR_ARG  # truncated
    assert rc(good + b"\0") == RT_ERR_ARG                                                      # too long
    assert rc(b"RTNOISE2" + good[8:]) == RT_ERR_ARG and rc(b"RTACCUM1" + good[8:]) == RT_ERR_ARG  # magic
    assert rc(good[:8] + struct.pack("<I", 2) + good[12:]) == RT_ERR_ARG                       # version
    assert rc(good[:12] + struct.pack("<I", 100) + good[16:]) == RT_ERR_ARG                    # header size
    for off in (HEADER + 101, len(good) - 1):                                                  # checksum: S2, S1
        flipped = bytearray(good)
        flipped[off] ^= 0x10
        assert rc(flipped) == RT_ERR_ARG
    # n_values that is not rows x width x 3 of the header's tiling, payload and size agreeing with it
    n = 5 * W * 3
    part = nr.pack(rtlib, _info(rtlib, W, H, 3, n_values=n, band_rows=4, band_first=0, band_stride=2), S1[:n], S2[:n])
    assert rc(part) == 0 and info.n_values == n
    whole_tiling = bytearray(part)
    struct.pack_into("<3i", whole_tiling, 16 + 4 * 7, H, 0, 1)  # band_rows, band_first, band_stride
    assert rc(whole_tiling) == RT_ERR_ARG
    wrong_n = bytearray(good)
    struct.pack_into("<q", wrong_n, 72, W * H * 3 - 3)
    assert rc(wrong_n) == RT_ERR_ARG
    # header fields at 0, -1 and INT32_MAX (fields: width height spp fb_first fb_count max_depth cam_mode
    # band_rows band_first band_stride stats flags).  Still a valid header: any spp, max_depth > 0, any
    # fb_first >= 0, no frame buffer yet, the other camera mode, one band of any height >= H, band 0, any
    # stride with one band, and stats / flags, which nothing here reads.
    BIG = 2 ** 31 - 1
    valid = {(2, BIG), (3, 0), (3, BIG), (4, 0), (5, BIG), (6, 0), (7, BIG), (8, 0), (9, BIG)}
    valid |= {(f, v) for f in (10, 11) for v in (0, -1, BIG)}
    for field in range(12):
        for v in (0, -1, BIG):
            b = bytearray(good)
            struct.pack_into("<i", b, 16 + 4 * field, v)
            assert rc(b) == (0 if (field, v) in valid else RT_ERR_ARG), (field, v)
    for v in (0, -1, -3, 2 ** 63 - 1, 2 ** 62):
        b = bytearray(good)
        struct.pack_into("<q", b, 72, v)
        assert rc(b) == RT_ERR_ARG
    # the accumulator's functions do not take a monitor's blob, nor the monitor's an accumulator's
    assert L.rt_accum_blob_info(good, len(good), ctypes.byref(info)) == RT_ERR_ARG
    sums = np.zeros(W * H * 3, np.float32)
    ainfo = _info(rtlib, W, H, 3)
    need = ctypes.c_size_t()
    L.rt_accum_blob_pack(ctypes.byref(ainfo), None, None, 0, ctypes.byref(need))
    abuf = ctypes.create_string_buffer(need.value)
    assert L.rt_accum_blob_pack(ctypes.byref(ainfo), sums.ctypes.data, abuf, need.value, None) == 0
    assert rc(abuf.raw) == RT_ERR_ARG
    assert L.rt_accum_blob_info(b"RTACCUM2" + abuf.raw[8:], need.value, ctypes.byref(info)) == RT_ERR_ARG
    assert L.rt_accum_blob_info(abuf.raw[:8] + struct.pack("<I", 2) + abuf.raw[12:], need.value, ctypes.byref(info)) == RT_ERR_ARG
    # pack refuses an info it could not read back, and a small buffer
    bad = _info(rtlib, W, H, 3, n_values=W * H * 3 - 3)
    s1 = S1.astype(np.uint32)
    assert L.rt_noise_blob_pack(ctypes.byref(bad), s1.ctypes.data, S2.ctypes.data, ctypes.create_string_buffer(len(good)),
                                len(good), None) == RT_ERR_ARG
    ok = _info(rtlib, W, H, 3)
    assert L.rt_noise_blob_pack(ctypes.byref(ok), s1.ctypes.data, S2.ctypes.data, ctypes.create_string_buffer(len(good) - 1),
                                len(good) - 1, None) == RT_ERR_ARG


def test_read_noise(rtlib, quantised, tmp_path):
    W, H = SHAPES[1]
    S1, S2 = nr.moments(quantised[(W, H)])
    want = nr.noise_map(S1, S2, NFB, H, W)
    thr = nr.pick_threshold(want)
    path = tmp_path / "m.noise"
    path.write_bytes(nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2))
    rep, tmax, tabove, nmap = rtlib.read_noise(str(path), thr)
    assert np.array_equal(nmap.view(np.uint32), want.view(np.uint32))
    wmax, wabove = nr.tiles(want, thr)
    assert np.array_equal(tmax, wmax) and np.array_equal(tabove, wabove) and tmax.shape == (1, 3)
    assert rep["fb_count"] == rep["fbs"] == NFB and rep["pixels_above"] == int(wabove.sum()) and rep["scene_fp"] == FP
    path.write_bytes(path.read_bytes()[:-2])
    with pytest.raises(rtlib.RtError) as e:
        rtlib.read_noise(str(path), thr)
    assert e.value.status == RT_ERR_ARG
