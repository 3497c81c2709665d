"""Progressive accumulator, host side (no GPU): the rt_accum_* ABI is declared, exported and bound,
and the host-only checkpoint functions (csrc/rt_accum_blob.cpp) pack, validate and finalise a blob
byte-identically to the oracle's average_images for every prefix of a frame-buffer sequence."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rt_accum_create", "rt_accum_add", "rt_accum_add_fbs", "rt_accum_image", "rt_accum_get_info",
         "rt_accum_save", "rt_accum_load", "rt_accum_destroy", "rt_accum_blob_info", "rt_accum_blob_image",
         "rt_accum_blob_pack"]
W, H, NFB = 17, 9, 5
HEADER = 96
RT_ERR_ARG = 1


def test_accum_abi_declared_exported_bound(rtlib):
    hdr = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(rt_accum_\w+)\s*\(", hdr, re.M))
    assert declared == set(NAMES)
    L = rtlib.lib()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert not [n for n in NAMES if n not in rtlib.ABI]
    timers = set(re.findall(r"^\s*float\s+(rt_accum_\w+)\s*\(", hdr, re.M))
    assert timers == {"rt_accum_last_add_ms", "rt_accum_last_image_ms"}
    assert all(hasattr(L, n) and n in rtlib.ABI for n in timers)


def test_blob_file_has_no_hip_include():
    """The host-only functions link into a stand-alone program: no HIP header in their file."""
    src = open(os.path.join(ROOT, "raytracing_gpu_amd", "csrc", "rt_accum_blob.cpp")).read()
    assert "rt_accum_blob_info" in src and not re.search(r'#\s*include\s*[<"]hip', src)


def _info(rtlib, k, n_values=W * H * 3, **kw):
    a = rtlib.make_args(W, H, 3, 2, k, 50, rtlib.RT_CAM_PER_PIXEL, seed=77, **kw)
    return rtlib.rt_accum_info(a, n_values, 0x1234_5678_9ABC_DEF0)


def _pack(rtlib, info, sums):
    L = rtlib.lib()
    need = ctypes.c_size_t()
    assert L.rt_accum_blob_pack(ctypes.byref(info), None, None, 0, ctypes.byref(need)) == 0
    assert need.value == HEADER + 4 * sums.size
    buf = ctypes.create_string_buffer(need.value)
    assert L.rt_accum_blob_pack(ctypes.byref(info), sums.ctypes.data, buf, need.value, None) == 0
    return buf.raw


@pytest.fixture(scope="module")
def frames(oracle):
    """5 random frame buffers in [-0.3, 1.3] with exact zeros, their quantised PPM-order images and
    the float32 running sums after each (in the frame buffer's own bottom-up row order)."""
    rng = np.random.default_rng(20240607)
    fbs = rng.uniform(-0.3, 1.3, (NFB, H * W * 3)).astype(np.float32)
    fbs[rng.random(fbs.shape) < 0.05] = 0.0
    q = [oracle.quantize_fb(f, W, H) for f in fbs]  # PPM order: top row first
    sums, acc = [], np.zeros(H * W * 3, np.float32)
    for p in q:
        c = p.reshape(H, W * 3)[::-1].reshape(-1).astype(np.int32)  # back to bottom row first
        acc = acc + (c * c).astype(np.float32) / np.float32(255.0 * 255.0)
        assert acc.dtype == np.float32
        sums.append(acc.copy())
    return q, sums


def test_blob_round_trip_matches_oracle_average(rtlib, oracle, frames, tmp_path):
    q, sums = frames
    L = rtlib.lib()
    for k in range(1, NFB + 1):
        info = _info(rtlib, k)
        blob = _pack(rtlib, info, sums[k - 1])
        got = rtlib.rt_accum_info()
        assert L.rt_accum_blob_info(blob, len(blob), ctypes.byref(got)) == 0
        assert got.as_dict() == info.as_dict()
        assert got.as_dict()["fb_count"] == k and got.as_dict()["seed"] == 77 and got.as_dict()["fb_first"] == 2
        img = np.zeros((H, W, 3), np.uint8)
        assert L.rt_accum_blob_image(blob, len(blob), img.ctypes.data) == 0
        want = oracle.average(q[:k], W, H)  # PPM order
        assert np.array_equal(img[::-1], want), f"prefix {k}"
        path = tmp_path / f"ck{k}.bin"
        path.write_bytes(blob)
        d, im2 = rtlib.read_checkpoint(str(path))
        assert d == info.as_dict() and np.array_equal(im2, img)


def test_blob_header_layout(rtlib, frames):
    """The documented little-endian header, field by field."""
    _, sums = frames
    blob = _pack(rtlib, _info(rtlib, 4), sums[3])
    assert blob[:8] == b"RTACCUM1"
    assert struct.unpack_from("<II", blob, 8) == (1, HEADER)
    assert struct.unpack_from("<12i", blob, 16) == (W, H, 3, 2, 4, 50, 1, H, 0, 1, 0, 0)
    assert struct.unpack_from("<QqQ", blob, 64) == (77, W * H * 3, 0x1234_5678_9ABC_DEF0)
    h = 0xCBF29CE484222325
    for b in blob[HEADER:]:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    assert struct.unpack_from("<Q", blob, 88)[0] == h
    assert np.array_equal(np.frombuffer(blob, "<f4", offset=HEADER), sums[3])


def test_blob_partial_tiling(rtlib, frames):
    """n_values follows the band tiling: H = 9 in bands of 4, every second band from the first -> rows
    0-3 and 8."""
    _, sums = frames
    n = 5 * W * 3
    info = _info(rtlib, 2, n_values=n, band_rows=4, band_first=0, band_stride=2)
    blob = _pack(rtlib, info, sums[1][:n])
    got = rtlib.rt_accum_info()
    assert rtlib.lib().rt_accum_blob_info(blob, len(blob), ctypes.byref(got)) == 0
    assert got.as_dict() == info.as_dict()


def test_blob_rejection(rtlib, frames):
    _, sums = frames
    L = rtlib.lib()
    good = _pack(rtlib, _info(rtlib, 3), sums[2])
    info = rtlib.rt_accum_info()

    def rc(b):
        return L.rt_accum_blob_info(bytes(b), len(b), ctypes.byref(info))

    assert rc(good) == 0
    assert rc(good[:-1]) == RT_ERR_ARG and rc(good[:HEADER]) == RT_ERR_ARG and rc(good[:40]) == RT_ERR_ARG  # truncated
    assert rc(good + b"\0") == RT_ERR_ARG                                                      # too long
    assert rc(b"RTACCUM2" + good[8:]) == RT_ERR_ARG                                            # magic
    assert rc(good[:8] + struct.pack("<I", 2) + good[12:]) == RT_ERR_ARG                       # version
    flipped = bytearray(good)
    flipped[HEADER + 101] ^= 0x10
    assert rc(flipped) == RT_ERR_ARG                                                           # checksum
    # n_values that is not rows x width x 3 of the header's tiling (payload and file size agreeing
    # with the wrong value, checksum right: only the tiling check can refuse it)
    n = 5 * W * 3
    part = _pack(rtlib, _info(rtlib, 3, n_values=n, band_rows=4, band_first=0, band_stride=2), sums[2][:n])
    assert rc(part) == 0
    whole_tiling = bytearray(part)
    struct.pack_into("<3i", whole_tiling, 16 + 4 * 7, H, 0, 1)  # band_rows, band_first, band_stride
    assert rc(whole_tiling) == RT_ERR_ARG
    wrong_n = bytearray(good)
    struct.pack_into("<q", wrong_n, 72, W * H * 3 - 3)
    assert rc(wrong_n) == RT_ERR_ARG
    # the image function validates the same way, and pack refuses an info it could not read back
    img = np.zeros(W * H * 3, np.uint8)
    assert L.rt_accum_blob_image(bytes(flipped), len(flipped), img.ctypes.data) == RT_ERR_ARG
    bad = _info(rtlib, 3, n_values=W * H * 3 - 3)
    assert L.rt_accum_blob_pack(ctypes.byref(bad), sums[2].ctypes.data, ctypes.create_string_buffer(len(good)),
                                len(good), None) == RT_ERR_ARG
    small = ctypes.create_string_buffer(len(good) - 1)
    ok = _info(rtlib, 3)
    assert L.rt_accum_blob_pack(ctypes.byref(ok), sums[2].ctypes.data, small, len(good) - 1, None) == RT_ERR_ARG
