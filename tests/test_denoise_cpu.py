"""Denoiser, host side (no GPU): the rt_denoise_* ABI is declared, exported and bound, and the host-only twin
of csrc/rt_denoise_blob.cpp equals the numpy definition of tests/denoise_ref.py byte for byte -- the image and
the gain as float bits -- on a monitor's side file and on an adaptive checkpoint; the properties the
definition implies; the argument table."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_ref as dr
import noise_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing_gpu_amd", "csrc")
INT_NAMES = ["rt_denoise_monitor", "rt_denoise_adaptive", "rt_denoise_monitor_blob", "rt_denoise_adaptive_blob"]
FLOAT_NAMES = ["rt_denoise_monitor_last_ms", "rt_denoise_adaptive_last_ms"]
RT_ERR_ARG, RT_ERR_STATE = 1, 3
FP = 0x0FED_CBA9_8765_4321
NFB = 5
PAPER = dict(search_radius=10, patch_radius=3, k=0.45, alpha=1.0, eps=1.0)


def test_denoise_abi_declared_exported_bound(rtlib):
    hdr = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert set(re.findall(r"^\s*int\s+(rt_denoise_\w+)\s*\(", hdr, re.M)) == set(INT_NAMES)
    assert set(re.findall(r"^\s*float\s+(rt_denoise_\w+)\s*\(", hdr, re.M)) == set(FLOAT_NAMES)
    assert re.findall(r"^\s*void\s+(rt_denoise_\w+)\s*\(", hdr, re.M) == ["rt_denoise_params_default"]
    L = rtlib.lib()
    for n in INT_NAMES + FLOAT_NAMES + ["rt_denoise_params_default"]:
        assert hasattr(L, n) and n in rtlib.ABI, n
    assert ctypes.sizeof(rtlib.rt_denoise_params) == 24
    d = rtlib.denoise_params().as_dict()
    assert 0 <= d["search_radius"] <= 10 and 0 <= d["patch_radius"] <= 3 and d["k"] > 0 and d["alpha"] >= 0 and d["eps"] > 0
    assert "No float is summed across pixels" in hdr


def test_denoise_sources_share_one_arithmetic_and_are_built():
    """The twin is host only (no HIP header), both halves compile rt_denoise_math.h, and both are built."""
    from raytracing_gpu_amd import _build

    twin = open(os.path.join(CSRC, "rt_denoise_blob.cpp")).read()
    dev = open(os.path.join(CSRC, "rt_denoise.hip")).read()
    assert not re.search(r'#\s*include\s*[<"]hip', twin)
    for src in (twin, dev):
        assert '#include "rt_denoise_math.h"' in src and "rtdn::term(" in src and "rtdn::weight(" in src
    assert "rt_denoise_blob.cpp" in _build.HIP_SOURCES and "rt_denoise.hip" in _build.HIP_SOURCES


def test_check_denoise_blob_program_builds_and_passes(tmp_path):
    """scripts/check_denoise_blob.cpp: the twin on images smaller than its window, patch and tile, with every
    refusal, in a stand-alone program (the one a sanitizer build runs)."""
    import subprocess

    exe = tmp_path / "check_denoise_blob"
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "scripts", "check_denoise_blob.cpp"),
                    *[os.path.join(CSRC, f"rt_{x}_blob.cpp") for x in ("accum", "noise", "adapt", "denoise")], "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_denoise_blob ok" in r.stdout, r.stdout + r.stderr


def _info(rtlib, W, H, k, **kw):
    a = rtlib.make_args(W, H, 3, 2, k, 50, rtlib.RT_CAM_PER_PIXEL, seed=77, **kw)
    return rtlib.rt_accum_info(a, W * H * 3, FP)


def _twin(rtlib, fn, blob, params, W, H, want_gain=True):
    """(status, image, gain) of a host-only denoise; the outputs start as sentinels."""
    img = np.full((H, W, 3), 0xAB, np.uint8)
    gain = np.full((H, W), -7.0, np.float32)
    p = rtlib.denoise_params(params) if params is not None else None
    rc = fn(bytes(blob), len(blob), ctypes.byref(p) if p is not None else None, img.ctypes.data,
            gain.ctypes.data if want_gain else None)
    return rc, img, gain


def _untouched(img, gain):
    return bool((img == 0xAB).all() and (gain == np.float32(-7.0)).all())


def _same(img, gain, want_img, want_gain):
    assert np.array_equal(img, want_img), f"image: {int((img != want_img).sum())} bytes differ"
    assert np.array_equal(gain.view(np.uint32), want_gain.view(np.uint32)), "gain bits"


@pytest.fixture(scope="module")
def quantised(oracle):
    """{(W, H): c [NFB][H*W*3] uint64} of random frame buffers with zeros, NaN and infinities."""
    out = {}
    for W, H in [(23, 19), (40, 37), (5, 3), (1, 1)]:
        out[(W, H)] = nr.quantise(oracle, nr.random_fbs(NFB, W * H * 3, 20241020 + W, special=True), W, H)
    return out


@pytest.mark.parametrize("W,H,R,f", [(23, 19, 3, 1), (40, 37, 10, 3), (5, 3, 10, 3), (1, 1, 10, 3), (1, 1, 0, 0)])
def test_monitor_twin_equals_the_definition(rtlib, quantised, W, H, R, f):
    S1, S2 = nr.moments(quantised[(W, H)])
    blob = nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2)
    prm = dict(PAPER, search_radius=R, patch_radius=f)
    rc, img, gain = _twin(rtlib, rtlib.lib().rt_denoise_monitor_blob, blob, prm, W, H)
    assert rc == 0
    want_img, want_gain = dr.denoise(S1, S2, NFB, H, W, R, f, prm["k"], prm["alpha"], prm["eps"])
    _same(img, gain, want_img, want_gain)
    assert (gain >= 1.0).all() and (gain <= dr.window_pixels(H, W, R)).all()
    if (W, H) == (40, 37):
        assert gain.max() > 1.0 and len(np.unique(gain)) > 100  # the weights are neither all 0 nor all 1
    # gain is optional, and other parameters give another image
    rc, img2, g2 = _twin(rtlib, rtlib.lib().rt_denoise_monitor_blob, blob, prm, W, H, want_gain=False)
    assert rc == 0 and np.array_equal(img2, img) and (g2 == np.float32(-7.0)).all()


@pytest.mark.parametrize("k,alpha,eps", [(0.2, 0.0, 1e-3), (3.0, 4.0, 100.0), (float("inf"), float("inf"), 1.0)])
def test_monitor_twin_other_parameters(rtlib, quantised, k, alpha, eps):
    """Small and large parameters, and the infinite ones whose NaN terms the definition takes as -64."""
    W, H = 23, 19
    c = quantised[(W, H)].copy()
    c[:, :30] = c[0, :30]  # some values of zero variance
    S1, S2 = nr.moments(c)
    blob = nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2)
    prm = dict(search_radius=4, patch_radius=2, k=k, alpha=alpha, eps=eps)
    rc, img, gain = _twin(rtlib, rtlib.lib().rt_denoise_monitor_blob, blob, prm, W, H)
    assert rc == 0
    _same(img, gain, *dr.denoise(S1, S2, NFB, H, W, 4, 2, k, alpha, eps))


@pytest.mark.parametrize("n", [2, nr.MAX_FBS])
def test_integer_bounds_with_saturated_values(rtlib, n):
    """Every frame buffer at c = 0 or c = 255: the largest S1, S2, D and Q; against numpy's checked bounds."""
    W, H = 9, 7
    rng = np.random.default_rng(n)
    m = rng.integers(0, n + 1, W * H * 3).astype(np.uint64)  # frame buffers at 255
    m[:6] = [0, n, n // 2, n, 0, 1]
    S1, S2 = m * np.uint64(65025), m * np.uint64(65025 ** 2)
    assert int(S1.max()) < 2 ** 32 and n * int(S2.max()) < 2 ** 63
    blob = nr.pack(rtlib, _info(rtlib, W, H, n), S1, S2)
    for R, f in [(3, 1), (10, 3)]:
        prm = dict(PAPER, search_radius=R, patch_radius=f)
        rc, img, gain = _twin(rtlib, rtlib.lib().rt_denoise_monitor_blob, blob, prm, W, H)
        assert rc == 0
        _same(img, gain, *dr.denoise(S1, S2, n, H, W, R, f, prm["k"], prm["alpha"], prm["eps"]))


def _adaptive_blob(rtlib, W, H, n_t, S1, S2):
    L = rtlib.lib()
    info = _info(rtlib, W, H, int(np.max(n_t)))
    n_t = np.ascontiguousarray(n_t, np.int32)
    active = np.zeros(n_t.size, np.uint8)
    sums = np.zeros(W * H * 3, np.float32)
    s1, s2 = np.ascontiguousarray(S1, np.uint32), np.ascontiguousarray(S2, np.uint64)
    need = ctypes.c_size_t()
    assert L.rt_adaptive_blob_pack(ctypes.byref(info), None, None, None, None, None, None, 0, ctypes.byref(need)) == 0
    buf = ctypes.create_string_buffer(need.value)
    assert L.rt_adaptive_blob_pack(ctypes.byref(info), n_t.ctypes.data, active.ctypes.data, sums.ctypes.data, s1.ctypes.data,
                                   s2.ctypes.data, buf, need.value, None) == 0
    return buf.raw


def _mixed_counts(oracle, W, H, counts):
    """(n_t [tiles], n per pixel [H][W], S1, S2): tile t has folded in the first counts[t] of 9 frame buffers."""
    c = nr.quantise(oracle, nr.random_fbs(9, W * H * 3, 424242, special=True), W, H).reshape(9, H, W, 3)
    ty, tx = (H + 15) // 16, (W + 15) // 16
    n_t = np.array(counts, np.int64).reshape(ty, tx)
    n_px = np.repeat(np.repeat(n_t, 16, 0), 16, 1)[:H, :W]
    c2 = c * c
    live = (np.arange(9)[:, None, None] < n_px[None])[..., None]
    S1 = (c2 * live).sum(0, dtype=np.uint64)
    S2 = (c2 * c2 * live).sum(0, dtype=np.uint64)
    return n_t.reshape(-1), n_px, S1.reshape(-1), S2.reshape(-1)


def test_adaptive_twin_equals_the_definition(rtlib, oracle):
    W, H = 40, 37
    n_t, n_px, S1, S2 = _mixed_counts(oracle, W, H, [2, 5, 9, 9, 2, 5, 5, 9, 2])
    blob = _adaptive_blob(rtlib, W, H, n_t, S1, S2)
    fn = rtlib.lib().rt_denoise_adaptive_blob
    for R, f in [(10, 3), (2, 1)]:
        prm = dict(PAPER, search_radius=R, patch_radius=f)
        rc, img, gain = _twin(rtlib, fn, blob, prm, W, H)
        assert rc == 0
        _same(img, gain, *dr.denoise(S1, S2, n_px, H, W, R, f, prm["k"], prm["alpha"], prm["eps"]))
    # the counts matter: the same moments read as 9 frame buffers everywhere give another result
    other = dr.denoise(S1, S2, 9, H, W, 2, 1, PAPER["k"], PAPER["alpha"], PAPER["eps"])
    assert not np.array_equal(other[1].view(np.uint32), gain.view(np.uint32))
    # a tile below two frame buffers: RT_ERR_STATE, nothing written
    low = n_t.copy()
    low[4] = 1
    S1b, S2b = S1.copy(), S2.copy()
    L = rtlib.lib()
    info = _info(rtlib, W, H, 9)
    act = np.ones(9, np.uint8)  # a tile below 2 must be active
    need = ctypes.c_size_t()
    L.rt_adaptive_blob_pack(ctypes.byref(info), None, None, None, None, None, None, 0, ctypes.byref(need))
    buf = ctypes.create_string_buffer(need.value)
    assert L.rt_adaptive_blob_pack(ctypes.byref(info), np.ascontiguousarray(low, np.int32).ctypes.data, act.ctypes.data,
                                   np.zeros(W * H * 3, np.float32).ctypes.data, S1b.astype(np.uint32).ctypes.data,
                                   S2b.ctypes.data, buf, need.value, None) == 0
    rc, img, gain = _twin(rtlib, fn, buf.raw, PAPER, W, H)
    assert rc == RT_ERR_STATE and _untouched(img, gain)


def _flat(values, W, H, n):
    """Moments of n identical frame buffers whose pixel (y, x) is at c = values[y][x] in every channel."""
    c = np.repeat(np.asarray(values, np.uint64).reshape(H, W, 1), 3, 2).reshape(-1)
    return np.uint64(n) * c * c, np.uint64(n) * c ** np.uint64(4)


def _plain(S1, n, W, H):
    """quant(sum / n) of the accumulator for frame buffers that all agree: c itself, below the 0.999 clamp."""
    return dr.quant((S1.astype(np.float32) / np.float32(n)) / np.float32(255.0 * 255.0)).reshape(H, W, 3)


def test_constant_image_is_kept_and_gain_counts_the_window(rtlib):
    W, H, n = 29, 18, 4
    S1, S2 = _flat(np.full((H, W), 180), W, H, n)
    blob = nr.pack(rtlib, _info(rtlib, W, H, n), S1, S2)
    for R, f in [(10, 3), (4, 0)]:
        rc, img, gain = _twin(rtlib, rtlib.lib().rt_denoise_monitor_blob, blob, dict(PAPER, search_radius=R, patch_radius=f), W, H)
        assert rc == 0
        assert np.array_equal(img, _plain(S1, n, W, H)) and (img == 180).all()
        assert np.array_equal(gain, dr.window_pixels(H, W, R))


def test_radius_zero_gives_gain_one(rtlib, quantised):
    W, H = 23, 19
    S1, S2 = nr.moments(quantised[(W, H)])
    blob = nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2)
    rc, img, gain = _twin(rtlib, rtlib.lib().rt_denoise_monitor_blob, blob, dict(PAPER, search_radius=0), W, H)
    assert rc == 0 and (gain == 1.0).all()
    # ... and the image is the mean of c^2 itself: quant(Q / (256 x 65025))
    Q = dr.prepare(S1.reshape(H, W, 3), S2.reshape(H, W, 3), NFB)[0]
    assert np.array_equal(img, dr.quant((Q.astype(np.float64) / (1.0 * 256.0 * 65025.0)).astype(np.float32)))


def test_two_flat_halves_do_not_mix(rtlib):
    """Left half at 60, right half at 200, no variance: a weight is 0 as soon as a patch pair straddles the edge,
    so the image is unchanged and the gain counts pixels of the pixel's own side only: all of the window's with
    single-pixel patches, no more than those with larger ones."""
    W, H, n, R = 30, 12, 3, 5
    v = np.full((H, W), 60)
    v[:, W // 2:] = 200
    S1, S2 = _flat(v, W, H, n)
    blob = nr.pack(rtlib, _info(rtlib, W, H, n), S1, S2)
    cy = np.array([min(H - 1, y + R) - max(0, y - R) + 1 for y in range(H)])
    side = np.array([(min(W // 2 - 1, x + R) - max(0, x - R) + 1) if x < W // 2 else
                     (min(W - 1, x + R) - max(W // 2, x - R) + 1) for x in range(W)])
    same_side = (cy[:, None] * side[None, :]).astype(np.float32)
    for f in (0, 1):
        rc, img, gain = _twin(rtlib, rtlib.lib().rt_denoise_monitor_blob, blob, dict(PAPER, search_radius=R, patch_radius=f), W, H)
        assert rc == 0 and np.array_equal(img, _plain(S1, n, W, H))
        assert np.array_equal(gain, np.round(gain)) and (gain >= 1).all()  # every weight is 0 or 1
        assert np.array_equal(gain, same_side) if f == 0 else (gain <= same_side).all() and (gain < same_side).any()
        far = np.r_[0:W // 2 - f, W // 2 + f:W]  # columns whose own patch does not straddle the edge
        assert (gain[:, far] > 1).all()


def test_argument_table(rtlib, quantised):
    W, H = 23, 19
    S1, S2 = nr.moments(quantised[(W, H)])
    L = rtlib.lib()
    fn = L.rt_denoise_monitor_blob
    good = nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2)
    small = dict(PAPER, search_radius=2, patch_radius=1)
    assert _twin(rtlib, fn, good, small, W, H)[0] == 0
    bad = [dict(search_radius=-1), dict(search_radius=11), dict(patch_radius=-1), dict(patch_radius=4), dict(k=0.0),
           dict(k=-1.0), dict(k=float("nan")), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(alpha=-0.5),
           dict(alpha=float("nan"))]
    for kw in bad:
        rc, img, gain = _twin(rtlib, fn, good, dict(small, **kw), W, H)
        assert rc == RT_ERR_ARG and _untouched(img, gain), kw
    # n < 2
    for n in (0, 1):
        blob = nr.pack(rtlib, _info(rtlib, W, H, n), S1 * np.uint64(0), S2 * np.uint64(0))
        rc, img, gain = _twin(rtlib, fn, blob, small, W, H)
        assert rc == RT_ERR_STATE and _untouched(img, gain)
    # a band tiling: every other band of 4 rows
    a = rtlib.make_args(W, H, 3, 2, NFB, 50, rtlib.RT_CAM_PER_PIXEL, seed=77, band_rows=4, band_first=0, band_stride=2)
    nv = len(rtlib.owned_rows(a)) * W * 3
    assert 0 < nv < W * H * 3
    band = nr.pack(rtlib, rtlib.rt_accum_info(a, nv, FP), S1[:nv], S2[:nv])
    info = rtlib.rt_accum_info()
    assert L.rt_noise_blob_info(band, len(band), ctypes.byref(info)) == 0 and info.n_values == nv
    rc, img, gain = _twin(rtlib, fn, band, small, W, H)
    assert rc == RT_ERR_ARG and _untouched(img, gain)
    # a malformed blob, a null image; null parameters are the defaults
    rc, img, gain = _twin(rtlib, fn, good[:-1], small, W, H)
    assert rc == RT_ERR_ARG and _untouched(img, gain)
    p = rtlib.denoise_params(small)
    assert fn(good, len(good), ctypes.byref(p), None, None) == RT_ERR_ARG
    rc, img, gain = _twin(rtlib, fn, good, None, W, H)
    assert rc == 0
    d = rtlib.denoise_params().as_dict()
    _same(img, gain, *dr.denoise(S1, S2, NFB, H, W, d["search_radius"], d["patch_radius"], d["k"], d["alpha"], d["eps"]))
    # the adaptive twin does not take a monitor's file, nor the monitor's an adaptive checkpoint
    assert _twin(rtlib, L.rt_denoise_adaptive_blob, good, small, W, H)[0] == RT_ERR_ARG


def test_denoise_checkpoint_files(rtlib, quantised, oracle, tmp_path):
    W, H = 23, 19
    S1, S2 = nr.moments(quantised[(W, H)])
    path = tmp_path / "m.noise"
    path.write_bytes(nr.pack(rtlib, _info(rtlib, W, H, NFB), S1, S2))
    prm = dict(PAPER, search_radius=3, patch_radius=1)
    want = dr.denoise(S1, S2, NFB, H, W, 3, 1, prm["k"], prm["alpha"], prm["eps"])
    img, gain = rtlib.denoise_checkpoint(str(path), prm, gain=True)
    _same(img, gain, *want)
    assert np.array_equal(rtlib.denoise_checkpoint(str(path), rtlib.denoise_params(prm)), want[0])
    with pytest.raises(rtlib.RtError) as e:
        rtlib.denoise_checkpoint(str(path), dict(prm, k=0.0))
    assert e.value.status == RT_ERR_ARG
    with pytest.raises(TypeError):
        rtlib.denoise_params(radius=3)
    n_t, n_px, A1, A2 = _mixed_counts(oracle, W, H, [2, 5, 9, 3])
    apath = tmp_path / "a.ckpt"
    apath.write_bytes(_adaptive_blob(rtlib, W, H, n_t, A1, A2))
    img, gain = rtlib.denoise_adaptive_checkpoint(str(apath), prm, gain=True)
    _same(img, gain, *dr.denoise(A1, A2, n_px, H, W, 3, 1, prm["k"], prm["alpha"], prm["eps"]))
    with pytest.raises(rtlib.RtError) as e:
        rtlib.denoise_checkpoint(str(apath), prm)
    assert e.value.status == RT_ERR_ARG
