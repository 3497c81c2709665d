"""Tile launches and the adaptive accumulator, host side (no GPU): the rt_render_tiles / rt_adapt_* ABI
is declared, exported and bound, the ctypes mirror of rt_adapt_report has the C struct's size, the
numpy model of tests/adapt_ref.py behaves as include/rt_hip.h says on hand-made planes, and rt_main
refuses --adaptive together with --progressive or --checkpoint."""
import ctypes
import os
import re
import subprocess

import numpy as np

import adapt_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_MAIN = os.path.join(ROOT, "examples", "bin", "rt_main")
INT_NAMES = ["rt_adapt_create", "rt_adapt_add", "rt_adapt_retire", "rt_adapt_image", "rt_adapt_counts",
             "rt_adapt_noise_map", "rt_adapt_get_report", "rt_adapt_destroy"]
FLOAT_NAMES = ["rt_adapt_last_add_ms", "rt_adapt_last_retire_ms"]


def test_adapt_abi_declared_exported_bound(rtlib):
    hdr = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert set(re.findall(r"^\s*int\s+(rt_adapt_\w+)\s*\(", hdr, re.M)) == set(INT_NAMES)
    assert set(re.findall(r"^\s*float\s+(rt_adapt_\w+)\s*\(", hdr, re.M)) == set(FLOAT_NAMES)
    assert re.search(r"^\s*int\s+rt_render_tiles\s*\(", hdr, re.M)
    L = rtlib.lib()
    for n in INT_NAMES + FLOAT_NAMES + ["rt_render_tiles"]:
        assert hasattr(L, n) and n in rtlib.ABI, n


def test_adapt_report_mirror_has_the_c_size(rtlib, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "rt_hip.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(rt_adapt_report), sizeof(rt_render_args)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    report, args = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(rtlib.rt_adapt_report) == report == 56
    assert ctypes.sizeof(rtlib.rt_render_args) == args
    assert [n for n, _ in rtlib.rt_adapt_report._fields_] == [
        "fbs", "tiles_x", "tiles_y", "tiles_active", "pixels", "pixels_active", "pixel_fbs", "pixels_above",
        "threshold", "max_noise"]


# ---------------------------------------------------------------- the model on hand-made planes
ROWS, WIDTH, NFB = 20, 40, 8  # 2 x 3 tiles, partial in both directions
ALT = (3, 17)                 # the alternating pixel: tile 1


def _planes(alternating=True):
    p = np.full((NFB, ROWS, WIDTH, 3), 100, np.uint8)
    p[:, :, 32:] = 200  # another constant in the last tile column
    if alternating:
        p[0::2, ALT[0], ALT[1]] = 10
        p[1::2, ALT[0], ALT[1]] = 250
    return p.reshape(NFB, -1)


def test_model_constant_tiles_retire_at_the_first_retire():
    out = ar.run(_planes(False), ROWS, WIDTH, [("add", 2), ("retire", 0.0, 0), ("add", 2)])
    assert (out["counts"] == 2).all() and out["fbs"] == 2
    rep = out["reports"][0]
    assert rep == {"fbs": 2, "tiles_x": 3, "tiles_y": 2, "tiles_active": 0, "pixels": ROWS * WIDTH, "pixels_active": 0,
                   "pixel_fbs": 2 * ROWS * WIDTH, "pixels_above": 0, "threshold": 0.0, "max_noise": 0.0}
    # quant(sum / n) of a constant plane c: int(256 * min(sqrt(c^2 / 65025), 0.999))
    assert out["image"][0, 0, 0] == int(256 * (100 / 255)) and out["image"][0, 39, 0] == int(256 * (200 / 255))
    assert (out["noise"] == 0).all()


def test_model_alternating_pixel_keeps_its_tile_active():
    steps = [("add", 2), ("retire", 0.5, 0), ("add", 2), ("retire", 0.5, 0), ("add", 2)]
    out = ar.run(_planes(), ROWS, WIDTH, steps)
    want = np.full((2, 3), 2, np.int32)
    want[0, 1] = 6
    assert np.array_equal(out["counts"], want)
    for k, rep in enumerate(out["reports"]):
        assert (rep["fbs"], rep["tiles_active"], rep["pixels_active"], rep["pixels_above"]) == (2 * k + 2, 1, 256, 1)
        assert rep["pixel_fbs"] == 2 * (ROWS * WIDTH - 256) + 256 * (2 * k + 2)
        assert rep["max_noise"] == out["maps"][k][ALT] > 0.5
        assert (np.delete(out["maps"][k].reshape(-1), ALT[0] * WIDTH + ALT[1]) == 0).all()
    # every pixel is the plain image of its tile's own count
    p = _planes().reshape(NFB, ROWS, WIDTH, 3).astype(np.float32)
    for n in (2, 6):
        acc = np.zeros((ROWS, WIDTH, 3), np.float32)
        for f in range(n):
            acc += p[f] * p[f] / np.float32(65025)
        sel = np.repeat(np.repeat(out["counts"], 16, 0), 16, 1)[:ROWS, :WIDTH] == n
        assert np.array_equal(out["image"][sel], ar.quant(acc / np.float32(n)).astype(np.uint8)[sel])


def test_model_max_above_one_lets_it_retire_and_retiring_is_final():
    steps = [("add", 2), ("retire", 0.5, 1), ("add", 4), ("retire", -1.0, 0)]
    out = ar.run(_planes(), ROWS, WIDTH, steps)
    assert (out["counts"] == 2).all() and out["fbs"] == 2  # the add after everything retired does nothing
    first, second = out["reports"]
    assert (first["tiles_active"], first["pixels_above"]) == (0, 1)
    # a retire that nothing could pass brings no tile back; every pixel is above a negative threshold
    assert (second["tiles_active"], second["fbs"], second["pixels_above"]) == (0, 2, ROWS * WIDTH)
    assert second["pixel_fbs"] == first["pixel_fbs"] == 2 * ROWS * WIDTH


def test_model_does_not_depend_on_how_adds_are_split():
    rng = np.random.default_rng(5)
    planes = rng.integers(0, 256, (NFB, ROWS * WIDTH * 3)).astype(np.uint8)
    planes[:, : 16 * WIDTH * 3] //= 64  # the upper tile row is quieter in absolute terms
    a = ar.run(planes, ROWS, WIDTH, [("add", 4), ("retire", 12.0, 3), ("add", 4), ("retire", 12.0, 3)])
    b = ar.run(planes, ROWS, WIDTH, [("add", 1)] * 4 + [("retire", 12.0, 3)] + [("add", 3), ("add", 1), ("retire", 12.0, 3)])
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["image"], b["image"])
    assert np.array_equal(a["noise"].view(np.uint32), b["noise"].view(np.uint32)) and a["reports"] == b["reports"]


# ---------------------------------------------------------------- the item list of a tile launch, on the CPU
def test_tile_list_records_are_a_permutation(tmp_path):
    """scripts/check_tile_list.cpp replays tile_items_kernel's index arithmetic over the host's records
    (csrc/rt_tile_list.h): every store lands inside the item list, the list is a permutation of the
    listed tiles' items, a tile's pixels of one frame buffer in one run."""
    hdr = open(os.path.join(ROOT, "raytracing_gpu_amd", "csrc", "rt_tile_list.h")).read()
    assert not re.search(r'#\s*include\s*[<"]hip', hdr)
    exe = tmp_path / "check_tile_list"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "raytracing_gpu_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "check_tile_list.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "check_tile_list ok" in r.stdout, r.stderr


# ---------------------------------------------------------------- rt_main's option checks (before any GPU call)
def test_rt_main_refuses_adaptive_with_progressive_or_checkpoint(rtlib, tmp_path):
    from raytracing_gpu_amd import _build

    _build.build_examples()
    out = str(tmp_path / "o.ppm")
    base = [RT_MAIN, "big1", "70", "2", "8", out, "--adaptive", "2", "--until-noise", "1.0"]
    for extra in (["--progressive", "2"], ["--checkpoint", str(tmp_path / "c.bin")]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 99 and "--adaptive" in r.stderr and "cannot be combined" in r.stderr, r.stderr
        assert not os.path.exists(out)
    r = subprocess.run(base[:6] + ["--adaptive", "2"], capture_output=True, text=True)
    assert r.returncode == 99 and "needs --until-noise" in r.stderr
    r = subprocess.run(base[:6] + ["--max-above", "2"], capture_output=True, text=True)
    assert r.returncode == 99 and "need --adaptive" in r.stderr
