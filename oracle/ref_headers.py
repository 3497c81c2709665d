"""ctypes wrapper of oracle/_ref/libref_headers.so: the reference's own class headers compiled for the
host (oracle/refhdr/ref_headers.cpp; built by `make -C oracle ref` where the reference is present).

TEST INFRASTRUCTURE ONLY: tests/test_refhdr_cpu.py pins the oracle to it, tests/golden/
make_refhdr_golden.py records its results.  The library is never committed and never travels without
the reference; `available()` says whether it is here.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_float, c_int, c_void_p

import numpy as np

from . import ref_cpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_ref", "libref_headers.so")
REFERENCE_ROOT = "/root/reference"

_lib = None


def available() -> bool:
    return os.path.exists(LIB_PATH)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not available():
            raise RuntimeError(f"{LIB_PATH} missing: run `make -C oracle ref` (needs the reference)")
        L = ctypes.CDLL(LIB_PATH)
        L.refhdr_scene_from_flat.argtypes = [c_void_p, POINTER(c_void_p)]
        L.refhdr_scene_destroy.argtypes = [c_void_p]
        L.refhdr_render.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
        L.refhdr_bvh_build.argtypes = [c_void_p, c_int, c_int, c_float, c_float] + [c_void_p] * 7
        L.refhdr_perlin_build.argtypes = [c_void_p] * 6
        L.refhdr_camera_build.argtypes = [c_void_p] * 3 + [c_float] * 6 + [c_void_p]
        L.refhdr_instance_consts.argtypes = [c_float, c_float, c_void_p]
        _lib = L
    return _lib


_states: dict = {}


def states(n: int, seed: int = 1984) -> np.ndarray:
    """curand_init(seed, slot, 0) for slot < n as (n, 6) words (d, v0..v4), from the oracle's pinned XORWOW."""
    key = (n, seed)
    if key not in _states:
        _states[key] = np.stack([ref_cpu.xorwow_init(seed, s, 0) for s in range(n)])
    return _states[key]


class HdrScene:
    """The reference's objects for a flattened rt_scene_soa (a ctypes struct, include/rt_hip.h)."""

    def __init__(self, soa):
        self._h = c_void_p()
        rc = lib().refhdr_scene_from_flat(ctypes.byref(soa), ctypes.byref(self._h))
        if rc != 0:
            raise ValueError("the reference's classes cannot hold this scene", rc)

    def render(self, W: int, H: int, spp: int, fb_id: int = 0, max_depth: int = 50, cam_mode: int = 0):
        """One frame buffer: (fb (H, W, 3) float32, segments (H, W) int32)."""
        fb = np.zeros((H, W, 3), np.float32)
        segs = np.zeros((H, W), np.int32)
        rc = lib().refhdr_render(self._h, W, H, spp, fb_id, max_depth, cam_mode, states(W * H).ctypes.data,
                                 fb.ctypes.data, segs.ctypes.data)
        if rc != 0:
            raise RuntimeError("refhdr_render failed")
        return fb, segs

    def bvh_build(self, first: int, n: int, state, t0: float = 0.0, t1: float = 1.0) -> dict:
        """bvh.h's build constructor over primitives [first, first + n); ref_cpu.bvh_build_call's dict."""
        return ref_cpu.bvh_build_call(lib().refhdr_bvh_build, self._h, first, n, state, t0, t1)

    def __del__(self):
        try:
            if self._h:
                lib().refhdr_scene_destroy(self._h)
        except Exception:
            pass


def camera_build(frm, at, vfov, aspect, aperture, focus, t0=0.0, t1=1.0, vup=(0, 1, 0)) -> np.ndarray:
    """camera.h's constructor: rt_camera's 24 floats (origin, lower_left, horizontal, vertical, u, v, w,
    lens_radius, time0, time1)."""
    out = np.zeros(24, np.float32)
    a = [np.ascontiguousarray(x, np.float32) for x in (frm, at, vup)]
    lib().refhdr_camera_build(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, vfov, aspect, aperture, focus, t0, t1,
                              out.ctypes.data)
    return out


def instance_consts(angle: float, density: float = 1.0) -> np.ndarray:
    """(sin_theta, cos_theta) of rotate_y's constructor for an angle in degrees and neg_inv_density of
    constant_medium's for a density."""
    out = np.zeros(3, np.float32)
    lib().refhdr_instance_consts(angle, density, out.ctypes.data)
    return out


def perlin_build(state) -> dict:
    """perlin.h's constructor from the six state words: its tables and the state afterwards."""
    out = {"ranvec": np.zeros((256, 3), np.float32), "perm_x": np.zeros(256, np.int32), "perm_y": np.zeros(256, np.int32),
           "perm_z": np.zeros(256, np.int32), "state": np.zeros(6, np.uint32)}
    st = np.ascontiguousarray(state, np.uint32)
    rc = lib().refhdr_perlin_build(st.ctypes.data, *[out[k].ctypes.data for k in ("ranvec", "perm_x", "perm_y", "perm_z", "state")])
    if rc != 0:
        raise RuntimeError("refhdr_perlin_build failed")
    return out
