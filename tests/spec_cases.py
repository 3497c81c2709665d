"""What tests/test_spec_cpu.py and tests/test_spec_gpu.py share: the scenes on which the casts and planes that
follow mirrors and glass (rt_spec_* of include/rt_hip.h) are checked, their camera rays, and the host twin's
answers computed once."""
from __future__ import annotations

import functools

import numpy as np

import aov_ref as ar
import flat_cases as fc
import raytracing_gpu_amd as rt
from flat_scenes import FlatScene

F32 = np.float32
W, H = 24, 16
PATH_FIELDS = ("bounces", "status", "first_prim", "first_material", "throughput", "depth")
STATUS = {"MISS": 0, "SURFACE": 1, "ESCAPED": 2, "LIMIT": 3, "ABSORBED": 4}


def _checker(s: FlatScene) -> int:
    return s.lambertian(s.checker(s.solid((0.2, 0.3, 0.1)), s.solid((0.9, 0.9, 0.9))))


def mirror_hall() -> FlatScene:
    """Two facing fuzz-0 metal rects in the planes x = -1.5 and x = 1.5, a lambertian floor and a sphere between
    them, seen from inside the hall at 45 degrees to its axis: neighbouring pixels have chains of 0 to more than
    16 bounces, ending on the floor, on the sphere or in the sky above the mirrors."""
    s = FlatScene()
    s.camera((0.0, 1.0, -1.0), (1.5, 0.9, 0.5), 60.0)
    left, right = s.metal((0.9, 0.9, 0.9), 0.0), s.metal((0.8, 0.85, 0.9), 0.0)
    s.world = [s.obj_prim(s.rect("yz", 0.0, 2.0, -2.0, 30.0, -1.5, left)), s.obj_prim(s.rect("yz", 0.0, 2.0, -2.0, 30.0, 1.5, right)),
               s.obj_prim(s.rect("xz", -1.5, 1.5, -2.0, 30.0, 0.0, _checker(s))),
               s.obj_prim(s.sphere((0.2, 0.5, 3.0), 0.5, s.lambertian((0.8, 0.3, 0.3))))]
    return s


def glass() -> FlatScene:
    """A glass sphere with a hollow inner sphere of negative radius (front and back faces) and a glass box
    (total internal reflection, ir 1.5) over a checker floor, the camera facing the ball."""
    s = FlatScene()
    s.camera((-0.7, 0.9, -4.0), (-0.2, 0.7, 0.0), 40.0)
    g = s.dielectric(1.5)
    s.world = [s.obj_prim(s.sphere((-0.7, 0.8, 0.0), 0.8, g)), s.obj_prim(s.sphere((-0.7, 0.8, 0.0), -0.7, g)),
               s.obj_prim(s.box((0.5, 0.0, -0.5), (1.5, 1.2, 0.5), g)), s.obj_prim(fc.ground(s, _checker(s), y=0.0)),
               s.obj_prim(s.sphere((0.3, 0.4, 2.0), 0.4, s.lambertian((0.8, 0.3, 0.3))))]
    return s


def glass_ball() -> FlatScene:
    """The glass sphere alone over the floor, filling the view from the front: the oracle pin's scene."""
    s = FlatScene()
    s.camera((0.0, 0.8, -4.0), (0.0, 0.8, 0.0), 24.0)
    s.world = [s.obj_prim(s.sphere((0.0, 0.8, 0.0), 0.8, s.dielectric(1.5))), s.obj_prim(fc.ground(s, _checker(s), y=0.0)),
               s.obj_prim(s.sphere((0.9, 0.4, 2.0), 0.4, s.lambertian((0.8, 0.3, 0.3))))]
    return s


def fuzz_threshold() -> FlatScene:
    """Three metal spheres of fuzz 0, 0.25 and 0.5: under max_fuzz = 0.25 the first two are mirrors (<=)."""
    s = FlatScene()
    s.camera((0.0, 1.0, -5.0), (0.0, 0.4, 0.0), 35.0)
    s.world = [s.obj_prim(s.sphere((-1.1, 0.5, 0.0), 0.5, s.metal((0.9, 0.6, 0.5), 0.0))),
               s.obj_prim(s.sphere((0.0, 0.5, 0.0), 0.5, s.metal((0.5, 0.9, 0.6), 0.25))),
               s.obj_prim(s.sphere((1.1, 0.5, 0.0), 0.5, s.metal((0.5, 0.6, 0.9), 0.5))),
               s.obj_prim(fc.ground(s, _checker(s), y=0.0))]
    return s


def moving_mirror() -> FlatScene:
    """A fuzz-0 metal sphere that moves during the shutter, between a lambertian one and the floor: the chain's
    continuation rays carry the primary ray's time."""
    s = FlatScene()
    s.camera((0.0, 1.0, -5.0), (0.0, 0.5, 0.0), 35.0, t0=0.0, t1=1.0)
    s.world = [s.obj_prim(s.moving((-0.6, 0.6, 0.0), (0.4, 1.1, 0.2), 0.0, 1.0, 0.6, s.metal((0.9, 0.9, 0.9), 0.0))),
               s.obj_prim(s.moving((1.2, 0.4, 0.3), (1.2, 0.9, 0.3), 0.0, 1.0, 0.4, s.lambertian((0.8, 0.3, 0.3)))),
               s.obj_prim(fc.ground(s, _checker(s), y=0.0))]
    return s


def medium_mirror() -> FlatScene:
    """A sphere of fog beside a mirror that shows it: seen directly or in the mirror, the chain ends on the medium's boundary, with the phase material."""
    s = FlatScene()
    s.camera((0.0, 1.0, -5.0), (0.0, 0.7, 0.0), 35.0)
    fog = s.isotropic((0.6, 0.7, 0.9))
    ball = s.obj_prim(s.sphere((0.3, 0.7, -0.5), 0.6, s.dielectric(1.5)))
    s.world = [s.obj_prim(s.rect("yz", 0.0, 2.0, -2.0, 2.0, 1.4, s.metal((0.9, 0.9, 0.9), 0.0))), s.medium(ball, 0.5, fog),
               s.obj_prim(fc.ground(s, _checker(s), y=0.0))]
    return s


def short_normal() -> FlatScene:
    """A fuzz-0 metal triangle without vertex normals: its shading normal is the unnormalised cross product of
    its edges, here of squared length 0.41 < 0.5, so the mirrored direction points into the surface and the
    reference's scatter returns false (RT_SPEC_ABSORBED)."""
    s = FlatScene()
    s.camera((0.0, 0.5, -3.0), (0.0, 0.4, 0.0), 35.0)
    s.world = [s.obj_prim(s.tri((-0.4, 0.1, 0.0), (0.4, 0.1, 0.0), (-0.4, 0.9, 0.0), s.metal((0.9, 0.9, 0.9), 0.0))),
               s.obj_prim(fc.ground(s, _checker(s), y=0.0))]
    return s


SCENES: dict = {"short_normal": short_normal, "mirror_hall": mirror_hall, "glass": glass, "glass_ball": glass_ball, "fuzz_threshold": fuzz_threshold,
                "moving_mirror": moving_mirror, "medium_mirror": medium_mirror,
                "first": functools.partial(rt.Scene.builtin, "first"), "big1": functools.partial(rt.Scene.builtin, "big1")}
# the scenes of the device tests ("every scene above")
DEVICE_SCENES = ("mirror_hall", "glass", "fuzz_threshold", "moving_mirror", "medium_mirror", "short_normal", "first", "big1")
BOUNCES = (0, 1, 4, 16)
_built: dict = {}


def scene(name: str):
    if name not in _built:
        _built[name] = SCENES[name]()
    return _built[name]


def soa(name: str):
    return scene(name).soa


@functools.lru_cache(maxsize=None)
def rays(name: str, n: int | None = None) -> np.ndarray:
    """Camera rays of a W x H image over two shutter times and the lens (three entries of the averaged pass's
    pattern), W * H of each in pixel order; the first n of them."""
    cam = soa(name).camera
    tab = ar.pattern(3)
    r = np.concatenate([ar.rays(cam, W, H, tab[k], 1) for k in range(3)])
    r.setflags(write=False)
    return r if n is None else r[:n]


@functools.lru_cache(maxsize=None)
def host_trace(name: str, max_bounces: int, max_fuzz: float = 0.25, glass_: int = 1):
    """rt.trace_host of rays(name), computed once and shared (read only)."""
    hits, paths = rt.trace_host(soa(name), rays(name), max_bounces=max_bounces, max_fuzz=max_fuzz, glass=glass_)
    hits.setflags(write=False), paths.setflags(write=False)
    return hits, paths


@functools.lru_cache(maxsize=None)
def host_planes(name: str, width: int, height: int, S: int | None, max_bounces: int) -> dict:
    """rt.guide_host(..., samples=S, specular=max_bounces), computed once and shared (read only)."""
    d = rt.guide_host(soa(name), width, height, samples=S, specular=dict(max_bounces=max_bounces))
    for a in d.values():
        a.setflags(write=False)
    return d


def diff_paths(a, b) -> str:
    bad = [f for f in PATH_FIELDS if np.asarray(a[f]).tobytes() != np.asarray(b[f]).tobytes()]
    return "path fields that differ: " + ", ".join(bad)
