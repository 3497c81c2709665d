"""What tests/test_guide_cpu.py and tests/test_guide_gpu.py share: the scenes the ray casts are checked on, the
camera rays the oracle captures on them (ref_capture_rays, bound here: oracle/ref_cpu.py is left as it is) and
the hits as arrays."""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import flat_cases as fc
import raytracing_gpu_amd as rt
from flat_scenes import FlatScene

W, H = 24, 16
HIT_FIELDS = ("t", "p", "n", "albedo", "u", "v", "prim", "material", "front", "pad")


def one_prim(kind: str) -> FlatScene:
    """The ground and one primitive of a kind, every material lambertian."""
    s = fc.look(FlatScene())
    m, g = s.lambertian((0.8, 0.3, 0.3)), s.lambertian(s.checker(s.solid((0.2, 0.3, 0.1)), s.solid((0.9, 0.9, 0.9))))
    nrm = [(0.2, 0.1, -1.0), (-0.2, 0.1, -1.0), (0.0, -0.3, -1.0)]
    tv = ((-1.0, -0.3, 1.2), (1.0, -0.2, 0.9), (0.1, 1.5, 1.4))
    if kind == "rect_xy":
        o = s.obj_prim(s.rect("xy", -1.2, 1.0, -0.2, 1.4, 1.5, m))
    elif kind == "rect_xz":
        o = s.obj_prim(s.rect("xz", -1.2, 1.0, 0.0, 2.0, 0.3, m))
    elif kind == "rect_yz":
        o = s.obj_prim(s.rect("yz", -0.3, 1.4, 0.0, 2.0, 0.6, m))
    elif kind == "box":
        o = s.obj_prim(s.box((-0.8, -0.3, 0.2), (0.7, 0.9, 1.5), m))
    elif kind == "box_moved":
        o = s.xform(s.obj_prim(s.box((-0.8, -0.3, -0.6), (0.7, 0.9, 0.7), m)), 25.0, (0.3, 0.1, 1.0))
    elif kind == "box_rotated_only":
        o = s.xform(s.obj_prim(s.box((-0.8, -0.3, 0.2), (0.7, 0.9, 1.5), m)), -35.0, flags=2)
    elif kind == "tri_flat":
        o = s.obj_prim(s.tri(*tv, m))
    elif kind == "tri_normals":
        o = s.obj_prim(s.tri(*tv, m, uv=(0.1, 0.1, 0.9, 0.2, 0.4, 0.8), normals=nrm))
    s.world = [o, s.obj_prim(fc.ground(s, g))]
    return s


ONE_PRIM_KINDS = ("rect_xy", "rect_xz", "rect_yz", "box", "box_moved", "box_rotated_only", "tri_flat", "tri_normals")
TIE_KINDS = ("sphere_twice_in_bvh", "sphere_across_entries", "triangle_in_list_and_bvh", "moving_spheres")

# name -> builder of a FlatScene or of a built-in rt.Scene: media-free scenes whose materials all scatter
SCENES: dict = {}
for _n in (3, 4, 5):
    SCENES[f"garden_{_n}_bvh"] = functools.partial(fc.garden, _n, _n)
    SCENES[f"garden_{_n}_list"] = functools.partial(fc.garden, _n, _n, True)
SCENES["movers"] = functools.partial(fc.movers, 0.25, 0.75)
for _k in ONE_PRIM_KINDS:
    SCENES[_k] = functools.partial(one_prim, _k)
for _k in TIE_KINDS:
    SCENES[f"ties_{_k}"] = functools.partial(fc.ties, _k)
    SCENES[f"ties_{_k}_swapped"] = functools.partial(fc.ties, _k, True)
SCENES["chain"] = fc.chain
SCENES["big1"] = functools.partial(rt.Scene.builtin, "big1")
SCENES["cornell"] = functools.partial(rt.Scene.builtin, "cornell")

# further scenes of the device tests: media, every world shape, the random grammar
MORE: dict = {f"media_{k}": functools.partial(fc.media_limits, k) for k in ("tiny_dt", "far")}
for _k in ("one_prim", "one_bvh", "bvh_7_prims", "bvh_8_prims", "bvh_then_list", "two_bvhs", "instanced_bvhs", "medium_over_list",
           "medium_over_xform", "medium_over_bvh", "medium_not_last", "entries_9", "entries_17"):
    MORE[f"world_{_k}"] = functools.partial(fc.world_shape, _k)
for _s in range(4):
    MORE[f"random_{_s}"] = functools.partial(fc.random_scene, _s)


def grazing() -> FlatScene:
    """Rects in the planes z = 0 and y = 0 and a box with a face in x = 0.5, for rays that start on a plane,
    reach it at t = 0.001 exactly, or run parallel to it."""
    s = FlatScene()
    s.camera((0, 0.5, -4), (0, 0, 0), 40.0)
    m = [s.lambertian((0.8, 0.3, 0.3)), s.lambertian(s.checker(s.solid((0.2, 0.3, 0.1)), s.solid((0.9, 0.9, 0.9)))), s.metal((0.7, 0.7, 0.7), 0.0)]
    s.world = [s.obj_prim(s.rect("xy", -1.0, 1.0, -1.0, 1.0, 0.0, m[0])), s.obj_prim(s.rect("xz", -2.0, 2.0, -2.0, 2.0, 0.0, m[1])),
               s.obj_prim(s.box((0.5, 0.25, 0.5), (1.5, 1.0, 1.5), m[2])), s.obj_prim(s.rect("yz", -1.0, 1.0, -1.0, 1.0, -1.5, m[0]))]
    return s


MORE["grazing"] = grazing
GRAZING_RAYS = np.array([
    [0.2, 0.3, 0.0, 0.0, 0.0, 1.0, 0, 0],        # from the xy rect's plane: t = 0 there, nothing behind
    [0.2, 0.3, 0.0, 0.0, -1.0, 0.0, 0, 0],       # in the xy rect's plane, towards the xz rect: parallel, t = inf
    [0.2, 0.3, -0.001, 0.0, 0.0, 1.0, 0, 0],     # t = 0.001 exactly: a hit (t < 0.001 is false)
    [0.2, 0.3, -0.00099, 0.0, 0.0, 1.0, 0, 0],   # just inside: no hit on that rect
    [0.2, 0.001, -3.0, 0.0, -1.0, 0.0, 0, 0],    # onto the xz rect at t = 0.001
    [0.2, 0.0, -3.0, 0.0, 1.0, 0.0, 0, 0],       # from the xz rect's plane upwards
    [0.0, 0.5, 1.0, 1.0, 0.0, 0.0, 0, 0],        # axis-aligned onto the box's x = 0.5 face
    [0.5, 0.5, 1.0, 1.0, 0.0, 0.0, 0, 0],        # from that face's plane: the far face
    [0.625, 0.5, -3.0, 0.0, 0.0, 1.0, 0, 0],     # parallel to four of the box's faces (t = +-inf there), through two
    [-1.375, 0.125, -3.0, 0.0, 0.0, 1.0, 0, 0],  # beside the yz rect's plane (inside it: 0 / 0) and the xz rect's: t = inf
    [-1.25, 0.125, -3.0, 0.0, 0.0, 1.0, 0, 0],   # parallel to the yz rect and the xz rect at once, beside both
    [-3.0, 0.5, -0.5, 1.0, 0.0, 0.0, 0.5, 0],    # axis-aligned through the yz rect
], np.float32)


def extra_rays(name: str) -> np.ndarray:
    """Rays with zero direction components from the camera's origin and a point beside it; on `grazing` also
    GRAZING_RAYS.  None of them evaluates 0 / 0 in a primitive test (whose NaN sign differs between processors)."""
    o = np.array(list(soa(name).camera.origin), np.float32)
    rays = []
    for org in (o, o + np.float32(0.25)):
        for d in ((0, 0, 1), (0, -1, 0), (1, 0, 0), (0, -1, 1), (1, 0, 1), (-1, -1, 0)):
            rays.append([*org, *d, 0.5, 0])
    rays = np.array(rays, np.float32)
    return np.concatenate([rays, GRAZING_RAYS]) if name == "grazing" else rays


_built: dict = {}


def scene(name: str):
    """The built scene (kept: its arrays back every .soa handed out)."""
    if name not in _built:
        _built[name] = (SCENES.get(name) or MORE[name])()
    return _built[name]


def soa(name: str):
    return scene(name).soa


def capture(oracle, soa_, depth: int, width: int = W, height: int = H):
    """(records [n][8] float32, fb [height][width][3]) of a one-sample render of one thread with the per-pixel
    camera: every world query as o, d, time, bounce depth."""
    L = oracle.lib()
    L.ref_capture_rays.restype = ctypes.c_longlong
    L.ref_capture_rays.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    ref = oracle.RefScene.from_flat(soa_)
    buf = np.zeros((width * height * depth + 8, 8), np.float32)
    L.ref_capture_rays(buf.ctypes.data, len(buf))
    try:
        fb, _, _ = ref.render(width, height, 1, 0, depth, oracle.REF_CAM_PER_PIXEL, threads=1)
    finally:
        n = L.ref_capture_rays(None, 0)
    assert n <= len(buf)
    return buf[:n].copy(), fb.reshape(height, width, 3)


@functools.lru_cache(maxsize=None)
def camera_rays(name: str):
    """(rays [W*H][8], follows [W*H] bool, origin of the following record [W*H][3]) of a depth-2 render: every
    camera ray in pixel order, whether a depth-1 record follows it directly, and that record's origin."""
    from oracle import ref_cpu

    rec, _ = capture(ref_cpu, soa(name), 2)
    cam = np.flatnonzero(rec[:, 7] == 0)
    assert len(cam) == W * H, "one depth-0 record per pixel"
    nxt = np.minimum(cam + 1, len(rec) - 1)
    follows = (cam + 1 < len(rec)) & (rec[nxt, 7] == 1)
    return rec[cam].copy(), follows, rec[nxt, :3].copy()


def same_hits(a, b) -> bool:
    """Two hit arrays equal bit for bit in every field."""
    return a.tobytes() == b.tobytes()


def diff_hits(a, b) -> str:
    bad = [f for f in HIT_FIELDS if np.asarray(a[f]).tobytes() != np.asarray(b[f]).tobytes()]
    return "fields that differ: " + ", ".join(bad)
