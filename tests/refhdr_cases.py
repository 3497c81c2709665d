"""Scenes shared by the reference-header pins: tests/test_refhdr_cpu.py (the oracle against the reference's
own class headers compiled for the host, oracle/refhdr/), tests/golden/make_refhdr_golden.py (their recorded
results) and tests/test_refhdr_gpu.py (the kernels against the record, with no oracle in between)."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass

import numpy as np

import flat_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refhdr_renders.npz")
BUILTIN = ("basic", "first", "big1", "two_spheres", "two_perlin", "cornell", "cornell_smoke", "triangle", "triangles",
           "final", "earth", "door")
BUILTIN_SHAPE = (48, 27, 2, 2, 50)  # W, H, spp, fbs, depth
# The recorded cases: one written scene per group of flat_cases.py (the lds group's limits are the kernel's,
# not the reference's), and two built-in scenes.  All REF mode, flat_cases' 40 x 24, 4 spp, 2 fbs.
RECORDED = ("bvh:5_world", "boxes:shrunk_mid", "deep:chain", "time:shutter_quarter", "world:bvh_then_list",
            "camera:inside_glass", "shade:lambertian_checker_image_solid", "shade:glass_0.7_solid",
            "ties:sphere_twice_in_bvh", "random:8", "big1", "cornell_smoke")


@dataclass
class Entry:
    scene: object  # has .soa; what Context.upload takes
    depth: int


def builtin_assets(name: str):
    """(product keywords, oracle keywords) of a built-in scene: the synthetic texture and mesh the GPU
    parity tests use for the scenes that read files in the reference."""
    from raytracing_gpu_amd import assets

    if name not in ("earth", "door", "final"):
        return {}, {}
    img = assets.synthetic_image(341, 152)
    if name == "earth":
        return dict(images=[img]), dict(images=[img])
    m = assets.synthetic_mesh(24, 32, image=0)
    return dict(images=[img], meshes=[m]), dict(images=[img], meshes=[(m.tris, m.vertex_normals, m.image)])


@functools.lru_cache(maxsize=None)
def builtin_scene(name: str):
    """rt_scene_build's flattened scene (host only)."""
    import raytracing_gpu_amd as rt

    return rt.Scene.builtin(name, **builtin_assets(name)[0])


def recorded_entry(key: str) -> Entry:
    if ":" in key:
        c = flat_cases.get(key)
        return Entry(c.scene, c.depth)
    return Entry(builtin_scene(key), 50)


def key_name(key: str) -> str:
    return key.replace(":", "__")


def first_difference(got: np.ndarray, want: np.ndarray):
    """None, or (number of differing pixels, (row, column) of the first) of two (H, W, 3) float32 images
    compared as bits."""
    d = (np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32)).any(axis=2)
    return (int(d.sum()), tuple(int(x) for x in np.argwhere(d)[0])) if d.any() else None
