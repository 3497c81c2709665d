"""CPU checks of the flattened-scene path (no GPU, no context):

* the two scene builders agree: the oracle's own builders (RefScene(name)) and the oracle reading what
  rt_scene.cpp flattened (RefScene.from_flat(Scene.builtin(name).soa)) render the same bits and count
  the same segments, box tests and primitive tests, for every name rt_scene_build[_ex] accepts;
* every case and seed tests/test_flat_gpu.py renders is a usable input: finite floats, not sky, and
  the feature it is built around reached (flat_cases.py keeps the evidence with the case);
* rt_scene_validate refuses a table of scenes, each a valid one with one field broken.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import flat_cases
from flat_scenes import FlatScene

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ("basic", "first", "big1", "random", "two_spheres", "two_perlin", "cornell", "cornell_smoke", "triangle",
         "triangles", "backpack", "earth", "door", "cup", "final", "coincident", "coincident_step")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _assets(name):
    from raytracing_gpu_amd import assets

    if name not in ("earth", "door", "cup", "final"):
        return {}, {}
    img = assets.synthetic_image(341, 152)
    m = assets.synthetic_mesh(24, 32, image=0) if name == "cup" else \
        assets.door_mesh_from_fixture(os.path.join(GOLD, "door_assimp.npz"))
    return dict(images=[img], meshes=[m]), dict(images=[img], meshes=[(m.tris, True, 0)])


@pytest.mark.parametrize("name", NAMES)
def test_builders_agree(rtlib, oracle, name):
    """rt_scene.cpp's flattening against the oracle's independent builders, through from_flat: frame
    buffers bit for bit, and the three counters, 32x18, 2 spp, fb ids 0 and 3, both camera modes."""
    pa, oa = _assets(name)
    named = oracle.RefScene(name, **oa)
    host = rtlib.Scene.builtin(name, **pa)
    flat = oracle.RefScene.from_flat(host.soa)
    assert flat.aspect == named.aspect
    W, H, spp = 32, 18, 2
    for cam in (oracle.REF_CAM_REF_SLOT0, oracle.REF_CAM_PER_PIXEL):
        for fb in (0, 3):
            want, wc, _ = named.render(W, H, spp, fb, 50, cam)
            got, gc, _ = flat.render(W, H, spp, fb, 50, cam)
            assert np.array_equal(_bits(got), _bits(want)), f"{name} cam {cam} fb {fb}"
            assert gc == wc, f"{name} cam {cam} fb {fb}: {gc} != {wc}"


# ---------------------------------------------------------------- conditions on the GPU test's inputs
@pytest.mark.parametrize("case", flat_cases.all_case_ids())
def test_case_is_a_usable_input(oracle, rtlib, case):
    """The oracle alone on a committed case: rt_scene_validate accepts it, every float is finite (NaN
    payloads are not comparable across hosts), at least 1.3 segments per sample (not sky), and the
    case's own evidence that the branch it is built around is reached."""
    c = flat_cases.get(case)
    rc, why = rtlib.validate_scene(c.scene.soa)
    assert rc == 0, why
    r = flat_cases.oracle_render(oracle, case, flat_cases.REF)
    for fb in r.fbs:
        assert np.isfinite(fb).all()
    samples = flat_cases.W * flat_cases.H * flat_cases.SPP * flat_cases.NFB
    assert r.counters["samples"] == samples
    assert r.counters["segments"] >= 1.3 * samples, r.counters
    if c.evidence is not None:
        c.evidence(c, r, oracle)


def test_discarded_seeds_are_few():
    assert len(flat_cases.DISCARDED_SEEDS) * 8 <= len(flat_cases.DISCARDED_SEEDS) + len(flat_cases.SEEDS)
    assert len(flat_cases.SEEDS) == 32 and not set(flat_cases.SEEDS) & set(flat_cases.DISCARDED_SEEDS)


# ---------------------------------------------------------------- rt_scene_validate
def _valid():
    """One scene with every array in use: BVH, list, transform, media, triangle, every texture kind."""
    s = FlatScene()
    img = s.image(np.arange(5 * 3 * 3, dtype=np.uint8).reshape(3, 5, 3))
    ck = s.checker(s.solid((0.2, 0.3, 0.1)), s.noise(4.0))
    m_img, m_ck = s.lambertian(img), s.lambertian(ck)
    m_turb, m_glass = s.metal(s.turbulent(2.0, 3), 0.1), s.dielectric(1.5)
    ids = [s.sphere((x, 0, 0), 0.4, m) for x, m in ((-2, m_img), (-1, m_ck), (0, m_turb), (1, m_glass))]
    ids.append(s.tri((2, -0.5, 0), (3, -0.5, 0), (2, 0.5, 0), m_ck))
    s.world.append(s.bvh(ids))
    b = s.box((-1, 1, -1), (1, 2, 1), m_ck)
    s.world.append(s.xform(s.obj_prim(b), 15.0, (0, 0.5, 0)))
    r0 = s.rect("xz", -5, 5, -5, 5, -1, m_ck)
    s.rect("xy", -5, 5, -1, 5, 4, m_img)
    s.world.append(s.obj_list(r0, 2))
    s.world.append(s.medium(s.obj_prim(s.sphere((0, 3, 0), 0.5, m_glass)), 0.5, s.isotropic((1, 1, 1))))
    return s


def _break_object(kind, field, value):
    def f(s):
        o = next(o for o in s.objects if o.kind == kind)
        setattr(o, field, value)
    return f


def _break_last_row(field, value):
    def f(s):
        setattr(s.nodes[len(s.nodes) - 1], field, value)
    return f


def _set(seq, i, field, value):
    def f(s):
        setattr(getattr(s, seq)[i], field, value)
    return f


def _xform_self(s):
    k = next(k for k, o in enumerate(s.objects) if o.kind == 3)
    s.objects[k].a = k


def _medium_of_medium(s):
    k = next(k for k, o in enumerate(s.objects) if o.kind == 4)
    s.objects[k].a = k


def _xform_of_xform(s):
    k = next(k for k, o in enumerate(s.objects) if o.kind == 3)
    s.world.append(s.xform(k, 5.0))


def _leaf_twice(s):
    s.nodes[len(s.nodes) - 1].leaf_b = s.nodes[len(s.nodes) - 2].leaf_a


def _leaf_shared(s):
    s.world.append(s.obj_prim(s.nodes[len(s.nodes) - 1].leaf_a))


def _tri_index(v):
    def f(s):
        p = next(p for p in s.prims if p.type == 5)
        p.p[0] = v
    return f


def _image(field, value):
    def f(s):
        w, h, bpp, off = s.images[0]
        d = dict(width=w, height=h, bytes_per_pixel=bpp, offset=off)
        d[field] = value
        s.images[0] = (d["width"], d["height"], d["bytes_per_pixel"], d["offset"])
    return f


def _grey_without_tail(s):
    s.lambertian(s.image(np.zeros((4, 4), np.uint8)))  # the last texel's pixel[1..2] lie past texels


def _perm(s):
    s.perlins[0]["perm_y"][7] = 256


def _checker_of_checker(s):
    ck = next(k for k, t in enumerate(s.texs) if t.type == 1)
    s.texs[ck].a = ck


BROKEN = {
    "world_index_high": lambda s: s.world.append(len(s.objects)),
    "world_index_negative": lambda s: s.world.append(-1),
    "object_kind": _set("objects", 0, "kind", 5),
    "prim_object_index": _break_object(0, "a", 10 ** 6),
    "list_count": _break_object(1, "b", 10 ** 6),
    "list_count_zero": _break_object(1, "b", 0),
    "list_first_negative": _break_object(1, "a", -1),
    "bvh_rows_low": _break_object(2, "b", 1),
    "bvh_rows_high": _break_object(2, "b", 31),
    "bvh_nodes_short": _break_object(2, "a", 1),
    "bvh_leaf_a_missing": _break_last_row("leaf_a", -1),
    "bvh_leaf_a_high": _break_last_row("leaf_a", 10 ** 6),
    "bvh_leaf_b_high": _break_last_row("leaf_b", 10 ** 6),
    "bvh_leaf_b_low": _break_last_row("leaf_b", -2),
    "bvh_leaf_twice": _leaf_twice,
    "bvh_leaf_shared_with_prim_object": _leaf_shared,
    "xform_child_range": _break_object(3, "a", 10 ** 6),
    "xform_child_is_itself": _xform_self,
    "xform_of_xform": _xform_of_xform,
    "xform_flags": _break_object(3, "b", 4),
    "medium_child_range": _break_object(4, "a", -1),
    "medium_of_medium": _medium_of_medium,
    "medium_phase_material": _break_object(4, "b", 10 ** 6),
    "prim_type": _set("prims", 0, "type", 7),
    "prim_material": _set("prims", 0, "material", 10 ** 6),
    "triangle_index_high": _tri_index(1.0),
    "triangle_index_negative": _tri_index(-1.0),
    "triangle_index_fraction": _tri_index(0.5),
    "material_type": _set("mats", 0, "type", 5),
    "material_texture": _set("mats", 0, "texture", 10 ** 6),
    "material_texture_negative": _set("mats", 0, "texture", -1),
    "texture_type": _set("texs", 0, "type", 6),
    "image_index": _set("texs", 0, "a", 3),
    "checker_even": _set("texs", 3, "a", 10 ** 6),
    "checker_odd": _set("texs", 3, "b", -1),
    "checker_of_checker": _checker_of_checker,
    "perlin_index": _set("texs", 2, "a", 2),
    "perlin_permutation_entry": _perm,
    "turbulence_depth": _set("texs", 4, "b", -1),
    "image_offset": _image("offset", 10),
    "image_offset_negative": _image("offset", -1),
    "image_height": _image("height", 0),
    "image_bytes_per_pixel": _image("bytes_per_pixel", 5),
    "image_too_wide": _image("width", 6),
    "grey_image_without_tail": _grey_without_tail,
}


# the reason each entry must be refused for (a substring of rt_scene_validate's message)
REASON = {
    "world_index_high": "world index",
    "world_index_negative": "world index",
    "object_kind": "unknown kind",
    "prim_object_index": "prim index",
    "list_count": "prim index",
    "list_count_zero": "prim index",
    "list_first_negative": "prim index",
    "bvh_rows_low": "bvh out of range",
    "bvh_rows_high": "bvh out of range",
    "bvh_nodes_short": "bvh out of range",
    "bvh_leaf_a_missing": "bvh leaf out of range",
    "bvh_leaf_a_high": "bvh leaf out of range",
    "bvh_leaf_b_high": "bvh leaf out of range",
    "bvh_leaf_b_low": "bvh leaf out of range",
    "bvh_leaf_twice": "bvh leaf twice",
    "bvh_leaf_shared_with_prim_object": "also a bvh leaf",
    "xform_child_range": "child object out of range",
    "xform_child_is_itself": "transform child kind",
    "xform_of_xform": "transform child kind",
    "xform_flags": "transform flags",
    "medium_child_range": "child object out of range",
    "medium_of_medium": "medium boundary kind",
    "medium_phase_material": "phase material",
    "prim_type": "unknown type",
    "prim_material": "prim material",
    "triangle_index_high": "triangle index",
    "triangle_index_negative": "triangle index",
    "triangle_index_fraction": "triangle index",
    "material_type": "material 0: unknown type",
    "material_texture": "material 0: texture",
    "material_texture_negative": "material 0: texture",
    "texture_type": "texture 0: unknown type",
    "image_index": "image out of range",
    "checker_even": "checker texture out of range",
    "checker_odd": "checker texture out of range",
    "checker_of_checker": "checker of a checker",
    "perlin_index": "perlin table",
    "perlin_permutation_entry": "permutation entry",
    "turbulence_depth": "turbulence depth",
    "image_offset": "image 0: texels",
    "image_offset_negative": "image 0: texels",
    "image_height": "image 0: texels",
    "image_bytes_per_pixel": "image 0: texels",
    "image_too_wide": "image 0: texels",
    "grey_image_without_tail": "image 1: texels",
}
assert set(REASON) == set(BROKEN)


def test_valid_scene_is_accepted(rtlib, oracle):
    s = _valid()
    assert [t.type for t in s.texs[:5]] == [5, 0, 2, 1, 3]  # the indices the table breaks
    assert rtlib.validate_scene(s.soa) == (0, "")
    oracle.RefScene.from_flat(s.soa).render(8, 6, 1)


@pytest.mark.parametrize("name", list(BROKEN))
def test_broken_scene_is_refused(rtlib, oracle, name):
    """A valid scene with one field broken: RT_ERR_SCENE with a message, and the oracle's from_flat
    returns a status (it never aborts).  No context is created and nothing renders."""
    s = _valid()
    BROKEN[name](s)
    rc, why = rtlib.validate_scene(s.soa)
    assert rc == rtlib.RT_ERR_SCENE and REASON[name] in why, (rc, why)
    if name not in ("bvh_leaf_twice", "bvh_leaf_shared_with_prim_object"):  # the oracle has no such limit
        with pytest.raises(ValueError):
            oracle.RefScene.from_flat(s.soa)


def test_validate_arguments(rtlib):
    s = _valid()
    L = rtlib.lib()
    assert L.rt_scene_validate(None, None, 0) == rtlib.RT_ERR_ARG
    assert L.rt_scene_validate(ctypes.byref(s.soa), None, 0) == 0
    BROKEN["prim_type"](s)
    assert L.rt_scene_validate(ctypes.byref(s.soa), None, 0) == rtlib.RT_ERR_SCENE
    tiny = ctypes.create_string_buffer(4)
    assert L.rt_scene_validate(ctypes.byref(s.soa), tiny, 4) == rtlib.RT_ERR_SCENE and len(tiny.value) == 3


# ---------------------------------------------------------------- the camera and the spheres of BVHs
@pytest.mark.parametrize("kind", ["far_camera", "far_camera_instance", "far_camera_medium_boundary"])
def test_far_camera_is_refused(rtlib, kind):
    """A camera 1e4 from a unit scene sees its BVH's spheres from 22 000 radii: sphere.h's float test no
    longer resolves them (include/rt_hip.h, rt_scene_validate), whether the BVH is a world entry, under a
    transform or a medium's boundary.  The same scene from 400 radii passes (tests/test_flat_gpu.py)."""
    rc, why = rtlib.validate_scene(flat_cases.camera_case(kind).soa)
    assert rc == rtlib.RT_ERR_SCENE and "512 radii" in why, (rc, why)
    assert rtlib.validate_scene(flat_cases.camera_case(kind.replace("far_camera", "far_400r")).soa) == (0, "")


def test_far_moving_sphere_is_judged_over_the_shutter(rtlib):
    """A moving sphere near the camera at time0 and 1e4 away, in view, at time1."""
    def scene(t1):
        s = flat_cases.look(FlatScene(), t0=0.0, t1=t1)
        m = s.lambertian((0.5, 0.5, 0.5))
        ids = [s.moving((0, 0.1, 0.8), (-800.0, -3199.9, 10000.8), 0.0, 1.0, 0.45, m), s.sphere((1.1, 0, 0), 0.45, m),
               flat_cases.ground(s)]
        s.world.append(s.bvh(ids))
        return s
    assert rtlib.validate_scene(scene(0.01).soa) == (0, "")
    rc, why = rtlib.validate_scene(scene(1.0).soa)
    assert rc == rtlib.RT_ERR_SCENE and why.startswith("prim 0:") and "512 radii" in why, (rc, why)


def test_far_sphere_out_of_view_is_accepted(rtlib):
    """big1's placeholder spheres (r = 1e-5 at 1.7e4 from the camera, behind it) are no camera ray's business."""
    assert rtlib.validate_scene(rtlib.Scene.builtin("big1").soa) == (0, "")
