"""The CPU oracle pinned to the reference's own class headers, compiled for the host.

oracle/ref_cpu.cpp restates the reference by reading, and every GPU test ends in a comparison with it: a
misreading the oracle and the kernels share (a double promotion, an operand order, < against <=, the BVH's
visit and tie order, rotate_y's frame mix) would go unnoticed.  oracle/refhdr/ compiles hit, scatter,
emitted, value, get_ray, bounding_box and the BVH from the reference's headers themselves, and here the
oracle must give that library's float bits and segment counts, with no tolerance: on every written scene of
flat_cases.py (the branches the built-in scenes never take), on every built-in scene through
rt_scene_build's flattened output (which also holds rt_scene.cpp's flattening to the reference's classes),
on the builds that draw from the scene RNG (BVH leaf order and boxes, perlin's tables), and on the
constructors whose inputs the flat format does not keep (camera, rotate_y, constant_medium).  Fields that the
reference's classes compute themselves (rect extents, moving-sphere differences, a triangle's edges and dot
products) are never overwritten: the library refuses a record that does not hold the constructor's bits.
That found tests/flat_scenes.py's tri() summing its dot products in another order than triangle.h:28-30
(53 written scenes carried such a record, 12 of them then differed in 1 to 27 px); the writer was fixed, the oracle and the kernels were right.

The library exists only where the reference does: those tests skip where its directory is absent.
tests/golden/refhdr_renders.npz carries twelve of its results, which the oracle is checked against
everywhere (and the kernels in tests/test_refhdr_gpu.py).

Negative controls (the wrapper built once more, nothing committed): with -ffp-contract=fast -march=native,
82 of the 138 (case, camera mode) pairs of flat_cases.py differ; with material.h:102's pow(., 5) left to
the host's double pow, none does (the value only feeds a comparison with a uniform draw).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import flat_cases
import refhdr_cases
from flat_cases import NFB, PIX, REF, SPP, H, W
from flat_scenes import PERLIN_DTYPE
from refhdr_cases import first_difference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case: why the reference has no class for something in it (at most 1 in 8 cases, every group keeps one)
EXCLUDED: dict = {}


@pytest.fixture(scope="module")
def hdr():
    """oracle/_ref/libref_headers.so through oracle/ref_headers.py; built in-tree if absent."""
    from oracle import ref_headers

    if not os.path.isdir(ref_headers.REFERENCE_ROOT):
        pytest.skip("the reference is not on this machine")
    if not ref_headers.available():
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True, stdout=subprocess.DEVNULL)
    ref_headers.lib()
    return ref_headers


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_exclusions_within_the_cap():
    ids = flat_cases.all_case_ids()
    assert set(EXCLUDED) <= set(ids)
    assert 8 * len(EXCLUDED) <= len(ids)
    for g in {k.split(":")[0] for k in ids}:
        assert any(k not in EXCLUDED for k in flat_cases.group(g)), g


def _flat_params():
    out = []
    for name in flat_cases.all_case_ids():
        if name in EXCLUDED:
            continue
        out.append(pytest.param(name, REF, id=f"{name}-ref"))
        if flat_cases.CASES[name].per_pixel:
            out.append(pytest.param(name, PIX, id=f"{name}-per_pixel"))
    return out


@pytest.mark.parametrize("name,cam", _flat_params())
def test_written_scene(hdr, oracle, name, cam):
    c = flat_cases.get(name)
    want = hdr.HdrScene(c.scene.soa)
    got = flat_cases.oracle_render(oracle, name, cam)
    segs = np.zeros((H, W), np.int64)
    for f in range(NFB):
        fb, sg = want.render(W, H, SPP, f, c.depth, cam)
        segs += sg
        d = first_difference(got.fbs[f], fb)
        assert d is None, f"{name} fb {f}: {d[0]} px differ, first at {d[1]}"
    d = np.argwhere(got.segs != segs)
    assert not len(d), f"{name}: segments of {len(d)} px differ, first at {d[0]}"


@pytest.mark.parametrize("cam", [REF, PIX], ids=["ref", "per_pixel"])
@pytest.mark.parametrize("name", refhdr_cases.BUILTIN)
def test_builtin_scene(hdr, oracle, name, cam):
    """The oracle's own builders against the reference's classes over rt_scene_build's arrays."""
    Wb, Hb, spp, nfb, depth = refhdr_cases.BUILTIN_SHAPE
    want = hdr.HdrScene(refhdr_cases.builtin_scene(name).soa)
    ref = oracle.RefScene(name, **refhdr_cases.builtin_assets(name)[1])
    assert not ref.h20
    for f in range(nfb):
        got, _, gs = ref.render(Wb, Hb, spp, f, depth, cam, seg_per_pixel=True)
        fb, sg = want.render(Wb, Hb, spp, f, depth, cam)
        d = first_difference(got.reshape(Hb, Wb, 3), fb)
        assert d is None, f"{name} fb {f}: {d[0]} px differ, first at {d[1]}"
        d = np.argwhere(gs.reshape(Hb, Wb) != sg)
        assert not len(d), f"{name} fb {f}: segments of {len(d)} px differ, first at {d[0]}"


# ---------------------------------------------------------------- builds that draw from the scene RNG
def _flat_bvh(soa, rtlib):
    """The one BVH of a flattened scene: (first primitive, count, nodes as arrays)."""
    (o,) = [soa.objects[k] for k in range(soa.n_objects) if soa.objects[k].kind == rtlib.OBJ_BVH]
    inner, last0 = (1 << o.b) - 1, (1 << (o.b - 1)) - 1
    nd = [soa.nodes[o.a + k] for k in range(inner)]
    la = np.array([n.leaf_a for n in nd], np.int32)
    lb = np.array([n.leaf_b for n in nd], np.int32)
    leaves = np.concatenate([la[last0:], lb[last0:][lb[last0:] >= 0]])
    first, n = int(leaves.min()), len(leaves)
    assert sorted(leaves) == list(range(first, first + n))
    return first, n, last0, la, lb, np.array([list(n.lo) for n in nd], np.float32), np.array([list(n.hi) for n in nd], np.float32)


def _same_build(a, b, what):
    for k in ("leaf_a", "leaf_b", "axes", "state"):
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs, first at {np.argwhere(a[k] != b[k])[0]}"
    for k in ("lo", "hi"):
        d = np.argwhere(_bits(a[k]) != _bits(b[k]))
        assert not len(d), f"{what}: {k} of node {d[0][0]} differs"


@pytest.mark.parametrize("name", ["big1", "triangles"])
def test_builtin_bvh_build(hdr, oracle, rtlib, name):
    """bvh.h's build constructor (its merge sorts, its per-node axis draw), run over the flattened
    primitives from the scene RNG state at the point the scene builds its tree, gives the flattened
    scene's leaf order and every stored box, and the oracle's build.  The axes compared are not read out of
    the build (bvh.h keeps none): the library replays them from the same state with the reference's
    random_int, after checking that the build drew exactly one number per inner node, so they add a check
    of the draw count and of random_int, not of which node took which draw."""
    soa = refhdr_cases.builtin_scene(name).soa
    ref = oracle.RefScene(name)
    first, n, last0, la, lb, lo, hi = _flat_bvh(soa, rtlib)
    ((kind, n_mark, state),) = ref.rng_marks()
    assert (kind, n_mark) == (0, n)
    want = hdr.HdrScene(soa).bvh_build(first, n, state)
    assert np.array_equal(want["leaf_a"][last0:], la[last0:]) and np.array_equal(want["leaf_b"][last0:], lb[last0:])
    assert np.array_equal(want["axes"][:last0], la[:last0])  # an upper node's leaf_a slot holds its axis
    assert np.array_equal(_bits(want["lo"]), _bits(lo)) and np.array_equal(_bits(want["hi"]), _bits(hi))
    _same_build(oracle.RefScene.from_flat(soa).bvh_build(first, n, state), want, name)
    if name == "big1":
        assert np.array_equal(ref.bvh_axes(), want["axes"])


@pytest.mark.parametrize("n", range(3, 34))
def test_bvh_build_sizes(hdr, oracle, n):
    """3..33 primitives (the bvh:* group's range; bvh_node(int) lays out nothing smaller) of every kind,
    two of them coincident (a tie of the sort keys), over a shutter of [0.25, 0.75]: the oracle's build
    against bvh.h's."""
    s = flat_cases.look(flat_cases.FlatScene())
    mats = flat_cases.palette(s)
    g = np.random.default_rng(n)
    first = s.moving((-1.2, 1.3, 0.4), (-1.1, 1.5, 0.4), 0.0, 1.0, 0.45, mats[1])
    flat_cases.ground(s)
    for i in range(n - 2):
        c = np.array([g.uniform(-2, 2), g.uniform(0, 1), g.uniform(0, 3)])
        if i % 5 == 1:
            s.sphere(list(s.prims[-1].p)[:3] if s.prims[-1].type == 0 else c, 0.3, mats[0])
        elif i % 5 == 2:
            s.rect(("xy", "xz", "yz")[(i // 5) % 3], c[0] - 0.4, c[0] + 0.4, c[1] - 0.3, c[1] + 0.5, c[2], mats[3])
        elif i % 5 == 3:
            s.box(c - 0.3, c + 0.4, mats[5])
        elif i % 5 == 4:
            s.tri(c, c + (0.5, 0.0, 0.1), c + (0.1, 0.0, 0.6), mats[0])  # flat in y: the padded box
        else:
            s.sphere(c, 0.3, mats[2])
    s.world = [s.obj_list(first, n)]
    assert len(s.prims) - first == n
    state = oracle.xorwow_init(1984, n, 0)
    want = hdr.HdrScene(s.soa).bvh_build(first, n, state, 0.25, 0.75)
    _same_build(oracle.RefScene.from_flat(s.soa).bvh_build(first, n, state, 0.25, 0.75), want, f"n = {n}")
    last0 = (len(want["axes"]) + 1) // 2 - 1
    leaves = np.concatenate([want["leaf_a"][last0:], want["leaf_b"][last0:]])
    assert sorted(leaves[leaves >= 0]) == list(range(first, first + n))


# name: lookfrom, lookat, vfov, aspect, aperture, focus (scenes.h; vup (0, 1, 0), shutter [0, 1])
BUILTIN_CAMERAS = {
    "basic": ((0, 0, -3), (0, 0, 0), 40, 16 / 9, 0.0, 10.0), "first": ((-2, 2, -3), (0, 0, -1), 20, 16 / 9, 0.0, 10.0),
    "big1": ((13, 2, -3), (0, 0, 0), 20, 16 / 9, 0.1, 10.0), "two_spheres": ((13, 2, 3), (0, 0, 0), 20, 16 / 9, 0.1, 10.0),
    "two_perlin": ((13, 2, 3), (0, 0, 0), 20, 16 / 9, 0.1, 10.0), "cornell": ((278, 278, -800), (278, 278, 0), 40, 1.0, 0.0, 10.0),
    "cornell_smoke": ((278, 278, -800), (278, 278, 0), 40, 1.0, 0.0, 10.0), "triangle": ((0, 0, -3), (0, 0, 0), 40, 16 / 9, 0.0, 10.0),
    "triangles": ((0, 0, -3), (0, 0, 0), 40, 16 / 9, 0.0, 10.0), "earth": ((13, 0, 3), (0, 0, 0), 20, 16 / 9, 0.1, 10.0),
    "door": ((-3, 4, -5), (0, 1, 0), 20, 16 / 9, 0.0, 10.0), "final": ((478, 278, -600), (278, 278, 0), 40, 16 / 9, 0.0, 10.0),
}


def _camera_floats(c):
    return np.array([*c.origin, *c.lower_left, *c.horizontal, *c.vertical, *c.u, *c.v, *c.w, c.lens_radius, c.time0, c.time1],
                    np.float32)


@pytest.mark.parametrize("name", refhdr_cases.BUILTIN)
def test_builtin_camera(hdr, oracle, name):
    """camera.h's constructor (its tan, unit vectors and corner) on the scene's parameters gives the
    flattened scene's camera and the oracle's, bit for bit."""
    frm, at, vfov, aspect, aperture, focus = BUILTIN_CAMERAS[name]
    want = hdr.camera_build(frm, at, vfov, np.float32(aspect), aperture, focus)
    got = _camera_floats(refhdr_cases.builtin_scene(name).soa.camera)
    assert np.array_equal(_bits(got), _bits(want)), f"{name}: rt_scene.cpp's camera, floats {np.argwhere(_bits(got) != _bits(want)).ravel()}"
    got = oracle.RefScene(name, **refhdr_cases.builtin_assets(name)[1]).camera()
    assert np.array_equal(_bits(got), _bits(want)), f"{name}: the oracle's camera, floats {np.argwhere(_bits(got) != _bits(want)).ravel()}"


@pytest.mark.parametrize("vfov", [1.0, 20.0, 38.0, 90.0, 170.0])
@pytest.mark.parametrize("frm,at", [((0.4, 1.6, -5.0), (0, 0.1, 0.8)), ((800.0, 3200.0, -9440.0), (0, 0.1, 0.8)),
                                    ((1e-3, 2e-3, -5e-3), (0, 0, 0)), ((0, 0, 3), (0, 0, -1))])
def test_camera_constructor(hdr, oracle, frm, at, vfov):
    """The oracle's camera constructor against camera.h's away from the built-in scenes' parameters."""
    for aperture, focus in ((0.0, 10.0), (6.0, 0.5)):
        ref = oracle.RefScene("cornell" if vfov == 90.0 else "basic")  # aspect 1 and 16/9
        ref.set_camera(frm, at, vfov, aperture, focus)
        want = hdr.camera_build(frm, at, vfov, np.float32(ref.aspect), aperture, focus)
        assert np.array_equal(_bits(ref.camera()), _bits(want)), (frm, at, vfov, aperture, focus)


# scene: the angles of its rotate_y instances and the densities of its media, in object order (scenes.h; final: DESIGN.md)
BUILTIN_INSTANCES = {"cornell": ([15.0, -18.0], []), "cornell_smoke": ([15.0, -18.0], [0.01, 0.01]),
                     "final": ([15.0, -30.0], [0.2, 0.0001])}


@pytest.mark.parametrize("name", list(BUILTIN_INSTANCES))
def test_builtin_instance_constants(hdr, rtlib, name):
    """rotate_y's constructor (degrees_to_radians, sin, cos; hittable.h:77-81) and constant_medium's
    (-1/d, constant_medium.h:15-16) give the sin / cos and -1/density the flattened scene stores.  The
    oracle's own constructors are held to the same values by test_builtin_scene's renders."""
    soa = refhdr_cases.builtin_scene(name).soa
    objs = [soa.objects[k] for k in range(soa.n_objects)]
    angles, densities = BUILTIN_INSTANCES[name]
    rot = [o for o in objs if o.kind == rtlib.OBJ_XFORM and o.b & 2]
    med = [o for o in objs if o.kind == rtlib.OBJ_MEDIUM]
    assert len(rot) == len(angles) and len(med) == len(densities)
    for o, a in zip(rot, angles):
        assert np.array_equal(_bits(np.array([o.f[3], o.f[4]], np.float32)), _bits(hdr.instance_consts(a)[:2])), (name, a)
    for o, d in zip(med, densities):
        assert np.array_equal(_bits(np.array([o.f[0]], np.float32)), _bits(hdr.instance_consts(0.0, d)[2:])), (name, d)


@pytest.mark.parametrize("name", ["two_perlin", "final"])
def test_perlin_tables(hdr, oracle, name):
    """perlin.h's constructor from the scene RNG state at each noise texture's construction gives the
    flattened scene's tables, in construction order."""
    soa = refhdr_cases.builtin_scene(name).soa
    marks = [m for m in oracle.RefScene(name, **refhdr_cases.builtin_assets(name)[1]).rng_marks() if m[0] == 1]
    assert len(marks) == soa.n_perlins > 0
    buf = (ctypes.c_char * (soa.n_perlins * PERLIN_DTYPE.itemsize)).from_address(soa.perlins)
    tabs = np.frombuffer(buf, PERLIN_DTYPE)
    for k, (_, _, state) in enumerate(marks):
        want = hdr.perlin_build(state)
        p = tabs[k]
        assert np.array_equal(_bits(want["ranvec"]), _bits(p["ranvec"])), (name, k)
        for key in ("perm_x", "perm_y", "perm_z"):
            assert np.array_equal(want[key], p[key]), (name, k, key)


# ---------------------------------------------------------------- the record (runs everywhere)
@pytest.mark.parametrize("key", refhdr_cases.RECORDED)
def test_oracle_matches_the_record(oracle, key):
    """The oracle against what the reference's headers wrote down (tests/golden/make_refhdr_golden.py)."""
    rec = np.load(refhdr_cases.GOLDEN)
    e = refhdr_cases.recorded_entry(key)
    ref = oracle.RefScene.from_flat(e.scene.soa)
    segs = np.zeros((H, W), np.int64)
    for f in range(NFB):
        fb, _, sp = ref.render(W, H, SPP, f, e.depth, REF, seg_per_pixel=True)
        segs += sp.reshape(H, W)
        d = first_difference(fb.reshape(H, W, 3), rec[f"{refhdr_cases.key_name(key)}_fb{f}"].view(np.float32))
        assert d is None, f"{key} fb {f}: {d[0]} px differ, first at {d[1]}"
    d = np.argwhere(segs != rec[f"{refhdr_cases.key_name(key)}_segments"])
    assert not len(d), f"{key}: segments of {len(d)} px differ, first at {d[0]}"


def test_record_is_small():
    assert os.path.getsize(refhdr_cases.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(refhdr_cases.GOLDEN), "ref_images.npz"))


def test_record_is_current(hdr):
    """Where the reference is, the committed record is what its headers give now."""
    rec = np.load(refhdr_cases.GOLDEN)
    for key in refhdr_cases.RECORDED:
        e = refhdr_cases.recorded_entry(key)
        hs = hdr.HdrScene(e.scene.soa)
        segs = np.zeros((H, W), np.int32)
        for f in range(NFB):
            fb, sg = hs.render(W, H, SPP, f, e.depth, REF)
            segs += sg
            assert np.array_equal(_bits(fb), rec[f"{refhdr_cases.key_name(key)}_fb{f}"]), (key, f)
        assert np.array_equal(segs, rec[f"{refhdr_cases.key_name(key)}_segments"]), key
