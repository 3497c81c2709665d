"""The written scenes tests/test_flat_gpu.py renders and tests/test_flat_cpu.py checks as inputs.

A case is a FlatScene (flat_scenes.py) with the launch shape of every case -- 40x24, 4 samples per
pixel (probe-eligible), 2 frame buffers -- the kernel family its world shape must land in, and, where
it is built around a branch, `evidence`: a check on the oracle alone that the branch is reached.
Cases are grouped by the data-dependent branch of rt_kernels.hip they exist for ("Written
scenes").
"""
from __future__ import annotations

import functools
import math
import os
import re
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

import raytracing_gpu_amd as rt
from flat_scenes import FlatScene, F32

W, H, SPP, NFB = 40, 24, 4, 2
REF, PIX = 0, 1
STEP, RENDER = "render_step_kernel<", "render_kernel<"
F_LDS, F_STEP, F_QLDS, F_MERGE = 1 << 13, 1 << 14, 1 << 16, 1 << 17


@dataclass
class Case:
    build: Callable[[], FlatScene]
    family: str | None = None        # prefix of last_render_kernel() for the default launch
    depth: int = 50
    per_pixel: bool = False          # also rendered with RT_CAM_PER_PIXEL
    evidence: Callable | None = None  # evidence(case, oracle result, oracle module)
    options: dict = field(default_factory=dict)   # context options for the whole case (upload time)
    fallbacks: bool = False          # the stats twin must report fallbacks > 0
    merged: bool = False             # a list world the merged search takes (the global-memory launch has F_MERGE)
    mask_has: int = 0                # variant bits the default launch's kernel must have
    mask_lacks: int = 0              # ... and must not have
    scene: FlatScene | None = None


@dataclass
class Result:
    fbs: list
    counters: dict
    segs: np.ndarray


CASES: dict[str, Case] = {}


def case(name, **kw):
    def deco(fn):
        CASES[name] = Case(build=fn, **kw)
        return fn
    return deco


def all_case_ids() -> list[str]:
    return list(CASES)


def group(prefix: str) -> list[str]:
    return [k for k in CASES if k.startswith(prefix + ":")]


def get(name: str) -> Case:
    c = CASES[name]
    if c.scene is None:
        c.scene = c.build()
    return c


@functools.lru_cache(maxsize=None)
def _render(name: str, cam: int) -> Result:
    from oracle import ref_cpu

    c = get(name)
    return render_scene(ref_cpu, c.scene, cam, c.depth)


def render_scene(oracle, scene: FlatScene, cam: int = REF, depth: int = 50) -> Result:
    ref = oracle.RefScene.from_flat(scene.soa)
    fbs, tot, segs = [], None, np.zeros(W * H, np.int64)
    for f in range(NFB):
        fb, c, sp = ref.render(W, H, SPP, f, depth, cam, seg_per_pixel=True)
        fbs.append(fb.reshape(H, W, 3))
        tot = c if tot is None else {k: tot[k] + c[k] for k in tot}
        segs += sp
    return Result(fbs, tot, segs.reshape(H, W))


def oracle_render(oracle, name: str, cam: int = REF) -> Result:
    """The oracle's frame buffers and counters of a case (computed once per case and camera mode)."""
    return _render(name, cam)


def source_constants() -> dict:
    """kLdsBudget, kStackDepth and kPlanePairs as rt_kernels.hip defines them, and the schedule's kOrderTile and
    kProbeRadius (tests/sched_ref.py)."""
    src = open(os.path.join(os.path.dirname(rt.__file__), "csrc", "rt_kernels.hip")).read()
    out = {}
    for k in ("kLdsBudget", "kStackDepth", "kPlanePairs", "kOrderTile", "kProbeRadius"):
        expr = re.search(r"constexpr int %s = ([0-9* ]+);" % k, src).group(1)
        out[k] = math.prod(int(x) for x in expr.split("*"))
    return out


# ---------------------------------------------------------------- evidence helpers
def differs_from(twin: Callable[[], FlatScene], what: str):
    """The case's pixels differ from its twin's (the same scene without the feature): the feature shows."""
    def ev(c, r, oracle):
        t = render_scene(oracle, twin(), REF, c.depth)
        same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r.fbs, t.fbs))
        assert not same, what
    return ev


def more_prim_tests_than(twin: Callable[[], FlatScene], what: str):
    def ev(c, r, oracle):
        t = render_scene(oracle, twin(), REF, c.depth)
        assert r.counters["prim_tests"] > t.counters["prim_tests"], what
    return ev


def bvh_is_tested(c, r, oracle):
    assert r.counters["node_tests"] > 0 and r.counters["prim_tests"] > 0


# ---------------------------------------------------------------- building blocks
def palette(s: FlatScene, checker: bool = True) -> list[int]:
    """Six materials.  checker=False: without the checker texture, which no merged-search variant covers
    (the merged search is compiled for the feature set of everything but the checker)."""
    ck = s.checker(s.solid((0.2, 0.3, 0.1)), s.solid((0.9, 0.9, 0.9))) if checker else s.noise(3.0, 9)
    return [s.lambertian((0.8, 0.3, 0.3)), s.metal((0.8, 0.8, 0.8), 0.1), s.dielectric(1.5),
            s.lambertian((0.3, 0.4, 0.8)), s.lambertian(ck), s.metal((0.9, 0.7, 0.3), 0.0)]


def grid_spheres(s: FlatScene, n: int, mats: list[int], seed: int = 0, r: float = 0.38, y: float = 0.0) -> list[int]:
    g = np.random.default_rng(1000 + seed)
    cols = max(1, math.ceil(math.sqrt(n * 1.6)))
    ids = []
    for i in range(n):
        x = (i % cols - (cols - 1) / 2) * 0.95 + g.uniform(-0.1, 0.1)
        z = (i // cols) * 0.95 + g.uniform(-0.1, 0.1)
        ids.append(s.sphere((x, y + g.uniform(0.0, 0.3), z), r, mats[i % len(mats)]))
    return ids


def ground(s: FlatScene, mat: int | None = None, y: float = -0.38) -> int:
    return s.sphere((0, y - 1000.0, 0), 1000.0, s.lambertian((0.5, 0.5, 0.5)) if mat is None else mat)


def look(s: FlatScene, **kw) -> FlatScene:
    s.camera((0.4, 1.6, -5.0), (0, 0.1, 0.8), 38.0, **kw)
    return s


def garden(n: int, seed: int = 0, in_list: bool = False, boxes=None, pad=None, order=None) -> FlatScene:
    """A BVH of n primitives (n - 1 spheres and the ground) as the whole world, or after a primitive
    entry of a list world."""
    s = look(FlatScene())
    ids = grid_spheres(s, n - 1, palette(s, checker=not in_list), seed) + [ground(s)]
    if order is not None:
        ids = [ids[k] for k in order(len(ids))]
    b = s.bvh(ids, boxes=boxes(s, ids) if callable(boxes) else boxes, pad=pad(n) if callable(pad) else pad)
    if in_list:  # (a moving sphere and a rect: with them the scene's features take the merged-search variant)
        s.world.append(s.obj_prim(s.moving((-1.2, 1.3, 0.4), (-1.1, 1.5, 0.4), 0.0, 1.0, 0.45, s.metal((0.8, 0.6, 0.2), 0.3))))
        s.world.append(s.obj_prim(s.rect("xy", -2.5, -1.0, 0.2, 1.6, 3.0, s.lambertian((0.7, 0.7, 0.2)))))
    s.world.append(b)
    return s


# ---------------------------------------------------------------- group: BVH sizes
for _n in (3, 4, 5, 6, 7, 8, 9, 16, 17, 33):
    case(f"bvh:{_n}_world", family=STEP, evidence=bvh_is_tested, per_pixel=_n == 5)(functools.partial(garden, _n, _n))
    case(f"bvh:{_n}_list", family=RENDER, evidence=bvh_is_tested, per_pixel=_n == 6,
         merged=True)(functools.partial(garden, _n, _n, True))


# ---------------------------------------------------------------- group: stored boxes
def _loose_pad(n):
    rows = max(2, (n - 1).bit_length())
    return np.random.default_rng(7).uniform(0.0, 0.6, ((1 << rows) - 1, 3))


def _shrunk(s, ids):
    """Node 1 (mid level of a 3-row tree) shrunk to 70 % about its centre: its children's boxes poke out."""
    lo = np.min([s.prim_box(i)[0] for i in ids[:len(ids) // 2]], axis=0)
    hi = np.max([s.prim_box(i)[1] for i in ids[:len(ids) // 2]], axis=0)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    return {1: (c - 0.7 * h, c + 0.7 * h)}


def _leaf_cut(s, ids):
    """The first last-row node's box keeps only the lower left part of its primitives' box."""
    rows = max(2, (len(ids) - 1).bit_length())
    k = (1 << (rows - 1)) - 1
    m = ids[:len(ids) // (1 << (rows - 1))] or ids[:1]
    lo = np.min([s.prim_box(i)[0] for i in m], axis=0)
    hi = np.max([s.prim_box(i)[1] for i in m], axis=0)
    return {k: (lo, lo + 0.55 * (hi - lo))}


def _root_hides(s, ids):
    """The root box ends at x = 0.3: what lies right of it is not rendered."""
    return {0: ((-1100, -2100, -1100), (0.3, 1100, 1100))}


_plain9 = functools.partial(garden, 9, 9)
case("boxes:loosened", family=STEP, evidence=more_prim_tests_than(_plain9, "looser boxes test more primitives"))(
    functools.partial(garden, 9, 9, pad=_loose_pad))
case("boxes:shrunk_mid", family=STEP, per_pixel=True,
     evidence=differs_from(_plain9, "the shrunk box hides nothing"))(functools.partial(garden, 9, 9, boxes=_shrunk))
case("boxes:shrunk_mid_list", family=RENDER, merged=True,
     evidence=differs_from(functools.partial(garden, 9, 9, True), "the shrunk box hides nothing"))(
    functools.partial(garden, 9, 9, True, boxes=_shrunk))
case("boxes:leaf_cuts_primitive", family=STEP,
     evidence=differs_from(_plain9, "the cut leaf box hides nothing"))(functools.partial(garden, 9, 9, boxes=_leaf_cut))
case("boxes:root_hides", family=STEP,
     evidence=differs_from(_plain9, "the root box hides nothing"))(functools.partial(garden, 9, 9, boxes=_root_hides))
case("boxes:root_hides_list", family=RENDER, merged=True,
     evidence=differs_from(functools.partial(garden, 9, 9, True), "the root box hides nothing"))(
    functools.partial(garden, 9, 9, True, boxes=_root_hides))


# ---------------------------------------------------------------- group: deep traversal tree
def chain(n: int = 72, growth: float = 1.7) -> FlatScene:
    """Spheres along the view axis, centre distance growing geometrically, radius / distance growing from
    0.12 to 0.36 over the first dozen.  The SAH builder of the traversal tree then splits a few of the
    largest off at every level (both children inner nodes: a leaf child is tested at once and never
    pushed), and a ray from the origin enters both children of every level, the near one first: the far
    ones pile up on the 16-entry stack (about 21 deep here; the largest coordinate is 1e15).  The pushes
    that no longer fit are the far children of the deepest levels, spheres 5 to 15, and a ray between
    the cones of sphere 4 and sphere 15 misses the nearer spheres and hits one of exactly those first:
    without the fallback to the exact visit set it would get a sphere behind them."""
    s = FlatScene()
    s.camera((0, 0, 0), (0, 0, 1), 34.0, focus=1.0)
    mats = palette(s)
    ids = [s.sphere((0.0, 0.0, 0.05 * growth ** i), min(0.12 + 0.02 * i, 0.36) * 0.05 * growth ** i,
                    mats[(2, 0, 2, 1, 2, 3)[i % 6]]) for i in range(n)]
    s.world.append(s.bvh(ids))
    s.world.append(s.obj_prim(s.sphere((0, -3e6, 0), 2.99e6, mats[4])))
    return s


case("deep:chain", family=STEP, fallbacks=True, per_pixel=True, evidence=bvh_is_tested)(chain)


# ---------------------------------------------------------------- group: time
def movers(t0c: float, t1c: float, in_list: bool = False) -> FlatScene:
    """Moving spheres with (t0, dt) = (2, 0.5) beside ones with (0, 1), under a camera shutter [t0c, t1c]."""
    s = look(FlatScene(), t0=t0c, t1=t1c)
    mats = palette(s)
    ids = []
    for i in range(8):
        c0 = np.array([(i % 4 - 1.5) * 1.0, 0.1 * (i % 3), (i // 4) * 1.2])
        c1 = c0 + np.array([0.0, 0.5 + 0.1 * i, 0.2 * (i % 2)])
        ids.append(s.moving(c0, c1, 2.0, 2.5, 0.4, mats[i % 5]) if i % 2 else s.moving(c0, c1, 0.0, 1.0, 0.4, mats[i % 5]))
    ids += [s.sphere((0.2, 0.4, 2.6), 0.5, mats[5]), ground(s)]
    b = s.bvh(ids)
    if in_list:
        s.world.append(s.obj_prim(s.moving((-1.5, 1.4, 0.5), (-1.2, 1.8, 0.5), 2.0, 2.5, 0.35, mats[0])))
    s.world.append(b)
    return s


def _still(t0c, t1c):
    def twin():
        s = movers(t0c, t1c)
        for p in s.prims:
            if p.type == rt.PRIM_MOVING_SPHERE:
                p.p[4] = p.p[5] = p.p[6] = 0.0
        return s
    return twin


def _has_non_unit_movers(c, r, oracle):
    ts = {(p.p[7], p.p[8]) for p in c.scene.prims if p.type == rt.PRIM_MOVING_SPHERE}
    assert (0.0, 1.0) in ts and (2.0, 0.5) in ts


def _both(*evs):
    def ev(c, r, oracle):
        for e in evs:
            e(c, r, oracle)
    return ev


case("time:shutter_quarter", family=STEP, per_pixel=True,
     evidence=_both(_has_non_unit_movers, differs_from(_still(0.25, 0.75), "the spheres do not move")))(
    functools.partial(movers, 0.25, 0.75))
case("time:shutter_point", family=STEP,
     evidence=_both(_has_non_unit_movers, differs_from(_still(0.5, 0.5), "the spheres do not move")))(
    functools.partial(movers, 0.5, 0.5))
case("time:shutter_quarter_list", family=RENDER, evidence=_has_non_unit_movers)(functools.partial(movers, 0.25, 0.75, True))


def media_limits(which: str) -> FlatScene:
    """List world with a sphere-bounded medium that is not inert by medium_inert's limits: a moving
    boundary with a tiny time span (its centre runs off by more than 1e6 within |time| < 1024), or a
    boundary with a coordinate of 1e6 and more."""
    s = look(FlatScene(), t0=0.0, t1=0.002)
    mats = palette(s, checker=False)  # (with the moving sphere and the rect: the merged search's feature set, so
    for i in range(4):                # a medium taken for inert would show as F_MERGE on the global-memory launch)
        s.world.append(s.obj_prim(s.sphere(((i - 1.5) * 1.0, 0.1, 0.5 * (i % 2)), 0.42, mats[i])))
    s.world.append(s.obj_prim(s.moving((-2.2, 1.2, 1.0), (-2.2, 1.3, 1.0), 0.0, 1.0, 0.3, mats[0])))
    s.world.append(s.obj_prim(s.rect("xy", -3.0, 3.0, -0.4, 2.5, 3.5, mats[3])))
    glass, fog = s.dielectric(1.5), s.isotropic((0.6, 0.7, 0.9))
    if which == "tiny_dt":
        b = s.moving((0.3, 0.5, 1.0), (0.3, 2.0, 1.0), 0.0, 0.001, 0.9, glass)  # d = 1.5, dt = 1e-3
    else:
        b = s.sphere((1.0e6 + 1.5, 0.0, 0.0), 1.0e6, glass)  # its surface crosses the view at x = 1.5
    s.world.append(s.medium(s.obj_prim(b), 0.4, fog))
    s.world.append(s.obj_prim(ground(s)))
    return s


def _not_inert(c, r, oracle):
    s = c.scene
    m = next(o for o in s.objects if o.kind == rt.OBJ_MEDIUM)
    p = s.prims[s.objects[m.a].a]
    if p.type == rt.PRIM_SPHERE:
        assert max(abs(p.p[k]) for k in range(4)) >= 1e6
    else:
        assert (1024.0 + abs(p.p[7])) / abs(p.p[8]) * max(abs(p.p[k]) for k in (4, 5, 6)) >= 1e6


def _boundary_is_hit(c, r, oracle):
    """The medium's boundary lies where rays go: with the boundary sphere as an opaque entry in the
    medium's place the picture changes (the oracle does not count a medium's boundary queries, and a
    sphere-bounded medium never scatters, H1, so the medium itself leaves no trace: same segments)."""
    def twin(opaque):
        s = media_limits("tiny_dt" if "tiny" in c.build.args[0] else "far")
        k = next(k for k, o in enumerate(s.objects) if o.kind == rt.OBJ_MEDIUM)
        w = s.world.index(k)
        if opaque:
            s.prims[s.objects[s.objects[k].a].a].material = s.lambertian((0.9, 0.1, 0.9))
            s.world[w] = s.objects[k].a
        else:
            del s.world[w]
        return render_scene(oracle, s, REF, c.depth)
    without, opaque = twin(False), twin(True)
    assert without.counters["segments"] == r.counters["segments"]
    assert not all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(without.fbs, opaque.fbs)), \
        "no ray reaches the boundary"


case("time:medium_tiny_dt", family=RENDER, evidence=_both(_not_inert, _boundary_is_hit))(functools.partial(media_limits, "tiny_dt"))
case("time:medium_far_coordinate", family=RENDER, evidence=_both(_not_inert, _boundary_is_hit), per_pixel=True)(
    functools.partial(media_limits, "far"))


# ---------------------------------------------------------------- group: world shapes
def _small_bvh(s, mats, x0=0.0, z0=0.0, n=4, seed=0):
    g = np.random.default_rng(50 + seed)
    return s.bvh([s.sphere((x0 + (i % 2) * 0.8 + g.uniform(-0.1, 0.1), 0.1 + 0.75 * (i // 4), z0 + ((i // 2) % 2) * 0.8), 0.36,
                           mats[(i + seed) % len(mats)]) for i in range(n)])


def _extra_prims(s, mats, n, mixed=False):
    """n primitive entries on a circle; mixed: the first is a moving sphere and the second a rect."""
    out = []
    for i in range(n):
        a = 2 * math.pi * i / max(n, 1)
        c = np.array([2.3 * math.cos(a), 0.1 + 0.2 * (i % 3), 1.2 + 2.0 * math.sin(a)])
        if mixed and i == 0:
            out.append(s.obj_prim(s.moving(c, c + (0.0, 0.4, 0.1), 0.0, 1.0, 0.3, mats[0])))
        elif mixed and i == 1:
            out.append(s.obj_prim(s.rect("xy", c[0] - 0.4, c[0] + 0.4, -0.3, 0.8, c[2], mats[1])))
        else:
            out.append(s.obj_prim(s.sphere(c, 0.3, mats[i % len(mats)])))
    return out


MERGED_SHAPES = ("bvh_8_prims", "two_bvhs", "instanced_bvhs", "entries_9", "entries_17")


def world_shape(kind: str) -> FlatScene:
    s = look(FlatScene())
    merged = kind in MERGED_SHAPES
    mats = palette(s, checker=not merged)
    gr = s.obj_prim(ground(s))
    fog = s.isotropic((0.9, 0.5, 0.3))

    def box_rects(x0, y0, z0, x1, y1, z1, m):  # box.h's six sides as a list of rects
        first = s.rect("xy", x0, x1, y0, y1, z1, m)
        s.rect("xy", x0, x1, y0, y1, z0, m)
        s.rect("xz", x0, x1, z0, z1, y1, m)
        s.rect("xz", x0, x1, z0, z1, y0, m)
        s.rect("yz", y0, y1, z0, z1, x1, m)
        s.rect("yz", y0, y1, z0, z1, x0, m)
        return first

    if kind == "one_prim":
        s.world = [s.obj_prim(s.sphere((0, 0, 2), 3.0, mats[4]))]
        s.camera((0, 0.5, -4), (0, 0, 2), 40.0)
    elif kind == "one_bvh":
        s.world = [s.bvh([ground(s)] + [s.sphere((i - 1.5, 0.1, 0.6 * (i % 2)), 0.4, mats[i]) for i in range(4)])]
    elif kind in ("bvh_7_prims", "bvh_8_prims"):
        k = 7 if kind == "bvh_7_prims" else 8
        s.world = [_small_bvh(s, mats, -0.4, 0.4, 5)] + _extra_prims(s, mats, k - 1, merged) + [gr]
    elif kind == "bvh_then_list":
        s.world = [_small_bvh(s, mats, -1.6, 0.2, 4), s.obj_list(box_rects(0.3, -0.3, 0.2, 1.5, 0.9, 1.4, mats[0]), 6), gr]
    elif kind == "two_bvhs":
        s.world = [_small_bvh(s, mats, -1.7, 0.2, 5), _small_bvh(s, mats, 0.5, 0.6, 6, 1)] + _extra_prims(s, mats, 2, True) + [gr]
    elif kind == "instanced_bvhs":
        a, b = _small_bvh(s, mats, -0.4, 0.0, 4), _small_bvh(s, mats, -0.4, 0.0, 5, 2)
        s.world = [s.xform(a, 25.0, (-1.6, 0.0, 0.5), flags=1), s.xform(b, 30.0, (0.3, 0.2, 0.4), flags=2),
                   s.xform(a, -20.0, (1.5, 0.3, 1.6), flags=3)] + _extra_prims(s, mats, 2, True) + [gr]
    elif kind == "medium_over_list":
        s.world = _extra_prims(s, mats, 3) + [gr, s.medium(s.obj_list(box_rects(-1.0, -0.3, 0.0, 1.0, 1.2, 1.6, mats[0]), 6), 1.5, fog)]
    elif kind == "medium_over_xform":
        bx = s.obj_prim(s.box((-0.9, -0.3, -0.8), (0.9, 1.2, 0.8), mats[0]))
        s.world = _extra_prims(s, mats, 3) + [gr, s.medium(s.xform(bx, 20.0, (0.1, 0.0, 0.9)), 1.5, fog)]
    elif kind == "medium_over_bvh":
        first = box_rects(-1.0, -0.3, 0.0, 1.0, 1.2, 1.6, mats[0])
        s.world = _extra_prims(s, mats, 3) + [gr, s.medium(s.bvh(range(first, first + 6)), 1.5, fog)]
    elif kind == "medium_not_last":
        bx = s.obj_prim(s.box((-0.9, -0.3, 0.0), (0.9, 1.2, 1.6), mats[0]))
        s.world = [s.medium(bx, 1.5, fog)] + _extra_prims(s, mats, 3) + [_small_bvh(s, mats, -0.4, 2.0, 4), gr]
    elif kind in ("entries_9", "entries_17"):
        s.world = _extra_prims(s, mats, int(kind.split("_")[1]) - 1, True) + [gr]
    return s


def _thin(kind):
    def twin():
        s = world_shape(kind)
        for o in s.objects:
            if o.kind == rt.OBJ_MEDIUM:
                o.f[0] = -1e9  # -1/density of an all but empty medium: the draw is made, nothing scatters
        return s
    return twin


_scatters = {k: differs_from(_thin(k), "the medium never scatters") for k in
             ("medium_over_list", "medium_over_xform", "medium_over_bvh", "medium_not_last")}
for _k, _fam in (("one_prim", RENDER), ("one_bvh", STEP), ("bvh_7_prims", STEP), ("bvh_8_prims", RENDER),
                 ("bvh_then_list", RENDER), ("two_bvhs", RENDER), ("instanced_bvhs", RENDER), ("medium_over_list", RENDER),
                 ("medium_over_xform", RENDER), ("medium_over_bvh", RENDER), ("medium_not_last", RENDER),
                 ("entries_9", RENDER), ("entries_17", RENDER)):
    _merged = _k in MERGED_SHAPES
    case(f"world:{_k}", family=_fam, merged=_merged, mask_has=F_STEP if _fam == STEP else 0,
         mask_lacks=0 if _fam == STEP else F_STEP, evidence=_scatters.get(_k),
         per_pixel=_k in ("instanced_bvhs", "medium_over_bvh"))(functools.partial(world_shape, _k))


# ---------------------------------------------------------------- group: LDS fit
def lds_step_bytes(n_ref_nodes, n_prims, n_mats, n_texs, k) -> int:
    """rt_render's fit test of the stepwise kernel's LDS image (use_lds): staged float4s plus stacks."""
    slots = n_ref_nodes + 2 * k["kPlanePairs"]
    return (2 * slots + 3 * n_prims + (n_prims + 1) // 2 + n_mats + 2 * n_texs) * 16 + 1024 * k["kStackDepth"] * 2


def lds_fit_spheres(over: bool) -> FlatScene:
    """40 (fits) or 41 (does not) spheres under the world BVH, with as many unused solid textures as put
    the 40-sphere scene's LDS image at most 3.5 float4s below kLdsBudget."""
    k = source_constants()
    n = 41 if over else 40
    s = look(FlatScene())
    mats = palette(s)
    ids = grid_spheres(s, n - 1, mats, 3) + [ground(s)]
    s.world.append(s.bvh(ids))
    fits = lambda npr, nt: lds_step_bytes(63, npr, len(s.mats), nt, k) <= k["kLdsBudget"]
    while fits(40, len(s.texs) + 1):
        s.solid((0.1, 0.2, 0.3))
    assert fits(40, len(s.texs)) and not fits(41, len(s.texs)) and len(s.nodes) == 63
    return s


def qlds_bytes(n_leaves, n_mats, n_texs, n_images, k) -> int:
    """rt_scene_upload's fit test of the quantized traversal tree: pair records, stacks and tables."""
    return (n_leaves - 1) * 24 + 1024 * k["kStackDepth"] * 2 + 16 * (n_mats + 2 * n_texs + n_images) + 16


def lds_fit_triangles(over: bool) -> FlatScene:
    """As many distinct triangles under the world BVH as the quantized tree's fit test takes (about 120,
    next to unused solid textures that fill the tables), or one more."""
    k = source_constants()
    s = look(FlatScene())
    mats = [s.lambertian(c) for c in ((0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8), (0.8, 0.8, 0.3), (0.6, 0.6, 0.6),
                                      (0.8, 0.4, 0.7))]  # (the stepwise mesh variant: triangles, spheres, images)
    gr = ground(s)
    fits = lambda nl, nt: qlds_bytes(nl, len(s.mats), nt, 0, k) <= k["kLdsBudget"]
    while fits(120, len(s.texs) + 1):
        s.solid((0.1, 0.2, 0.3))
    n = 120
    while fits(n + 1, len(s.texs)):
        n += 1
    assert 120 <= n <= 121 and fits(n, len(s.texs)) and not fits(n + 1, len(s.texs))
    n += 1 if over else 0
    ids = []
    for i in range(n):
        x, z = (i % 12 - 6) * 0.45, (i // 12) * 0.45 - 0.5
        yy = -0.3 + 0.25 * ((i * 7) % 5)
        ids.append(s.tri((x, yy, z), (x + 0.42, yy + 0.1, z + 0.05), (x + 0.1, yy + 0.5, z + 0.3), mats[i % 6]))
    s.world.append(s.bvh(ids))
    s.world.append(s.obj_prim(gr))
    return s


case("lds:spheres_under", family=STEP, mask_has=F_LDS, per_pixel=True)(functools.partial(lds_fit_spheres, False))
case("lds:spheres_over", family=STEP, mask_lacks=F_LDS)(functools.partial(lds_fit_spheres, True))
case("lds:triangles_under", family=STEP, mask_has=F_QLDS)(functools.partial(lds_fit_triangles, False))
case("lds:triangles_over", family=STEP, mask_lacks=F_QLDS)(functools.partial(lds_fit_triangles, True))


# ---------------------------------------------------------------- group: camera
def camera_case(kind: str) -> FlatScene:
    sc = {"scale_small": 1e-3, "scale_large": 1e3}.get(kind, 1.0)
    s = FlatScene()
    mats = palette(s)
    ids = [s.sphere((sc * (i % 3 - 1) * 1.1, sc * 0.1 * i, sc * (i // 3) * 1.1), sc * 0.45, mats[i % 6]) for i in range(6)]
    ids.append(s.sphere((0, sc * -1000.45, 0), sc * 1000.0, mats[4]))
    frm, at, vfov, ap, focus = (0.4 * sc, 1.6 * sc, -5.0 * sc), (0, 0.1 * sc, 0.8 * sc), 38.0, 0.0, 10.0 * sc
    if kind == "inside_glass":
        ids.append(s.sphere(frm, 1.2, mats[2]))
    elif kind == "lens_wider_than_focus":
        ap, focus = 6.0, 0.5  # lens radius 3 against a focus distance of 0.5
    elif kind == "vfov_1":
        vfov, at = 1.0, (0, 0.1, 0.0)
    elif kind == "vfov_170":
        vfov = 170.0
    elif kind.startswith("far_camera"):  # 1e4 from the unit scene: 22 000 radii, refused by rt_scene_validate
        frm, vfov = (800.0, 3200.0, -9440.0), 0.03
    elif kind.startswith("far_400r"):  # 180 from it: 400 radii of its spheres, below the limit of 512
        frm, vfov = (14.4, 57.6, -169.9), 1.6
    s.camera(frm, at, vfov, ap, focus)
    b = s.bvh(ids)
    if kind.endswith("_instance"):
        b = s.xform(b, 20.0, (0.3, 0.0, 0.2))
    elif kind.endswith("_medium_boundary"):
        b = s.medium(b, 0.5, s.isotropic((0.8, 0.8, 0.9)))
    s.world.append(b)
    if kind == "inside_medium":
        s.world.append(s.medium(s.obj_prim(s.box((-3, -0.4, -6), (3, 3, 3), mats[0])), 0.15, s.isotropic((0.8, 0.8, 0.9))))
    return s


def _fog_scatters(c, r, oracle):
    def twin():
        s = camera_case("inside_medium")
        for o in s.objects:
            if o.kind == rt.OBJ_MEDIUM:
                o.f[0] = -1e9
        return s
    differs_from(twin, "the medium around the camera never scatters")(c, r, oracle)


for _k in ("inside_glass", "inside_medium", "lens_wider_than_focus", "vfov_1", "vfov_170", "far_400r", "far_400r_instance",
           "scale_small", "scale_large"):
    case(f"camera:{_k}", family=RENDER if _k in ("inside_medium", "far_400r_instance") else STEP,
         evidence=_fog_scatters if _k == "inside_medium" else None,
         per_pixel=_k in ("lens_wider_than_focus", "inside_glass"))(functools.partial(camera_case, _k))
# camera:far_camera itself (the issue's "camera at 1e4 from a unit scene") is outside what the header
# promises: tests/test_flat_cpu.py has its refusal, as a world BVH, under an instance and as a boundary.


# ---------------------------------------------------------------- group: shading matrix
TEXTURES = ("solid", "checker_solid_noise", "checker_image_solid", "noise", "turbulence_1", "turbulence_7", "marble",
            "image_1x1x3", "image_13x7x3", "image_64x64x3", "image_1x1x1", "image_13x7x1", "image_64x64x1", "image_none")


def make_texture(s: FlatScene, name: str) -> int:
    from raytracing_gpu_amd.assets import synthetic_image

    if name == "solid":
        return s.solid((0.7, 0.5, 0.3))
    if name == "checker_solid_noise":
        return s.checker(s.solid((0.9, 0.2, 0.2)), s.noise(3.0, 5))
    if name == "checker_image_solid":
        return s.checker(s.image(synthetic_image(13, 7, 3)), s.solid((0.2, 0.2, 0.9)))
    if name == "noise":
        return s.noise(4.0, 2)
    if name.startswith("turbulence"):
        return s.turbulent(2.5, int(name.split("_")[1]), 3)
    if name == "marble":
        return s.marble(3.0, 4)
    if name == "image_none":
        return s.image(None)
    w, h, c = (int(x) for x in name.split("_")[1].split("x"))
    return s.image(synthetic_image(w, h, c, seed=w), tail=3 - c if c < 3 else 0)


def shading(tex: str, mat: str, black: bool = False) -> FlatScene:
    """Every primitive type (sphere, moving sphere, the three rects, box, triangle with and without
    vertex normals) with one material over one texture, as a list world (`_bvh`: under one BVH)."""
    s = FlatScene(background=(0, 0, 0) if black else (0.7, 0.8, 1.0))
    s.camera((0.3, 1.8, -5.5), (0, 0.4, 0.6), 40.0)
    t = make_texture(s, tex)
    m = {"lambertian": lambda: s.lambertian(t), "metal_0": lambda: s.metal(t, 0.0), "metal_1": lambda: s.metal(t, 1.0),
         "glass_1.0": lambda: s.dielectric(1.0, t), "glass_0.7": lambda: s.dielectric(0.7, t),
         "glass_1.5": lambda: s.dielectric(1.5, t), "light": lambda: s.light(t), "isotropic": lambda: s.isotropic(t)}[mat]()
    nrm = [(0.2, 0.1, -1.0), (-0.2, 0.1, -1.0), (0.0, -0.3, -1.0)]
    ids = [s.sphere((-2.0, 0.5, 0.6), 0.6, m), s.moving((-0.6, 0.4, 0.2), (-0.6, 0.8, 0.2), 0.0, 1.0, 0.5, m),
           s.rect("xy", -3.0, 3.0, -0.2, 2.4, 2.6, m), s.rect("xz", -4.0, 4.0, -3.0, 3.0, -0.2, m),
           s.rect("yz", -0.2, 2.0, -1.0, 2.6, 2.9, m), s.box((0.4, -0.2, -0.3), (1.3, 0.7, 0.6), m),
           s.tri((1.5, -0.1, 0.2), (2.6, -0.1, 0.9), (2.0, 1.3, 0.6), m, uv=(0, 0, 1, 0, 0.5, 1)),
           s.tri((-1.6, 1.2, 1.5), (-0.2, 1.3, 1.7), (-0.9, 2.3, 1.6), m, uv=(0.1, 0.1, 0.9, 0.2, 0.4, 0.8), normals=nrm)]
    s.world = [s.obj_prim(i) for i in ids]
    if mat == "light":  # the emitters light diffuse twins of the two large rects, a little in front of them
        white = s.lambertian((0.8, 0.8, 0.8))
        s.world += [s.obj_prim(s.rect("xy", -3.0, 0.0, -0.2, 2.4, 2.5, white)),
                    s.obj_prim(s.rect("xz", -4.0, 4.0, -3.0, 1.5, -0.1, white)),
                    s.obj_prim(s.sphere((0, 0.3, -1.0), 0.5, white))]
    return s


def _lit(c, r, oracle):
    assert max(float(fb.max()) for fb in r.fbs) > 0.0, "nothing emits on the black background"


for _t in TEXTURES:
    case(f"shade:lambertian_{_t}", family=RENDER, merged="checker" not in _t, per_pixel=_t == "checker_image_solid")(functools.partial(shading, _t, "lambertian"))
for _m in ("metal_0", "metal_1", "glass_1.0", "glass_0.7", "isotropic"):
    case(f"shade:{_m}_solid", family=RENDER, merged=True)(functools.partial(shading, "solid", _m))
for _t in ("image_13x7x3", "image_13x7x1", "noise"):
    case(f"shade:metal_0_{_t}", family=RENDER, merged=True)(functools.partial(shading, _t, "metal_0"))
    case(f"shade:light_{_t}", family=RENDER, merged=True, evidence=_lit)(functools.partial(shading, _t, "light", True))
case("shade:glass_1.5_image_64x64x3", family=RENDER, merged=True)(functools.partial(shading, "image_64x64x3", "glass_1.5"))


# ---------------------------------------------------------------- group: ties
def ties(kind: str, swap: bool = False) -> FlatScene:
    """swap: the materials of the first two coincident primitives exchanged (the evidence's twin)."""
    s = look(FlatScene())
    mats = palette(s, checker=kind != "sphere_across_entries")
    red, blue, green = s.lambertian((0.9, 0.1, 0.1)), s.lambertian((0.1, 0.1, 0.9)), s.lambertian((0.1, 0.9, 0.1))
    if swap:
        red, blue = blue, red
    gr = ground(s)
    others = [s.sphere((1.4, 0.1, 0.3), 0.4, mats[1]), s.sphere((-1.5, 0.2, 0.9), 0.45, mats[2])]
    tv = ((-1.0, -0.3, 1.2), (1.0, -0.3, 1.2), (0.0, 1.5, 1.2))
    if kind == "sphere_twice_in_bvh":
        s.world = [s.bvh([s.sphere((0, 0.3, 0.8), 0.6, red), others[0], s.sphere((0, 0.3, 0.8), 0.6, blue), others[1], gr])]
    elif kind == "sphere_across_entries":
        s.world = [s.obj_prim(s.sphere((0, 0.3, 0.8), 0.6, red)), s.bvh([others[0], s.sphere((0, 0.3, 0.8), 0.6, blue), others[1], gr]),
                   s.obj_prim(s.sphere((0, 0.3, 0.8), 0.6, green))] + _extra_prims(s, mats, 2, True)
    elif kind == "triangle_in_list_and_bvh":
        s.world = [s.bvh([s.tri(*tv, red), others[0], s.tri(*tv, blue), others[1], gr, s.tri(*tv, green)]),
                   s.obj_list(s.tri(*tv, mats[3]), 1)]
    elif kind == "moving_spheres":
        mv = lambda m: s.moving((0, 0.3, 0.8), (0.3, 0.9, 0.8), 0.0, 1.0, 0.6, m)
        s.world = [s.bvh([mv(red), others[0], mv(blue), others[1], gr]), s.obj_prim(mv(green))]
    return s


def _tie_is_seen(kind, winner_swaps):
    """The coincident primitives tie in every query that reaches them, and the tie rule picks one: with the
    first two's materials exchanged the picture changes exactly when one of those two is the winner
    (inside a BVH the first visited wins; across list entries the last entry does, so there neither is)."""
    def ev(c, r, oracle):
        t = render_scene(oracle, ties(kind, swap=True), REF, c.depth)
        same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r.fbs, t.fbs))
        assert same != winner_swaps, "the tie is not resolved as the reference's rules say"
    return ev


case("ties:sphere_twice_in_bvh", family=STEP, per_pixel=True, evidence=_tie_is_seen("sphere_twice_in_bvh", True))(
    functools.partial(ties, "sphere_twice_in_bvh"))
case("ties:sphere_across_entries", family=RENDER, merged=True, evidence=_tie_is_seen("sphere_across_entries", False))(
    functools.partial(ties, "sphere_across_entries"))
case("ties:triangle_in_list_and_bvh", family=RENDER, evidence=_tie_is_seen("triangle_in_list_and_bvh", False))(
    functools.partial(ties, "triangle_in_list_and_bvh"))
case("ties:triangle_in_list_and_bvh_no_dedup", family=RENDER, options=dict(dedup_triangles=0),
     evidence=_tie_is_seen("triangle_in_list_and_bvh", False))(functools.partial(ties, "triangle_in_list_and_bvh"))
case("ties:moving_spheres", family=STEP, evidence=_tie_is_seen("moving_spheres", False))(functools.partial(ties, "moving_spheres"))


# ---------------------------------------------------------------- group: random scenes
SEEDS = tuple(range(1, 33))
DISCARDED_SEEDS: dict[int, str] = {}  # seed: reason (at most 1 in 8 of those tried)


def random_scene(seed: int) -> FlatScene:
    """A small grammar over everything above: a camera (shutter, aperture, field of view), materials
    over textures of every kind, and 1..6 world entries drawn from primitives, lists, BVHs with
    loosened or shrunk boxes, instances of them and media over them."""
    from raytracing_gpu_amd.assets import synthetic_image

    g = np.random.default_rng(seed)
    s = FlatScene()
    t0 = float(g.choice([0.0, 0.25, 0.5]))
    s.camera((g.uniform(-1, 1), g.uniform(1.0, 2.2), -5.0), (0, 0.2, 0.8), float(g.choice([25.0, 38.0, 60.0])),
             aperture=float(g.choice([0.0, 0.1])), focus=5.5, t0=t0, t1=float(t0 + g.choice([0.0, 0.5, 1.0])))
    texs = [s.solid(g.uniform(0.1, 0.9, 3)), s.noise(g.uniform(1, 5), seed), s.turbulent(2.0, int(g.integers(1, 8)), seed + 1),
            s.marble(3.0, seed + 2), s.image(synthetic_image(int(g.integers(1, 20)), int(g.integers(1, 20)), 3, seed)),
            s.image(synthetic_image(9, 5, 1, seed), tail=2)]
    texs.append(s.checker(texs[int(g.integers(0, 6))], texs[int(g.integers(0, 6))]))
    mats = [s.lambertian(t) for t in texs] + [s.metal(texs[0], g.uniform(0, 1)), s.metal(texs[4], 0.0),
                                              s.dielectric(1.5), s.dielectric(float(g.choice([0.7, 1.0, 2.4])))]
    pick = lambda: mats[int(g.integers(0, len(mats)))]

    def prim(cx, cz):
        k = int(g.integers(0, 6))
        c = np.array([cx + g.uniform(-0.2, 0.2), g.uniform(0.0, 0.8), cz + g.uniform(-0.2, 0.2)])
        r = g.uniform(0.25, 0.5)
        if k == 0:
            return s.sphere(c, r, pick())
        if k == 1:
            ta = float(g.choice([0.0, 2.0]))
            return s.moving(c, c + g.uniform(-0.3, 0.3, 3), ta, ta + float(g.choice([1.0, 0.5])), r, pick())
        if k == 2:
            return s.box(c - r, c + r * g.uniform(0.5, 1.5, 3), pick())
        if k == 3:
            pl = ("xy", "xz", "yz")[int(g.integers(0, 3))]
            a, b, kk = {"xy": (c[0], c[1], c[2]), "xz": (c[0], c[2], c[1]), "yz": (c[1], c[2], c[0])}[pl]
            return s.rect(pl, a - r, a + r, b - r, b + r, kk, pick())
        v = [c + g.uniform(-0.6, 0.6, 3) for _ in range(3)]
        return s.tri(*v, pick(), uv=g.uniform(0, 1, 6), normals=[g.uniform(-1, 1, 3) for _ in range(3)] if k == 5 else None)

    def leaf(cx, cz):
        k = int(g.integers(0, 3))
        if k == 0:
            return s.obj_prim(prim(cx, cz))
        if k == 1:
            first = prim(cx, cz)
            n = int(g.integers(1, 4))
            for _ in range(n - 1):
                prim(cx, cz)
            return s.obj_list(first, n)
        n = int(g.integers(3, 12))
        ids = [prim(cx + 0.5 * (i % 3 - 1), cz + 0.5 * (i // 3 - 1)) for i in range(n)]
        rows = max(2, (n - 1).bit_length())
        style = int(g.integers(0, 3))
        pad = g.uniform(0, 0.4, ((1 << rows) - 1, 3)) if style == 1 else None
        boxes = None
        if style == 2:
            lo = np.min([s.prim_box(i)[0] for i in ids[:n // 2]], axis=0)
            hi = np.max([s.prim_box(i)[1] for i in ids[:n // 2]], axis=0)
            boxes = {1: ((lo + hi) / 2 - 0.4 * (hi - lo), (lo + hi) / 2 + 0.4 * (hi - lo))}
        return s.bvh(ids, boxes=boxes, pad=pad)

    n_entries = int(g.integers(1, 7))
    for e in range(n_entries):
        cx, cz = (e % 3 - 1) * 1.5, (e // 3) * 1.6
        k = int(g.integers(0, 4))
        o = leaf(cx, cz)
        if k == 1:
            o = s.xform(o, g.uniform(-40, 40), g.uniform(-0.3, 0.3, 3), flags=int(g.integers(1, 4)))
        elif k == 2:
            o = s.medium(o if g.integers(0, 2) else s.xform(o, g.uniform(-20, 20), (0, 0.1, 0)), g.uniform(0.3, 2.0),
                         s.isotropic(g.uniform(0.2, 0.9, 3)))
        s.world.append(o)
    s.world.insert(int(g.integers(0, len(s.world) + 1)), s.obj_prim(s.sphere((0, -1000.3, 0), 1000.0, mats[0])))
    return s


for _s in SEEDS:
    case(f"random:{_s}", per_pixel=_s % 8 == 0)(functools.partial(random_scene, _s))
