"""A writer of flattened scenes (include/rt_hip.h, rt_scene_soa) for tests: whatever a test can write
down goes to `Context.upload` and to the oracle's `RefScene.from_flat` unchanged, through `.soa`.

Nothing here has to match the reference bit for bit: both sides consume what is stored (derived
fields, camera vectors, BVH boxes).  The arrays stay alive as long as the FlatScene does.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

import raytracing_gpu_amd as rt

F32 = np.float32
TRI_DTYPE = np.dtype([("v0", F32, 3), ("v1", F32, 3), ("v2", F32, 3), ("e0", F32, 3), ("e1", F32, 3),
                      ("d00", F32), ("d01", F32), ("d11", F32), ("inv_denom", F32), ("uv", F32, 6),
                      ("n0", F32, 3), ("n1", F32, 3), ("n2", F32, 3), ("vertex_normals", np.int32), ("pad", np.int32)])
PERLIN_DTYPE = np.dtype([("ranvec", F32, (256, 3)), ("perm_x", np.int32, 256), ("perm_y", np.int32, 256),
                         ("perm_z", np.int32, 256)])
IMAGE_DTYPE = np.dtype([("width", np.int32), ("height", np.int32), ("bytes_per_pixel", np.int32), ("offset", np.int32)])
assert TRI_DTYPE.itemsize == 144 and PERLIN_DTYPE.itemsize == 6144 and IMAGE_DTYPE.itemsize == 16

TEX_SOLID, TEX_CHECKER, TEX_NOISE, TEX_TURBULENT, TEX_MARBLE, TEX_IMAGE = range(6)
RECT_TYPE = {"xy": rt.PRIM_RECT_XY, "xz": rt.PRIM_RECT_XZ, "yz": rt.PRIM_RECT_YZ}
SKY = (0.7, 0.8, 1.0)


def v3(x) -> np.ndarray:
    return np.asarray(x, F32).reshape(3)


class FlatScene:
    def __init__(self, background=SKY, aspect: float = 40.0 / 24.0):
        self.background = v3(background)
        self.aspect = float(aspect)
        self.world: list[int] = []
        self.objects: list[rt.rt_object] = []
        self.prims: list[rt.rt_prim] = []
        self.tris: list[tuple] = []
        self.nodes: list[rt.rt_bvh_node] = []
        self.mats: list[rt.rt_material] = []
        self.texs: list[rt.rt_texture] = []
        self.perlins: list[np.ndarray] = []
        self.images: list[tuple] = []
        self.texels = bytearray()
        self.cam = rt.rt_camera()
        self.shutter = (0.0, 1.0)
        self.camera((0, 0, -3), (0, 0, 0), 40.0)
        self._keep = []  # every .soa handed out stays valid while the FlatScene lives

    # ---------------------------------------------------------------- camera (camera.h:18-47)
    def camera(self, frm, at, vfov, aperture=0.0, focus=10.0, t0=0.0, t1=1.0, vup=(0, 1, 0), aspect=None):
        frm, at, vup = v3(frm), v3(at), v3(vup)
        asp = F32(self.aspect if aspect is None else aspect)
        h = F32(math.tan(math.radians(float(vfov)) / 2.0))
        vh = F32(2.0) * h
        vw = asp * vh
        w = frm - at
        w = (w / F32(np.linalg.norm(w))).astype(F32)
        u = np.cross(vup, w).astype(F32)
        u = (u / F32(np.linalg.norm(u))).astype(F32)
        v = np.cross(w, u).astype(F32)
        horiz = (F32(focus) * vw * u).astype(F32)
        vert = (F32(focus) * vh * v).astype(F32)
        llc = (frm - horiz / F32(2) - vert / F32(2) - F32(focus) * w).astype(F32)
        c = self.cam
        for name, val in (("origin", frm), ("lower_left", llc), ("horizontal", horiz), ("vertical", vert),
                          ("u", u), ("v", v), ("w", w)):
            setattr(c, name, (ctypes.c_float * 3)(*[float(x) for x in val]))
        c.lens_radius = float(F32(aperture) / F32(2))
        c.time0, c.time1 = float(t0), float(t1)
        self.shutter = (float(t0), float(t1))
        return self

    # ---------------------------------------------------------------- textures, materials
    def _tex(self, type_, a=0, b=0, color=(0, 0, 0), scale=0.0) -> int:
        self.texs.append(rt.rt_texture(type_, a, b, 0, (ctypes.c_float * 3)(*[float(x) for x in color]), float(scale)))
        return len(self.texs) - 1

    def solid(self, color) -> int:
        return self._tex(TEX_SOLID, color=color)

    def checker(self, even: int, odd: int) -> int:
        return self._tex(TEX_CHECKER, even, odd)

    def perlin(self, seed: int = 1) -> int:
        g = np.random.default_rng(seed)
        p = np.zeros((), PERLIN_DTYPE)
        r = g.uniform(-1.0, 1.0, (256, 3))
        p["ranvec"] = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F32)
        for k in ("perm_x", "perm_y", "perm_z"):
            p[k] = g.permutation(256).astype(np.int32)
        self.perlins.append(p)
        return len(self.perlins) - 1

    def noise(self, scale: float, seed: int = 1) -> int:
        return self._tex(TEX_NOISE, self.perlin(seed), 0, scale=scale)

    def turbulent(self, scale: float, depth: int = 7, seed: int = 1) -> int:
        return self._tex(TEX_TURBULENT, self.perlin(seed), depth, scale=scale)

    def marble(self, scale: float, seed: int = 1) -> int:
        return self._tex(TEX_MARBLE, self.perlin(seed), 7, scale=scale)

    def image(self, texels, tail: int = 0) -> int:
        """An image texture over texels (H, W, C) uint8 in stbi layout, or None / width 0 for the
        reference's no-data cyan.  tail: extra bytes appended after the image (an image of fewer than
        3 bytes per pixel reads its last texel's neighbours there)."""
        if texels is None:
            self.images.append((0, 0, 0, len(self.texels)))
        else:
            a = np.ascontiguousarray(texels, np.uint8)
            a = a[:, :, None] if a.ndim == 2 else a
            self.images.append((a.shape[1], a.shape[0], a.shape[2], len(self.texels)))
            self.texels += a.tobytes() + bytes((37 * (k + 1)) & 255 for k in range(tail))
        return self._tex(TEX_IMAGE, len(self.images) - 1)

    def material(self, type_: int, tex: int = -1, param: float = 0.0) -> int:
        self.mats.append(rt.rt_material(type_, tex, float(param), 0))
        return len(self.mats) - 1

    def lambertian(self, tex_or_color) -> int:
        return self.material(rt.MAT_LAMBERTIAN, self._as_tex(tex_or_color))

    def metal(self, tex_or_color, fuzz: float) -> int:
        return self.material(rt.MAT_METAL, self._as_tex(tex_or_color), fuzz)

    def dielectric(self, ior: float, tex: int = -1) -> int:
        return self.material(rt.MAT_DIELECTRIC, tex, ior)

    def light(self, tex_or_color) -> int:
        return self.material(rt.MAT_DIFFUSE_LIGHT, self._as_tex(tex_or_color))

    def isotropic(self, tex_or_color) -> int:
        return self.material(rt.MAT_ISOTROPIC, self._as_tex(tex_or_color))

    def _as_tex(self, t) -> int:
        return t if isinstance(t, (int, np.integer)) else self.solid(t)

    # ---------------------------------------------------------------- primitives
    def _prim(self, type_: int, mat: int, p) -> int:
        q = [float(F32(x)) for x in p] + [0.0] * (10 - len(p))
        self.prims.append(rt.rt_prim((ctypes.c_float * 10)(*q), type_, mat))
        return len(self.prims) - 1

    def sphere(self, c, r, mat) -> int:
        return self._prim(rt.PRIM_SPHERE, mat, [*v3(c), r])

    def moving(self, c0, c1, t0, t1, r, mat) -> int:
        c0, c1 = v3(c0), v3(c1)
        return self._prim(rt.PRIM_MOVING_SPHERE, mat, [*c0, r, *(c1 - c0), t0, F32(t1) - F32(t0)])

    def rect(self, plane: str, a0, a1, b0, b1, k, mat) -> int:
        return self._prim(RECT_TYPE[plane], mat, [a0, a1, b0, b1, k, F32(a1) - F32(a0), F32(b1) - F32(b0)])

    def box(self, p0, p1, mat) -> int:
        return self._prim(rt.PRIM_BOX, mat, [*v3(p0), *v3(p1)])

    def tri(self, a, b, c, mat, uv=(0, 0, 1, 0, 0, 1), normals=None) -> int:
        a, b, c = v3(a), v3(b), v3(c)
        e0, e1 = b - a, c - a
        dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]  # triangle.h:28-30's order, every step in float32
        d00, d01, d11 = dot(e0, e0), dot(e0, e1), dot(e1, e1)
        t = np.zeros((), TRI_DTYPE)
        t["v0"], t["v1"], t["v2"], t["e0"], t["e1"] = a, b, c, e0, e1
        t["d00"], t["d01"], t["d11"] = d00, d01, d11
        t["inv_denom"] = F32(1) / (d00 * d11 - d01 * d01)
        t["uv"] = np.asarray(uv, F32)
        if normals is not None:
            t["n0"], t["n1"], t["n2"] = [v3(n) for n in normals]
            t["vertex_normals"] = 1
        self.tris.append(t)
        return self._prim(rt.PRIM_TRIANGLE, mat, [len(self.tris) - 1])

    def prim_box(self, pi: int, t0=None, t1=None):
        """(lo, hi) float32 of primitive pi over the shutter [t0, t1] (default: the camera's)."""
        t0 = self.shutter[0] if t0 is None else t0
        t1 = self.shutter[1] if t1 is None else t1
        q = self.prims[pi]
        p = np.array(list(q.p), F32)
        e = F32(1e-4)
        if q.type == rt.PRIM_SPHERE:
            r = abs(p[3])
            return p[:3] - r, p[:3] + r
        if q.type == rt.PRIM_MOVING_SPHERE:
            r = abs(p[3])
            cs = [p[:3] + ((F32(t) - p[7]) / p[8]) * p[4:7] for t in (t0, t1)]
            return np.minimum(cs[0], cs[1]) - r, np.maximum(cs[0], cs[1]) + r
        if q.type == rt.PRIM_RECT_XY:
            return np.array([p[0], p[2], p[4] - e], F32), np.array([p[1], p[3], p[4] + e], F32)
        if q.type == rt.PRIM_RECT_XZ:
            return np.array([p[0], p[4] - e, p[2]], F32), np.array([p[1], p[4] + e, p[3]], F32)
        if q.type == rt.PRIM_RECT_YZ:
            return np.array([p[4] - e, p[0], p[2]], F32), np.array([p[4] + e, p[1], p[3]], F32)
        if q.type == rt.PRIM_BOX:
            return p[:3].copy(), p[3:6].copy()
        t = self.tris[int(p[0])]
        vs = np.stack([t["v0"], t["v1"], t["v2"]])
        lo, hi = vs.min(axis=0), vs.max(axis=0)
        flat = np.abs(hi - lo) < 1e-6
        return (lo - np.where(flat, e, F32(0))).astype(F32), (hi + np.where(flat, e, F32(0))).astype(F32)

    # ---------------------------------------------------------------- objects
    def _obj(self, kind: int, a: int, b: int = 0, f=()) -> int:
        ff = [float(F32(x)) for x in f] + [0.0] * (8 - len(f))
        self.objects.append(rt.rt_object(kind, a, b, 0, (ctypes.c_float * 8)(*ff)))
        return len(self.objects) - 1

    def obj_prim(self, pi: int) -> int:
        return self._obj(rt.OBJ_PRIM, pi)

    def obj_list(self, first: int, count: int) -> int:
        return self._obj(rt.OBJ_LIST, first, count)

    def xform(self, child: int, deg: float = 0.0, off=(0, 0, 0), flags: int = 3) -> int:
        rad = math.radians(float(deg))
        return self._obj(rt.OBJ_XFORM, child, flags, [*v3(off), math.sin(rad), math.cos(rad)])

    def medium(self, boundary: int, density: float, phase_mat: int) -> int:
        return self._obj(rt.OBJ_MEDIUM, boundary, phase_mat, [F32(-1) / F32(density)])

    def bvh(self, prim_ids, boxes: dict | None = None, pad=None) -> int:
        """A reference-layout BVH (bvh.h:163-346) over prim_ids, in the order given: `rows` =
        ceil(log2 n) inner levels in heap order, the left child gets floor(n/2) primitives and the right
        child the rest, the last row holds one or two leaves with leaf_a filled first.  Boxes are the
        union of the children's (a leaf's is prim_box); `pad` = (n_nodes, 3) array loosens every box by
        that much on both sides; `boxes` = {node: (lo, hi)} replaces a node's stored box afterwards
        (nothing propagates: the stored boxes need not nest)."""
        ids = [int(i) for i in prim_ids]
        n = len(ids)
        assert n >= 3
        rows = max(2, (n - 1).bit_length())
        inner, last0 = (1 << rows) - 1, (1 << (rows - 1)) - 1
        members = [None] * inner
        members[0] = ids
        lo, hi = np.zeros((inner, 3), F32), np.zeros((inner, 3), F32)
        leaf = np.full((inner, 2), -1, np.int64)
        for k in range(last0):
            m = members[k]
            nl = len(m) // 2
            members[2 * k + 1], members[2 * k + 2] = m[:nl], m[nl:]
        for k in range(inner - 1, -1, -1):
            if k >= last0:
                m = members[k]
                assert 1 <= len(m) <= 2
                leaf[k, :len(m)] = m
                bs = [self.prim_box(i) for i in m]
                lo[k] = np.min([b[0] for b in bs], axis=0)
                hi[k] = np.max([b[1] for b in bs], axis=0)
            else:
                lo[k] = np.minimum(lo[2 * k + 1], lo[2 * k + 2])
                hi[k] = np.maximum(hi[2 * k + 1], hi[2 * k + 2])
                leaf[k, 0] = k % 3  # the split axis slot of an inner node (unused by the traversal)
        if pad is not None:
            lo, hi = (lo - np.asarray(pad, F32)).astype(F32), (hi + np.asarray(pad, F32)).astype(F32)
        for k, (blo, bhi) in (boxes or {}).items():
            lo[k], hi[k] = v3(blo), v3(bhi)
        base = len(self.nodes)
        for k in range(inner):
            self.nodes.append(rt.rt_bvh_node((ctypes.c_float * 3)(*[float(x) for x in lo[k]]), int(leaf[k, 0]),
                                             (ctypes.c_float * 3)(*[float(x) for x in hi[k]]), int(leaf[k, 1])))
        return self._obj(rt.OBJ_BVH, base, rows)

    def node_box(self, bvh_obj: int, k: int):
        nd = self.nodes[self.objects[bvh_obj].a + k]
        return np.array(list(nd.lo), F32), np.array(list(nd.hi), F32)

    def n_bvh_nodes(self, bvh_obj: int) -> int:
        return (1 << self.objects[bvh_obj].b) - 1

    # ---------------------------------------------------------------- the rt_scene_soa
    @property
    def soa(self) -> rt.rt_scene_soa:
        """The scene as it stands now (built on every access: edit the lists, then read .soa)."""
        def arr(ctype, items):
            return (ctype * max(len(items), 1))(*items)

        world = arr(ctypes.c_int32, self.world)
        objects, prims, nodes = arr(rt.rt_object, self.objects), arr(rt.rt_prim, self.prims), arr(rt.rt_bvh_node, self.nodes)
        mats, texs = arr(rt.rt_material, self.mats), arr(rt.rt_texture, self.texs)
        tris = np.concatenate([t.reshape(1) for t in self.tris]) if self.tris else np.zeros(1, TRI_DTYPE)
        perlins = np.concatenate([p.reshape(1) for p in self.perlins]) if self.perlins else np.zeros(1, PERLIN_DTYPE)
        images = np.array(self.images, IMAGE_DTYPE) if self.images else np.zeros(1, IMAGE_DTYPE)
        texels = np.frombuffer(bytes(self.texels) or b"\0", np.uint8).copy()
        s = rt.rt_scene_soa()
        s.camera = self.cam
        s.background = (ctypes.c_float * 3)(*[float(x) for x in self.background])
        s.aspect = self.aspect
        s.world, s.n_world = world, len(self.world)
        s.objects, s.n_objects = objects, len(self.objects)
        s.prims, s.n_prims = prims, len(self.prims)
        s.triangles, s.n_triangles = tris.ctypes.data, len(self.tris)
        s.nodes, s.n_nodes = nodes, len(self.nodes)
        s.materials, s.n_materials = mats, len(self.mats)
        s.textures, s.n_textures = texs, len(self.texs)
        s.perlins, s.n_perlins = perlins.ctypes.data, len(self.perlins)
        s.images, s.n_images = images.ctypes.data, len(self.images)
        s.texels, s.n_texels = texels.ctypes.data, len(self.texels)
        self._keep.append((world, objects, prims, nodes, mats, texs, tris, perlins, images, texels, s))
        return s
