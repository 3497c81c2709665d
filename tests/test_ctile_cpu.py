"""tests/ctile_ref.py (the camera-ray culling rule restated in float64) on hand-made cameras and spheres: the
reference that tests/test_ctile_gpu.py holds the device to must itself be what rt_kernels.hip documents, and
must by itself give the guarantee the render kernels rely on."""
import math

import numpy as np
import pytest

import ctile_ref as cr
import flat_cases
from flat_scenes import FlatScene

SHIFT, CAP = 3, 32
F64 = np.float64


def cam(lens=0.0, **kw):
    """Origin at 0 looking down -z, the focus plane 2 away and 2 x 2 large."""
    return cr.make_camera((0, 0, 0), (-1, -1, -2), (2, 0, 0), (0, 2, 0), lens, **kw)


def margin(fr, X, r):
    """The keep margin of a sphere (X, r), written from the documentation: the radius, 4e-3 of the reach, the lens
    term and 1e-6."""
    reach = float(np.linalg.norm(np.asarray(X, F64) - fr.O)) + r + fr.L
    return r + 4e-3 * reach + fr.L * max(1.0, reach / (fr.dmin - fr.L)) + 1e-6


def test_source_constants():
    assert cr.source_constants() == {"kTileShift": SHIFT, "kTileCap": CAP}


def test_view_abi_declared_exported_bound(rtlib):
    """rt_camera_tiles_get_info / rt_camera_tiles_read are declared in the header, exported by the library and
    bound; the ctypes mirror of rt_camera_tiles_info has the C struct's ten int32 fields in the header's order,
    and the RT_CTILES_* constants are the header's."""
    import ctypes
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_hip.h")).read()
    for n in ("rt_camera_tiles_get_info", "rt_camera_tiles_read"):
        assert re.search(r"^\s*int\s+%s\s*\(" % n, hdr, re.M), n
        assert n in rtlib.ABI and hasattr(rtlib.lib(), n), n
    body = re.search(r"typedef struct rt_camera_tiles_info \{(.*?)\} rt_camera_tiles_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in re.findall(r"int32_t\s+([^;]+);", body) for f in decl.split(",")]
    assert fields == [k for k, _ in rtlib.rt_camera_tiles_info._fields_]
    assert ctypes.sizeof(rtlib.rt_camera_tiles_info) == 4 * len(fields) == 40
    for k in ("COUNT", "ENTRIES", "MASK", "SPHERES", "IDS"):
        assert int(re.search(r"#define RT_CTILES_%s (\d+)" % k, hdr).group(1)) == getattr(rtlib, "RT_CTILES_" + k)
    assert len(rtlib.CTILES_DTYPES) == 5
    o = rtlib.rt_camera_tiles_info()
    assert rtlib.lib().rt_camera_tiles_get_info(None, ctypes.byref(o)) == rtlib.RT_ERR_ARG  # host code: no context needed
    assert rtlib.lib().rt_camera_tiles_read(None, 0, None, 0, None) == rtlib.RT_ERR_ARG


def test_tiles_and_the_partial_last_tile():
    assert cr.tile_grid(100, 50, SHIFT) == (13, 7) and cr.tile_grid(96, 54, SHIFT) == (12, 7) and cr.tile_grid(40, 24, SHIFT) == (5, 3)
    assert cr.tile_rect(100, 50, 12, SHIFT) == (96, 0, 100, 8)      # 4 px wide
    assert cr.tile_rect(100, 50, 6 * 13, SHIFT) == (0, 48, 8, 50)   # 2 px high
    assert cr.tile_rect(20, 10, 5, SHIFT) == (16, 8, 20, 10)


@pytest.mark.parametrize("lens", [0.0, 0.05])
def test_frustum_planes(lens):
    """The four unit normals point inward, pass through the origin and through the tile's corners padded by
    0.01 px; dmin is the distance to the focus plane."""
    W, H = 20, 10
    for t in range(6):
        fr = cr.Frustum(cam(lens), W, H, t, SHIFT)
        i0, j0, i1, j1 = cr.tile_rect(W, H, t, SHIFT)
        assert fr.ok and abs(fr.dmin - 2.0) < 1e-12 and abs(fr.L - (float(np.float32(lens)) * (1 + 1e-5) + 1e-7)) < 1e-15
        assert np.allclose(np.linalg.norm(fr.N, axis=1), 1.0, atol=1e-14)
        corners = [(i0 - 0.01, j0 - 0.01), (i1 + 0.01, j0 - 0.01), (i1 + 0.01, j1 + 0.01), (i0 - 0.01, j1 + 0.01)]
        for c, (x, y) in enumerate(corners):
            d = np.array([-1 + 2 * x / W, -1 + 2 * y / H, -2.0])
            assert np.allclose(fr.D[c], d, atol=1e-12)
            assert abs(fr.N[c] @ d) < 1e-12 and abs(fr.N[(c + 3) & 3] @ d) < 1e-12  # on the two planes it spans
            assert fr.N[(c + 1) & 3] @ d > 0 and fr.N[(c + 2) & 3] @ d > 0           # inside the other two
        mid = np.array([-1 + (i0 + i1) / W, -1 + (j0 + j1) / H, -2.0])
        assert (fr.N @ mid > 0).all()


@pytest.mark.parametrize("lens", [0.0, 0.05])
@pytest.mark.parametrize("t", [0, 2, 5])
def test_spheres_on_and_about_each_side_plane(t, lens):
    """A sphere centred on a side plane is kept; pushed outward it is kept up to the documented margin and dropped
    just past it (the margin found by bisection on the documented formula, 1e-3 relative to either side)."""
    W, H, r = 20, 10, 0.01
    fr = cr.Frustum(cam(lens), W, H, t, SHIFT)
    for c in range(4):
        P = 1.5 * (fr.D[c] + fr.D[(c + 1) & 3])  # on plane c, between its two corner rays, 3 focus distances out
        at = lambda delta: P - delta * fr.N[c]
        kept, near = fr.sees([[*at(0.0), r]])
        assert kept[0] and not near[0]
        lo, hi = 0.0, 1.0
        for _ in range(200):  # delta - margin(delta) grows with delta: the margin's slope is ~4e-3
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if mid < margin(fr, at(mid), r) else (lo, mid)
        assert 0.03 < lo < 0.5
        assert lens == 0.0 or lo > 3 * 0.05  # the lens term: L * reach / (dmin - L) with reach ~ 6
        # (the rule reads float spheres: the steps must survive the cast, a float ulp at 6 is 5e-7)
        sph = np.array([[*at(lo * (1 - 1e-3)), r], [*at(lo * (1 + 1e-3)), r]], np.float32)
        kept, near = fr.sees(sph)
        assert kept[0] and not kept[1] and not near.any()


def test_near_pairs_are_counted():
    """A sphere placed (in float32) as close to a threshold as float32 allows is reported as near only when it is
    within 1e-9 relative: the band is narrow, a float32 step is ~1e-7."""
    fr = cr.Frustum(cam(), 20, 10, 0, SHIFT)
    # a sphere whose plane distance equals -m exactly: radius 0 margin terms only; construct m from pd
    X = np.array([-3.0, -0.5, -2.0], np.float32)
    C = X.astype(F64) - fr.O
    pd = float(fr.N[3] @ C)  # plane 3 is the tile's left side: X lies outside it
    assert pd < 0
    # choose r so that the margin equals -pd: m = r (1 + 4e-3) + 4e-3 |C| + 1e-6
    r = (-pd - 4e-3 * np.linalg.norm(C) - 1e-6) / (1 + 4e-3)
    near = [bool(fr.sees([[*X, np.float32(r * (1 + e))]])[1][0]) for e in (-1e-3, 0.0, 1e-3)]
    kept = [bool(fr.sees([[*X, np.float32(r * (1 + e))]])[0][0]) for e in (-1e-3, 0.0, 1e-3)]
    assert near[0] is False and near[2] is False and kept[0] is False and kept[2] is True
    # float32(r) is within 6e-8 of r: near only if that lands inside 1e-9; either way the flag equals its definition
    m = margin(fr, X, float(np.float32(r)))
    assert near[1] == (abs(pd + m) <= cr.NEAR_REL * m)


def test_camera_inside_a_sphere():
    fr = cr.Frustum(cam(0.05), 16, 16, 3, SHIFT)
    sph = np.array([[0, 0, -0.5, 5.0]], np.float32)
    assert fr.sees(sph)[0][0]
    want = 0.5 - 5.0 - fr.L - 1e-5 * (0.5 + 5.0 + fr.L) - 1e-6
    key = fr.nearest(sph)[0]
    assert key < 0 and key.dtype == np.float32
    assert float(key) <= want < float(np.nextafter(key, np.float32(np.inf)))  # rounded down, by less than one ulp
    assert abs(fr.nearest64(sph)[0] - want) < 1e-15


def test_float_rd():
    x = np.array([1.0 + 1e-9, 1.0, -1.0 - 1e-9, np.inf, -np.inf, np.nan, 1e39, -1e39], F64)
    got = cr.float_rd(x)
    big = np.finfo(np.float32).max
    assert got.tolist()[:5] == [1.0, 1.0, float(np.nextafter(np.float32(-1), np.float32(-2))), np.inf, -np.inf]
    assert got[5] == -np.inf and got[6] == big and got[7] == -np.inf  # (1e39 rounds down to the largest float)


@pytest.mark.parametrize("lens, ok", [(1.0, False), (0.99999, False), (0.999, True), (0.25, True), (3.0, False)])
def test_lens_against_focus_distance(lens, ok):
    """ok = dmin > 2 L: with the lens radius at half the focus distance (L carries 1e-5 on top) nothing is culled:
    every count is -1 and every mask all ones."""
    sph = np.array([[50, 0, -2, 0.1], [0, 0, -4, 0.1]], np.float32)  # the first far outside every tile
    tb = cr.Tables(cam(lens), 16, 16, sph, SHIFT, CAP)
    assert tb.ok.all() == ok and tb.ok.any() == ok
    if ok and lens > 0.9:  # the lens term L reach / (dmin - L) keeps everything within sight
        assert tb.kept.all()
    elif ok:
        assert not tb.kept[:, 0].any() and tb.kept[:, 1].all()
        assert (tb.counts() == 1).all() and (tb.masks() == 0xFFFFFFFE).all()
    else:
        assert (tb.counts() == -1).all() and (tb.masks() == 0xFFFFFFFF).all()


def test_unbounded_and_nan_spheres_are_always_kept():
    sph = np.array([[0, 0, 0, np.inf], [1e30, 0, 0, 1.0], [np.nan, 0, 0, 1.0], [50, 0, -2, 0.1]], np.float32)
    tb = cr.Tables(cam(), 16, 16, sph, SHIFT, CAP)
    assert tb.kept[:, 0].all() and tb.kept[:, 2].all() and not tb.kept[:, 3].any() and not tb.near.any()
    assert (tb.key[:, 0] == -np.inf).all() and (tb.key[:, 2] == -np.inf).all()
    assert not tb.kept[:, 1].any()  # far, but bounded: 1e30 to the right of every tile
    assert (tb.masks() == 0xFFFFFFFF & ~0b1010).all()


def test_partial_last_tile_is_clipped_to_the_image():
    """W = 20: the last column's tiles are 4 px wide.  A small sphere seen through where pixel 22 would be lies
    outside them; one seen through pixel 18 lies inside."""
    W, H = 20, 10
    at = lambda i, j: 3.0 * np.array([-1 + 2 * (i + 0.5) / W, -1 + 2 * (j + 0.5) / H, -2.0])
    sph = np.array([[*at(18, 3), 0.01], [*at(22, 3), 0.01], [*at(18, 11), 0.01]], np.float32)
    tb = cr.Tables(cam(), W, H, sph, SHIFT, CAP)
    assert (tb.tx, tb.ty) == (3, 2)
    assert np.flatnonzero(tb.kept[:, 0]).tolist() == [2] and not tb.kept[:, 1].any() and not tb.kept[:, 2].any()
    assert tb.counts().tolist() == [0, 0, 1, 0, 0, 0]


def test_counts_overflow_at_the_cap():
    sph = np.array([[0.001 * k, 0, -4, 0.1] for k in range(CAP + 1)], np.float32)
    tb = cr.Tables(cam(), 8, 8, sph[:CAP], SHIFT, CAP)
    assert tb.counts().tolist() == [CAP]
    tb = cr.Tables(cam(), 8, 8, sph, SHIFT, CAP)
    assert tb.counts().tolist() == [-1]
    # masks: 35 entries have 32 bits; a dropped entry past them changes nothing
    far = np.array([[50, 0, -2, 0.1]] * 35, np.float32)
    assert (cr.Tables(cam(), 8, 8, far, SHIFT, CAP).masks() == 0).all()
    assert (cr.Tables(cam(), 8, 8, far[:3], SHIFT, CAP).masks() == 0xFFFFFFF8).all()


@pytest.mark.parametrize("lens", [0.0, 0.3])
def test_rays_of_tile_are_the_tiles_family(lens):
    W, H = 20, 10
    c = cam(lens, time0=0.25, time1=0.75)
    for t in (0, 2, 5):
        i0, j0, i1, j1 = cr.tile_rect(W, H, t, SHIFT)
        r = cr.rays_of_tile(c, W, H, t, 256, 7, SHIFT).astype(F64)
        assert r.shape == (256, 8)
        off = r[:, :3]  # the origin is 0
        F = r[:, :3] + r[:, 3:6]  # the point on the focus plane
        s, v = (F[:, 0] + 1) / 2 * W, (F[:, 1] + 1) / 2 * H
        assert np.allclose(F[:, 2], -2.0, atol=1e-6) and np.allclose(off[:, 2], 0.0)
        assert (s >= i0 - 1e-4).all() and (s <= i1 + 1e-4).all() and (v >= j0 - 1e-4).all() and (v <= j1 + 1e-4).all()
        for q, (x, y) in enumerate([(i0, j0), (i1, j0), (i1, j1), (i0, j1)]):  # the corners, jitter 0 and 1
            assert abs(s[q] - x) < 1e-4 and abs(v[q] - y) < 1e-4
        rad = np.linalg.norm(off, axis=1)
        assert (rad <= lens * (1 + 1e-6)).all()
        if lens:
            assert (rad[:16] >= lens * (1 - 1e-6)).all() and (rad >= lens * (1 - 1e-6)).sum() >= 64
            assert (rad < 0.9 * lens).sum() >= 64
        tm = r[:, 6]
        assert (tm >= 0.25).all() and (tm <= 0.75).all() and (tm == 0.25).sum() >= 16 and (tm == 0.75).sum() >= 16
        assert ((tm > 0.25) & (tm < 0.75)).sum() >= 128
        assert not np.array_equal(r, cr.rays_of_tile(c, W, H, t, 256, 8, SHIFT))
        assert np.array_equal(r, cr.rays_of_tile(c, W, H, t, 256, 7, SHIFT))


def test_sphere_hits_by_hand():
    import raytracing_gpu_amd as rt

    p = np.zeros((3, 10))
    p[0, :4] = (0, 0, -5, 1)
    p[1, :4] = (0, 0, 0, 2)  # the ray starts inside: the far root
    p[2, :9] = (0, 10, -5, 1, 0, -20, 0, 0.25, 0.5)  # at time 0.5 the centre is (0, 0, -5)
    ty = np.array([rt.PRIM_SPHERE, rt.PRIM_SPHERE, rt.PRIM_MOVING_SPHERE])
    rays = np.array([[0, 0, 0, 0, 0, -2, 0.5, 0], [0, 0, 0, 0, 0, -2, 0.25, 0], [0, 0, 0, 0, 1, 0, 0.5, 0]], np.float32)
    t = cr.sphere_hits((p, ty), rays)
    assert np.allclose(t[0], [2.0, 1.0, 2.0]) and np.allclose(t[1][:2], [2.0, 1.0]) and t[1][2] == np.inf
    assert t[2][0] == np.inf and np.isclose(t[2][1], 2.0)


def test_entry_of_prim():
    import raytracing_gpu_amd as rt

    for name in ("world:medium_over_bvh", "world:instanced_bvhs", "world:bvh_then_list", "world:medium_over_xform"):
        s = flat_cases.get(name).scene
        under = cr.entry_of_prim(s)
        assert under.shape == (len(s.prims), len(s.world))
        for w, oi in enumerate(s.world):
            o = s.objects[oi]
            while o.kind in (rt.OBJ_XFORM, rt.OBJ_MEDIUM):
                o = s.objects[o.a]
            n = {rt.OBJ_PRIM: 1, rt.OBJ_LIST: o.b}.get(o.kind)
            if o.kind == rt.OBJ_BVH:
                n = sum(1 for k in range(cr_rows(o)) for p in (s.nodes[o.a + k].leaf_a, s.nodes[o.a + k].leaf_b)
                        if k >= (1 << (o.b - 1)) - 1 and p >= 0)
            assert under[:, w].sum() == n, (name, w)
        if name == "world:instanced_bvhs":  # entries 0 and 2 instance the same BVH
            assert np.array_equal(under[:, 0], under[:, 2]) and (under.sum(axis=1) <= 2).all() and (under.sum(axis=1) == 2).sum() == 4
        elif name == "world:bvh_then_list":
            assert under[:, 1].sum() == 6 and (under.sum(axis=1) <= 1).all()
        else:
            assert (under.sum(axis=1) <= 1).all()


def cr_rows(o):
    return (1 << o.b) - 1


# ------------------------------------------------------------------ the guarantee, on the reference alone
def _garden(lens, t0=0.0, t1=1.0):
    s = FlatScene(aspect=96.0 / 54.0)
    s.camera((0.4, 1.6, -5.0), (0, 0.1, 0.8), 38.0, aperture=2 * lens, focus=5.0, t0=t0, t1=t1)
    m = s.lambertian((0.5, 0.5, 0.5))
    flat_cases.grid_spheres(s, 60, [m], 1, r=0.3)
    for i in range(6):
        c0 = np.array([(i - 2.5) * 0.9, 0.9, 1.0 + 0.3 * i])
        s.moving(c0, c0 + (0.2, 0.5, 0.0), 0.0, 1.0, 0.25, m)
    flat_cases.ground(s)
    return s


def _own_spheres(s):
    """Bounding spheres of a sphere scene's primitives over the shutter, the primitive itself where it is still."""
    import raytracing_gpu_amd as rt

    out = []
    for k in range(len(s.prims)):
        lo, hi = (x.astype(F64) for x in s.prim_box(k))
        c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
        still = s.prims[k].type == rt.PRIM_SPHERE
        rad = abs(s.prims[k].p[3]) if still else float(np.linalg.norm(h))
        out.append([*c, rad * (1 + 1e-6) + 1e-6 * np.abs(c).sum()])
    return np.array(out, np.float32)


@pytest.mark.parametrize("lens, shutter", [(0.0, (0.0, 1.0)), (0.15, (0.25, 0.75))], ids=["pinhole", "lens_shutter"])
def test_the_rule_alone_gives_the_guarantee(lens, shutter):
    """96 rays per tile against every sphere in float64: a sphere hit past t_min is kept by the rule for that tile,
    no nearer than its key.  Spheres both kept and dropped exist, so the check is not vacuous."""
    W, H = 40, 24
    s = _garden(lens, *shutter)
    c = cr.camera_of(s)
    sph = _own_spheres(s)
    tb = cr.Tables(c, W, H, sph, SHIFT, CAP)
    assert tb.ok.all() and tb.near.sum() == 0
    assert tb.kept.any(axis=1).all() and (~tb.kept).any(axis=1).all()
    spheres = cr.spheres_of(s)
    hits = 0
    for t in range(tb.tx * tb.ty):
        rays = cr.rays_of_tile(c, W, H, t, 96, 11, SHIFT)
        th = cr.sphere_hits(spheres, rays)
        dn = np.linalg.norm(rays[:, 3:6].astype(F64), axis=1)
        r, p = np.nonzero(np.isfinite(th))
        hits += len(r)
        assert tb.kept[t, p].all(), f"tile {t}: a ray hits sphere {p[~tb.kept[t, p]][:1]} that the rule drops"
        assert (th[r, p] * dn[r] >= tb.key[t, p].astype(F64)).all(), f"tile {t}: a hit undercuts its key"
    assert hits > 1000


def test_big1_is_not_vacuous_at_the_test_sizes():
    """What tests/test_ctile_gpu.py asserts of the device's big1 tables holds for the rule: at 96 x 54 at least one
    tile overflows the cap and at least half do not; 40 x 24 and 100 x 50 have both kinds too.  (Bounding spheres
    written here from the primitives; the device test reads the uploaded ones.)"""
    import raytracing_gpu_amd as rt

    sc = rt.Scene.builtin("big1")
    p = sc.prims()
    ty = p[:, 10].view(np.int32) & 0xFF
    assert np.isin(ty, (rt.PRIM_SPHERE, rt.PRIM_MOVING_SPHERE)).all()
    c = cr.camera_of(sc)
    t0, t1 = float(c["time0"]), float(c["time1"])
    sph = []
    for q, k in zip(p.astype(F64), ty):
        r = abs(q[3])
        if k == rt.PRIM_SPHERE:
            lo, hi = q[:3] - r, q[:3] + r
        else:
            cs = [q[:3] + (t - q[7]) / q[8] * q[4:7] for t in (t0, t1)]
            lo, hi = np.minimum(*cs) - r, np.maximum(*cs) + r
        cen, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
        sph.append([*cen, math.sqrt(float(h @ h)) * (1 + 2e-6) + 1e-6 * np.abs(cen).sum()])
    sph = np.array(sph, np.float32)
    for (W, H), half in (((96, 54), True), ((40, 24), False), ((100, 50), True)):
        tb = cr.Tables(c, W, H, sph, SHIFT, CAP)
        cnt = tb.counts()
        assert tb.ok.all() and tb.near.sum() == 0
        assert (cnt == -1).any() and (cnt >= 1).any(), (W, H, cnt.tolist())
        if half:
            assert 2 * (cnt >= 0).sum() >= len(cnt), (W, H, cnt.tolist())
