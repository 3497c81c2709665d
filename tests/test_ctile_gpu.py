"""The camera-ray culling tables read back (rt_camera_tiles_get_info / rt_camera_tiles_read) and held to
tests/ctile_ref.py.

A culling table that is vacuous (every list overflowed, every mask all ones) renders the oracle's frames and
only costs time; one that is too small is wrong only for the rays that graze the dropped candidate, a handful
of pixels at tile edges; a key that is too large or a list out of order only matters where a nearer winner
already stands.  The parity tests at 40 x 24 to 96 x 54 see none of these.  Here the per-tile candidate lists
(world = one BVH) and entry masks (list worlds) are compared with the rule restated in float64, and their
guarantee -- no camera ray of a tile hits something the tile's table lacks, or nearer than its key -- is tested
with 256 rays per tile through the host ray cast.  Every launch is also compared with the oracle's frames bit
for bit.  Groups as DESIGN.md 4.3 lists them.
"""
import ctypes

import numpy as np
import pytest

import ctile_ref as cr
import flat_cases
from flat_scenes import FlatScene

pytestmark = pytest.mark.gpu

REF = 0
STEP = "render_step_kernel<"
RAYS = 256
LISTS, MASKS, NONE = 1, 2, 0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def row_of_35() -> FlatScene:
    """35 sphere entries in a row across the view: a mask has bits for the first 32 only, and entries 32 to 34 (the
    right end) must be tested all the same."""
    s = FlatScene()
    mats = flat_cases.palette(s, checker=False)
    for k in range(35):
        s.world.append(s.obj_prim(s.sphere(((k - 17) * 0.4, 0.1 * (k % 3), 0.2 * (k % 2)), 0.18, mats[k % 6])))
    s.camera((0.0, 1.0, -12.0), (0, 0, 0), 40.0)
    return s


# name: (scene, W, H, what the launch must be handed)
CASES = {
    "big1_96x54": ("big1", 96, 54, LISTS),
    "big1_40x24": ("big1", 40, 24, LISTS),
    "big1_100x50": ("big1", 100, 50, LISTS),  # 13 x 7 tiles, the last column 4 px wide, the last row 2 px high
    "inside_glass": ("camera:inside_glass", 40, 24, LISTS),
    "vfov_1": ("camera:vfov_1", 40, 24, LISTS),
    "vfov_170": ("camera:vfov_170", 40, 24, LISTS),
    "far_400r": ("camera:far_400r", 40, 24, LISTS),
    "scale_small": ("camera:scale_small", 40, 24, LISTS),
    "scale_large": ("camera:scale_large", 40, 24, LISTS),
    "lens_wider_than_focus": ("camera:lens_wider_than_focus", 40, 24, LISTS),  # every count -1
    "shutter_quarter": ("time:shutter_quarter", 40, 24, LISTS),
    # "first" (a sphere of negative radius) is a list of six primitives: masks
    "first": ("first", 40, 24, MASKS),
    "cornell_smoke": ("cornell_smoke", 48, 48, MASKS),
    "medium_over_bvh": ("world:medium_over_bvh", 40, 24, MASKS),
    "bvh_then_list": ("world:bvh_then_list", 40, 24, MASKS),
    "row_of_35": ("row_of_35", 40, 24, MASKS),
    "inside_medium": ("camera:inside_medium", 40, 24, MASKS),
    # "triangles" is a BVH followed by a primitive: the stepwise kernel runs, whose depth-0 queries take lists
    # only when the world is one BVH, and masks belong to the other kernel.  It gets neither table.
    "triangles": ("triangles", 40, 24, NONE),
}
LIST_CASES = [k for k, v in CASES.items() if v[3] == LISTS]
MASK_CASES = [k for k, v in CASES.items() if v[3] == MASKS]

_scenes, _oracle_fb, _runs = {}, {}, {}


def _scene(name):
    """(what Context.upload takes, the oracle's scene)."""
    import raytracing_gpu_amd as rt
    from oracle import ref_cpu

    if name not in _scenes:
        if name == "row_of_35":
            s = row_of_35()
            _scenes[name] = (s, ref_cpu.RefScene.from_flat(s.soa))
        elif ":" in name:
            s = flat_cases.get(name).scene
            _scenes[name] = (s, ref_cpu.RefScene.from_flat(s.soa))
        else:
            _scenes[name] = (rt.Scene.builtin(name), ref_cpu.RefScene(name))
    return _scenes[name]


def _want(name, W, H, spp):
    if (name, W, H, spp) not in _oracle_fb:
        _oracle_fb[(name, W, H, spp)] = _scene(name)[1].render(W, H, spp, 0, 50, REF)[0].reshape(H, W, 3)
    return _oracle_fb[(name, W, H, spp)]


def _launch(rtlib, ctx, name, W, H, spp=1, tiles=None, **kw):
    """One launch of one frame buffer, compared with the oracle's frame; returns what the launch was handed."""
    import torch

    assert ctx.options()["bins_min_items_per_lane"] == 0.0 or "threshold" in kw
    kw.pop("threshold", None)
    args = rtlib.make_args(W, H, spp, 0, 1, 50, REF, **kw)
    rows = rtlib.owned_rows(args)
    ctx.render_init(W, H, 1984)
    fb = torch.full((len(rows) * W * 3,), float("nan"), dtype=torch.float32, device="cuda")
    try:
        if tiles is None:
            ctx.render(args, fb.data_ptr())
        else:
            ctx.render_tiles(args, tiles, fb.data_ptr())
    except rtlib.RtError as e:
        if e.status == rtlib.RT_ERR_HIP:  # a device error: nothing more starts on this GPU
            pytest.exit(f"{name} {W}x{H}: {e}", returncode=3)
        raise
    got = fb.cpu().numpy().reshape(len(rows), W, 3)
    want = _want(name, W, H, spp)[rows]
    if tiles is None:
        diff = (_bits(got) != _bits(want)).any(axis=2)
        assert not diff.any(), f"{name} {W}x{H} {kw}: {int(diff.sum())} pixels differ from the oracle"
    else:  # the listed 16 x 16 tiles are the oracle's, the rest untouched
        m = ~np.isnan(got).all(axis=2)
        assert m.any() and not m.all() and np.array_equal(_bits(got[m]), _bits(want[m]))
    return ctx.camera_tiles_info()["last_used"]


def _read_all(rtlib, ctx):
    """Every array the context holds, None for the ones it reports as absent (RT_ERR_STATE)."""
    out = {}
    for k in ("COUNT", "ENTRIES", "MASK", "SPHERES", "IDS"):
        try:
            out[k] = ctx.camera_tiles_read(getattr(rtlib, "RT_CTILES_" + k))
        except rtlib.RtError as e:
            assert e.status == rtlib.RT_ERR_STATE, (k, e)
            out[k] = None
    return out


class Run:
    """A case's launch, read-backs and reference, computed once and shared by the groups below."""

    def __init__(self, rtlib, ctx, case):
        name, W, H, want = CASES[case]
        k = cr.source_constants()
        self.case, self.name, self.W, self.H, self.want = case, name, W, H, want
        self.scene = _scene(name)[0]
        ctx.upload(self.scene)
        self.used = _launch(rtlib, ctx, name, W, H)
        self.kernel = ctx.last_render_kernel()
        self.info = ctx.camera_tiles_info()
        self.arr = _read_all(rtlib, ctx)
        self.cam = cr.camera_of(self.scene)
        self.shift, self.cap = k["kTileShift"], k["kTileCap"]
        self.tx, self.ty = cr.tile_grid(W, H, self.shift)
        self.nt = self.tx * self.ty
        self.sph = None if self.arr["SPHERES"] is None else self.arr["SPHERES"].reshape(-1, 4)
        self.ref = None if self.sph is None else cr.Tables(self.cam, W, H, self.sph, self.shift, self.cap)
        if want == LISTS and self.arr["COUNT"] is not None:
            self.cnt = self.arr["COUNT"].astype(np.int64)
            e = self.arr["ENTRIES"].reshape(self.nt, self.cap, 2)
            self.ids, self.keys = e[:, :, 0].astype(np.int64), e[:, :, 1].copy().view(np.float32)
        self._hits = None

    def hits(self, rtlib):
        """Per tile: (rays, the host cast's hits) of RAYS rays of the tile's family."""
        if self._hits is None:
            rays = np.concatenate([cr.rays_of_tile(self.cam, self.W, self.H, t, RAYS, 5, self.shift) for t in range(self.nt)])
            h = rtlib.cast_host(self.scene, rays)
            self._hits = rays.reshape(self.nt, RAYS, 8), h.reshape(self.nt, RAYS)
        return self._hits


def _run(rtlib, ctx, case) -> Run:
    if case not in _runs:
        _runs[case] = Run(rtlib, ctx, case)
    return _runs[case]


# ------------------------------------------------------------------ a. the tables ran and are not vacuous
@pytest.mark.parametrize("case", list(CASES))
def test_the_launch_was_handed_its_table(rtlib, gpu_ctx, oracle, case):
    """a. last_used and the view's sizes are what the world's shape says."""
    r = _run(rtlib, gpu_ctx, case)
    s = r.scene.soa
    one_bvh = s.n_world == 1 and s.objects[s.world[0]].kind == rtlib.OBJ_BVH
    assert r.kernel.startswith(STEP) == (r.want != MASKS), r.kernel
    assert r.used == r.want and r.info["last_used"] == r.want
    assert r.info["kind"] == r.want
    assert (r.info["cap"], r.info["tile_shift"]) == (r.cap, r.shift)
    if r.want != NONE:
        assert (r.info["width"], r.info["height"], r.info["tiles_x"], r.info["tiles_y"]) == (r.W, r.H, r.tx, r.ty)
    assert r.info["n_kind"] == (1 if one_bvh else 2)
    assert r.info["n"] == len(r.sph) == (int(cr.entry_of_prim(r.scene).any(axis=1).sum()) if one_bvh else min(s.n_world, 32))
    present = {LISTS: {"COUNT", "ENTRIES", "SPHERES", "IDS"}, MASKS: {"MASK", "SPHERES"}, NONE: {"SPHERES"}}[r.want]
    assert {k for k, v in r.arr.items() if v is not None} == present
    if r.want == LISTS:
        assert len(r.arr["COUNT"]) == r.nt and len(r.arr["ENTRIES"]) == r.nt * r.cap * 2 and len(r.arr["IDS"]) == r.info["n"]
    if r.want == MASKS:
        assert len(r.arr["MASK"]) == r.nt


OFF = {"no_bins": dict(bins=False), "exact": dict(exact=True), "audit": dict(audit=True, widest=True), "threshold": dict(threshold=1e9)}
# (the audit mode runs with the widest variant, which is not the stepwise kernel: lists have no audit case; masks
# have no threshold)
OFF_CASES = [("big1_40x24", "no_bins"), ("big1_40x24", "exact"), ("big1_40x24", "threshold"),
             ("cornell_smoke", "no_bins"), ("cornell_smoke", "exact"), ("cornell_smoke", "audit")]


@pytest.mark.parametrize("case, off", OFF_CASES)
def test_switches_that_turn_the_tables_off(rtlib, gpu_ctx, oracle, ctx_opts, case, off):
    """a. RT_FLAG_NO_CAMERA_BINS, RT_FLAG_EXACT_TRAVERSAL, the audit mode and bins_min_items_per_lane = 1e9 hand the
    kernel nothing; the launches before and after them are handed their table."""
    name, W, H, want = CASES[case]
    gpu_ctx.upload(_scene(name)[0])
    widest = dict(widest=True) if off == "audit" else {}
    assert _launch(rtlib, gpu_ctx, name, W, H, **widest) == want
    if off == "threshold":
        ctx_opts(bins_min_items_per_lane=1e9)
    assert _launch(rtlib, gpu_ctx, name, W, H, **OFF[off]) == NONE
    if off == "threshold":
        ctx_opts(bins_min_items_per_lane=0.0)
    assert _launch(rtlib, gpu_ctx, name, W, H, **widest) == want


def test_tables_are_not_vacuous(rtlib, gpu_ctx, oracle):
    """a. big1 at 96 x 54: at least one tile overflows its list and at least half do not; cornell_smoke: at least
    one mask has a clear bit among its entries' bits."""
    r = _run(rtlib, gpu_ctx, "big1_96x54")
    assert (r.cnt == -1).sum() >= 1 and 2 * (r.cnt >= 0).sum() >= r.nt, r.cnt.tolist()
    assert (r.cnt[r.cnt >= 0] >= 1).all() and r.cnt.max() <= r.cap
    r = _run(rtlib, gpu_ctx, "cornell_smoke")
    m = r.arr["MASK"].astype(np.int64)
    n = r.info["n"]
    assert n == 8 and ((m & ((1 << n) - 1)) != (1 << n) - 1).any(), [hex(x) for x in m]


# ------------------------------------------------------------------ b. membership equals the rule
@pytest.mark.parametrize("case", LIST_CASES)
def test_list_membership_equals_the_rule(rtlib, gpu_ctx, oracle, case):
    """b. cnt = -1 exactly when the rule keeps more than cap spheres (or the camera is degenerate), and a list's ids
    are exactly the primitives of the kept spheres.  No pair lies within 1e-9 of its threshold."""
    r = _run(rtlib, gpu_ctx, case)
    assert int(r.ref.near.sum()) == 0, "a (tile, sphere) pair lies on its threshold: choose another input"
    want = r.ref.counts()
    assert np.array_equal(r.cnt, want), f"tiles {np.flatnonzero(r.cnt != want)[:8]}: {r.cnt[r.cnt != want][:8]} != {want[r.cnt != want][:8]}"
    ids_of = r.arr["IDS"].astype(np.int64)
    for t in np.flatnonzero(r.cnt >= 0):
        got, exp = sorted(r.ids[t, :r.cnt[t]].tolist()), sorted(ids_of[r.ref.kept[t]].tolist())
        assert got == exp, f"tile {t}: listed {got}, the rule keeps {exp}"
    if case == "lens_wider_than_focus":
        assert (r.cnt == -1).all() and not r.ref.ok.any()
    else:
        assert r.ref.ok.all() and (r.cnt >= 0).any()


@pytest.mark.parametrize("case", MASK_CASES)
def test_mask_bits_equal_the_rule(rtlib, gpu_ctx, oracle, case):
    """b. Bit w < min(n, 32) is clear exactly when the rule drops entry w; every bit above is set."""
    r = _run(rtlib, gpu_ctx, case)
    assert int(r.ref.near.sum()) == 0, "a (tile, entry) pair lies on its threshold: choose another input"
    got, want = r.arr["MASK"].astype(np.int64), r.ref.masks()
    assert np.array_equal(got, want), f"tiles {np.flatnonzero(got != want)[:8]}: {[hex(x) for x in got[got != want][:8]]}"
    n = min(r.info["n"], 32)
    assert (got >> n == 0xFFFFFFFF >> n).all()
    if case == "row_of_35":
        assert r.scene.soa.n_world == 35 and n == 32 and ((got & 0xFFFFFFFF) != 0xFFFFFFFF).any()


# ------------------------------------------------------------------ c. keys and order
@pytest.mark.parametrize("case", LIST_CASES)
def test_list_keys_and_order(rtlib, gpu_ctx, oracle, case):
    """c. Within a list the keys are nondecreasing and the ids distinct; every key is within one float ulp of the
    restated `nearest` rounded down (two double evaluations that agree to ~1e-16 straddle at most one rounding
    boundary of a float)."""
    r = _run(rtlib, gpu_ctx, case)
    ids_of = r.arr["IDS"].astype(np.int64)
    q_of = {int(p): q for q, p in enumerate(ids_of)}
    assert len(q_of) == len(ids_of), "a primitive has two bounding spheres"
    checked = 0
    for t in np.flatnonzero(r.cnt >= 0):
        c = r.cnt[t]
        ids, keys = r.ids[t, :c], r.keys[t, :c]
        assert len(set(ids.tolist())) == c, f"tile {t}: an id twice"
        assert (np.diff(keys.astype(np.float64)) >= 0).all(), f"tile {t}: keys not ascending {keys}"
        want = r.ref.key[t, [q_of[int(p)] for p in ids]]
        lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
        assert ((keys >= lo) & (keys <= hi)).all(), f"tile {t}: keys {keys} restated {want}"
        checked += c
    assert checked > 0 or case == "lens_wider_than_focus"


# ------------------------------------------------------------------ d. the guarantee, by rays
@pytest.mark.parametrize("case", LIST_CASES + MASK_CASES)
def test_no_ray_of_a_tile_escapes_its_table(rtlib, gpu_ctx, oracle, case):
    """d. 256 rays per tile (corners, lens rim, shutter ends, random) through the host ray cast: the winner's
    primitive is in the tile's list (unless it overflowed) at t |d| >= its key, or its entry's mask bit is set.  For
    scenes of spheres alone also every sphere against every ray in float64: each one hit past t_min is listed and
    respects its key.  No tolerance: the rule's margins are the tolerance."""
    r = _run(rtlib, gpu_ctx, case)
    rays, hits = r.hits(rtlib)
    won = hits["prim"] >= 0
    assert won.sum() >= r.nt, "hardly a ray hits anything"
    dn = np.linalg.norm(rays[:, :, 3:6].astype(np.float64), axis=2)
    spheres = cr.spheres_of(r.scene)
    if r.want == MASKS:
        under = cr.entry_of_prim(r.scene)
        mask = r.arr["MASK"].astype(np.int64)
        allowed = np.array([[w >= 32 or (m >> w) & 1 == 1 for w in range(under.shape[1])] for m in mask])  # [tile, entry]
        for t in range(r.nt):
            p = hits["prim"][t][won[t]]
            ok = (under[p] & allowed[t][None, :]).any(axis=1)
            assert ok.all(), f"tile {t}: a ray's winner, primitive {p[~ok][:1]}, lies under an entry whose bit is clear"
        if case == "row_of_35":
            assert (hits["prim"][won] >= 32).any(), "no ray reaches the entries without a bit"
        if spheres is not None and under.sum(axis=1).max() == 1:
            ent = under.argmax(axis=1)
            for t in range(r.nt):
                th = cr.sphere_hits(spheres, rays[t])
                p = np.unique(np.nonzero(np.isfinite(th))[1])
                assert allowed[t][ent[p]].all(), f"tile {t}: a ray hits a sphere of an entry whose bit is clear"
        return
    ids_of = r.arr["IDS"].astype(np.int64)
    q_of = np.full(r.scene.soa.n_prims, -1, np.int64)
    q_of[ids_of] = np.arange(len(ids_of))
    for t in range(r.nt):
        key = np.full(len(ids_of), np.nan)  # per sphere of the tile: its key, NaN when not listed
        if r.cnt[t] >= 0:
            key[q_of[r.ids[t, :r.cnt[t]]]] = r.keys[t, :r.cnt[t]]
        else:
            key[:] = -np.inf  # an overflowed tile traverses the tree
        q = q_of[hits["prim"][t][won[t]]]
        assert (q >= 0).all()
        assert not np.isnan(key[q]).any(), f"tile {t}: the winner {ids_of[q[np.isnan(key[q])][:1]]} is not in the list"
        d = hits["t"][t][won[t]].astype(np.float64) * dn[t][won[t]]
        assert (d >= key[q]).all(), f"tile {t}: a winner at {d[d < key[q]][:1]} undercuts its key {key[q][d < key[q]][:1]}"
        if spheres is not None:
            th = cr.sphere_hits(spheres, rays[t])[:, ids_of]
            rr, qq = np.nonzero(np.isfinite(th))
            assert not np.isnan(key[qq]).any(), f"tile {t}: a ray hits sphere {ids_of[qq[np.isnan(key[qq])][:1]]}, not in the list"
            assert (th[rr, qq] * dn[t][rr] >= key[qq]).all(), f"tile {t}: a hit undercuts its key"


# ------------------------------------------------------------------ e. caching
def _snapshot(rtlib, ctx):
    a = _read_all(rtlib, ctx)
    return ctx.camera_tiles_info(), {k: None if v is None else v.copy() for k, v in a.items()}


def _same_tables(a, b, tiles_only=False):
    keys = ("COUNT", "MASK") if tiles_only else ("COUNT", "MASK", "SPHERES", "IDS")
    ok = all((a[1][k] is None) == (b[1][k] is None) and (a[1][k] is None or np.array_equal(a[1][k], b[1][k])) for k in keys)
    if ok and a[1]["COUNT"] is not None:  # only the first count pairs of a tile are defined
        cap = a[0]["cap"]
        ea, eb = a[1]["ENTRIES"].reshape(-1, cap, 2), b[1]["ENTRIES"].reshape(-1, cap, 2)
        ok = all(np.array_equal(ea[t, :max(c, 0)], eb[t, :max(c, 0)]) for t, c in enumerate(a[1]["COUNT"]))
    return ok


@pytest.mark.parametrize("name, want", [("big1", LISTS), ("cornell_smoke", MASKS)])
def test_the_table_is_cached_per_scene_and_size(rtlib, gpu_ctx, oracle, name, want):
    """e. Kept across launches of one configuration, across a band launch of the same image and across
    rt_render_tiles; rebuilt for another size and after a new upload with another camera."""
    W, H = 48, 48
    sc = _scene(name)[0]
    gpu_ctx.upload(sc)
    assert gpu_ctx.camera_tiles_info()["kind"] == 0  # a new scene: nothing valid yet
    assert _launch(rtlib, gpu_ctx, name, W, H) == want
    a = _snapshot(rtlib, gpu_ctx)
    assert a[0]["kind"] == want and (a[0]["width"], a[0]["height"]) == (W, H)
    assert _launch(rtlib, gpu_ctx, name, W, H, spp=2) == want
    assert _same_tables(a, _snapshot(rtlib, gpu_ctx))
    assert _launch(rtlib, gpu_ctx, name, W, H, band_rows=4, band_first=1, band_stride=3) == want  # rows parity-exact
    b = _snapshot(rtlib, gpu_ctx)
    assert b[0] == a[0] and _same_tables(a, b)
    assert _launch(rtlib, gpu_ctx, name, W, H, tiles=[0, 4, 8]) == want  # rt_render_tiles leaves it as it was
    b = _snapshot(rtlib, gpu_ctx)
    assert b[0] == a[0] and _same_tables(a, b)
    # a launch that is handed nothing leaves the table in place
    assert _launch(rtlib, gpu_ctx, name, W, H, bins=False) == NONE
    b = _snapshot(rtlib, gpu_ctx)
    assert b[0] == dict(a[0], last_used=NONE) and _same_tables(a, b)
    # another size: rebuilt
    assert _launch(rtlib, gpu_ctx, name, 40, 24) == want
    c = _snapshot(rtlib, gpu_ctx)
    assert (c[0]["width"], c[0]["height"], c[0]["tiles_x"], c[0]["tiles_y"]) == (40, 24, 5, 3)
    assert len(c[1]["COUNT" if want == LISTS else "MASK"]) == 15
    assert _launch(rtlib, gpu_ctx, name, W, H) == want
    assert _same_tables(a, _snapshot(rtlib, gpu_ctx))


def test_a_new_upload_with_another_camera_rebuilds_the_table(rtlib, gpu_ctx, oracle):
    """e. camera:vfov_1 and camera:vfov_170 hold the same spheres under two cameras, at one size."""
    W, H = 40, 24
    snaps = []
    for name in ("camera:vfov_1", "camera:vfov_170", "camera:vfov_1"):
        gpu_ctx.upload(_scene(name)[0])
        assert gpu_ctx.camera_tiles_info()["kind"] == 0
        with pytest.raises(rtlib.RtError) as e:
            gpu_ctx.camera_tiles_read(rtlib.RT_CTILES_COUNT)
        assert e.value.status == rtlib.RT_ERR_STATE
        assert _launch(rtlib, gpu_ctx, name, W, H) == LISTS
        snaps.append(_snapshot(rtlib, gpu_ctx))
    assert np.array_equal(snaps[0][1]["SPHERES"], snaps[1][1]["SPHERES"])
    assert not np.array_equal(snaps[0][1]["COUNT"], snaps[1][1]["COUNT"])
    assert _same_tables(snaps[0], snaps[2])


def test_read_sizes_and_errors(rtlib, gpu_ctx, oracle):
    """The size and error conventions are rt_schedule_read's."""
    r = _run(rtlib, gpu_ctx, "big1_40x24")
    gpu_ctx.upload(r.scene)
    assert _launch(rtlib, gpu_ctx, r.name, r.W, r.H) == LISTS
    L, c = rtlib.lib(), gpu_ctx._c
    need = ctypes.c_size_t(0)
    assert L.rt_camera_tiles_read(c, rtlib.RT_CTILES_COUNT, None, 0, ctypes.byref(need)) == 0 and need.value == 4 * r.nt
    assert L.rt_camera_tiles_read(c, rtlib.RT_CTILES_ENTRIES, None, 0, ctypes.byref(need)) == 0 and need.value == 8 * r.nt * r.cap
    assert L.rt_camera_tiles_read(c, rtlib.RT_CTILES_SPHERES, None, 0, ctypes.byref(need)) == 0 and need.value == 16 * r.info["n"]
    buf = np.full(4 * r.nt, 0x5A, np.uint8)
    assert L.rt_camera_tiles_read(c, rtlib.RT_CTILES_COUNT, buf.ctypes.data, 4 * r.nt - 1, None) == rtlib.RT_ERR_ARG
    assert (buf == 0x5A).all()  # nothing copied
    assert L.rt_camera_tiles_read(c, rtlib.RT_CTILES_COUNT, buf.ctypes.data, 4 * r.nt, None) == 0
    assert np.array_equal(buf.view("<i4"), r.arr["COUNT"])
    assert L.rt_camera_tiles_read(c, rtlib.RT_CTILES_MASK, None, 0, ctypes.byref(need)) == rtlib.RT_ERR_STATE
    assert L.rt_camera_tiles_read(c, 5, None, 0, ctypes.byref(need)) == rtlib.RT_ERR_ARG
    assert L.rt_camera_tiles_read(c, -1, None, 0, ctypes.byref(need)) == rtlib.RT_ERR_ARG
    assert L.rt_camera_tiles_get_info(c, None) == rtlib.RT_ERR_ARG
