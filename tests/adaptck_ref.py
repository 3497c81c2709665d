"""The adaptive accumulator with checkpoints, reopening and dilation (rt_adaptive_* of include/rt_hip.h)
as a numpy model, shared by tests/test_adaptck_cpu.py and tests/test_adaptck_gpu.py.  It extends
tests/adapt_ref.py's model (same planes, same float32 sums in fb order, same integer moments, the noise
formula of tests/noise_ref.py) by what the new calls add: tiles that fold from their own n_t, the limit of
an add, the Chebyshev dilation of retire and reopen, and the checkpoint blob packed and unpacked."""
import struct

import numpy as np

import adapt_ref as ar
import noise_ref as nr

TILE = nr.TILE
HEADER = nr.HEADER
MAX_FBS = nr.MAX_FBS
MAGIC = b"RTADAPT1"
ARG_FIELDS = ("width", "height", "spp", "fb_first", "fb_count", "max_depth", "cam_mode", "band_rows", "band_first",
              "band_stride", "stats", "flags")


def dilate(mask, r):
    """mask [ty][tx] bool -> the tiles within Chebyshev distance r of a set one."""
    mask = np.asarray(mask, bool)
    out = np.zeros_like(mask)
    for y, x in zip(*np.nonzero(mask)):
        out[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    return out


class Model:
    """planes: [nfb][rows*width*3] integers 0..255, plane f = c of frame buffer fb_first + f (owned rows
    ascending).  State as the device keeps it: n_t and active per tile, per value the float32 sum and the
    uint64 moments."""

    def __init__(self, planes, rows, width):
        self.c = np.asarray(planes).astype(np.uint64).reshape(-1, rows, width, 3)
        self.rows, self.width = rows, width
        self.ty, self.tx = ar.tile_grid(rows, width)
        self.tid = ar.pixel_tiles(rows, width)
        n = self.ty * self.tx
        self.n_t = np.zeros(n, np.int64)
        self.active = np.ones(n, bool)
        self.sums = np.zeros((rows, width, 3), np.float32)
        self.S1 = np.zeros((rows, width, 3), np.uint64)
        self.S2 = np.zeros((rows, width, 3), np.uint64)
        self.px = np.bincount(self.tid.reshape(-1), minlength=n)

    @property
    def fbs(self):
        return int(self.n_t.max())

    def add(self, count, limit=MAX_FBS):
        """Every active tile receives min(count, limit - n_t) planes from its own n_t on; returns the
        number of (pixel, frame buffer) pairs rendered."""
        assert count >= 1 and limit >= 1
        work = 0
        start = self.n_t.copy()  # a tile belongs to the group of the n_t it starts the call with
        for n in np.unique(start[self.active]):
            give = min(count, limit - int(n))
            if give <= 0:
                continue
            group = self.active & (start == n)
            mask = group[self.tid]
            for f in range(int(n), int(n) + give):
                c2 = self.c[f] * self.c[f]
                self.sums[mask] = (self.sums + c2.astype(np.float32) / np.float32(255.0 * 255.0))[mask]
                self.S1[mask] += c2[mask]
                self.S2[mask] += (c2 * c2)[mask]
            self.n_t[group] = n + give
            work += int(self.px[group].sum()) * give
        return work

    def noise(self):
        out = np.zeros((self.rows, self.width), np.float32)
        for n in np.unique(self.n_t):
            assert n >= 2
            m = nr.noise_map(self.S1.reshape(-1), self.S2.reshape(-1), int(n), self.rows, self.width)
            sel = self.n_t[self.tid] == n
            out[sel] = m[sel]
        return out

    def above(self, T):
        nmap = self.noise()
        hot = (nmap > np.float32(T)).reshape(-1).astype(np.int64)
        return nmap, np.bincount(self.tid.reshape(-1), hot, self.ty * self.tx).astype(np.int64)

    def tile_max(self):
        return nr.tiles(self.noise(), 0.0)[0]

    def report(self, T):
        nmap, above = self.above(T)
        return {"fbs": self.fbs, "tiles_x": self.tx, "tiles_y": self.ty, "tiles_active": int(self.active.sum()),
                "pixels": self.rows * self.width, "pixels_active": int(self.px[self.active].sum()),
                "pixel_fbs": int((self.px * self.n_t).sum()), "pixels_above": int(above.sum()),
                "threshold": float(np.float32(T)), "max_noise": float(nmap.max())}

    def retire(self, T, max_above=0, r=0):
        assert self.fbs >= 2 and r >= 0
        _, above = self.above(T)
        failing = self.active & (above > max_above)
        self.active &= dilate(failing.reshape(self.ty, self.tx), r).reshape(-1)
        return self.report(T)

    def reopen(self, T, max_above=0, r=0):
        assert self.fbs >= 2 and r >= 0
        _, above = self.above(T)
        self.active |= dilate((above > max_above).reshape(self.ty, self.tx), r).reshape(-1)
        return self.report(T)

    def counts(self):
        return self.n_t.reshape(self.ty, self.tx).astype(np.int32)

    def flags(self):
        return self.active.reshape(self.ty, self.tx).copy()

    def image(self):
        return ar.quant(self.sums / self.n_t[self.tid].astype(np.float32)[:, :, None]).astype(np.uint8)

    def pack(self, info):
        """The checkpoint blob of this state; info: dict of the header's fields but fb_count and n_values."""
        return pack(info, self.n_t, self.active, self.sums, self.S1, self.S2)


def fnv1a(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def header(info, n_values, fb_count, payload_hash):
    f = dict(info, fb_count=fb_count)
    return (MAGIC + struct.pack("<II", 1, HEADER) + struct.pack("<12i", *[f[k] for k in ARG_FIELDS]) +
            struct.pack("<QqQQ", f["seed"], n_values, f["scene_fp"], payload_hash))


def payload(n_t, active, sums, S1, S2):
    out = np.asarray(n_t).astype("<i4").tobytes() + np.asarray(active).astype(np.uint8).tobytes()
    out += b"\0" * (-(HEADER + len(out)) % 8)
    out += np.asarray(sums, np.float32).astype("<f4").tobytes()
    out += b"\0" * (-(HEADER + len(out)) % 8)
    return out + np.asarray(S2).astype("<u8").tobytes() + np.asarray(S1).astype("<u4").tobytes()


def pack(info, n_t, active, sums, S1, S2, fb_count=None):
    body = payload(n_t, active, sums, S1, S2)
    return header(info, int(np.asarray(sums).size), int(np.max(n_t)) if fb_count is None else fb_count, fnv1a(body)) + body


def rehash(blob):
    """blob with its payload hash recomputed (for a blob edited on purpose)."""
    return blob[:88] + struct.pack("<Q", fnv1a(blob[HEADER:])) + blob[HEADER:]


def layout(n_values, tiles):
    """Byte offsets of a blob's sections: n_t, active, pad0, sums, pad1, S2, S1, total."""
    n_t = HEADER
    active = n_t + 4 * tiles
    pad0 = active + tiles
    sums = (pad0 + 7) // 8 * 8
    pad1 = sums + 4 * n_values
    s2 = (pad1 + 7) // 8 * 8
    s1 = s2 + 8 * n_values
    return {"n_t": n_t, "active": active, "pad0": pad0, "sums": sums, "pad1": pad1, "S2": s2, "S1": s1, "total": s1 + 4 * n_values}


def unpack(blob, n_values, tiles):
    l = layout(n_values, tiles)
    assert len(blob) == l["total"]
    return {"n_t": np.frombuffer(blob, "<i4", tiles, l["n_t"]).astype(np.int64),
            "active": np.frombuffer(blob, np.uint8, tiles, l["active"]).astype(bool),
            "sums": np.frombuffer(blob, "<f4", n_values, l["sums"]).copy(),
            "S2": np.frombuffer(blob, "<u8", n_values, l["S2"]).copy(),
            "S1": np.frombuffer(blob, "<u4", n_values, l["S1"]).astype(np.uint64)}


def midpoints(values):
    """float32 thresholds midway between adjacent distinct values of `values` that lie at least 8 ulp apart,
    ascending: a decision against one of them cannot depend on an ulp of a value."""
    v = np.unique(np.asarray(values, np.float32))
    out = []
    for a, b in zip(v[:-1], v[1:]):
        if nr.ulps(b) - nr.ulps(a) >= 8:
            t = np.float32((np.float64(a) + np.float64(b)) / 2)
            assert a < t < b
            out.append(float(t))
    return out


def clear_of(T, maps, ulp=2):
    """No value of the noise maps lies within `ulp` ulp of the threshold T."""
    t = nr.ulps(np.float32(T))
    return all(int(np.abs(nr.ulps(m) - t).min()) > ulp for m in maps)
