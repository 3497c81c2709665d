"""The adaptive accumulator (rt_adapt_* of include/rt_hip.h) as a numpy model, shared by
tests/test_adapt_cpu.py and tests/test_adapt_gpu.py.  It is fed the 8-bit planes c = quant(fb) of
every frame buffer and a list of steps, and keeps per value what the device keeps: the float32 sum
(accum_add_kernel's operations in fb order), the integer moments S1 and S2, and per 16 x 16 tile n_t
and an active flag.  The noise formula is tests/noise_ref.py's."""
import numpy as np

import noise_ref as nr

TILE = nr.TILE


def quant(x):
    """write_frame_buffer's quantisation of float32 values (color.h:40-44), NaN as 0."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.sqrt(x)
    r = np.where(np.isnan(r), np.float32(0), r)
    c = np.clip(r, np.float32(0), np.float32(0.999)).astype(np.float32)
    return (np.float32(256.0) * c).astype(np.int32)


def tile_grid(rows, width):
    return (rows + TILE - 1) // TILE, (width + TILE - 1) // TILE


def pixel_tiles(rows, width):
    """[rows][width] tile id of every pixel."""
    ty, tx = tile_grid(rows, width)
    return (np.arange(rows)[:, None] // TILE) * tx + np.arange(width)[None, :] // TILE


def run(planes, rows, width, steps):
    """planes: [nfb][rows*width*3] integers 0..255 in the frame buffers' own layout (owned rows
    ascending); steps: ("add", k) renders and folds in the next k planes for the active tiles,
    ("retire", T, max_above) retires every active tile with at most max_above pixels of noise > T.
    Returns a dict: counts int32 [ty][tx] (n_t), image uint8 [rows][width][3], noise float32
    [rows][width] (None before 2 frame buffers), reports (one dict per retire step, rt_adapt_report's
    fields), maps (the noise map at every retire step)."""
    c = np.asarray(planes).astype(np.uint64).reshape(-1, rows, width, 3)
    ty, tx = tile_grid(rows, width)
    tid = pixel_tiles(rows, width)
    n_t = np.zeros(ty * tx, np.int64)
    active = np.ones(ty * tx, bool)
    sums = np.zeros((rows, width, 3), np.float32)
    S1 = np.zeros((rows, width, 3), np.uint64)
    S2 = np.zeros((rows, width, 3), np.uint64)
    fbs = 0
    reports, maps = [], []

    def noise():
        out = np.zeros((rows, width), np.float32)
        for n in np.unique(n_t):
            m = nr.noise_map(S1.reshape(-1), S2.reshape(-1), int(n), rows, width)
            sel = n_t[tid] == n
            out[sel] = m[sel]
        return out

    for step in steps:
        if step[0] == "add":
            if not active.any():
                continue
            mask = active[tid]
            for f in range(fbs, fbs + step[1]):
                c2 = c[f] * c[f]
                sums[mask] = (sums + c2.astype(np.float32) / np.float32(255.0 * 255.0))[mask]
                S1[mask] += c2[mask]
                S2[mask] += (c2 * c2)[mask]
            fbs += step[1]
            n_t[active] = fbs
        elif step[0] == "retire":
            _, T, max_above = step
            assert fbs >= 2
            nmap = noise()
            above = np.bincount(tid.reshape(-1), (nmap > np.float32(T)).reshape(-1).astype(np.int64), ty * tx).astype(np.int64)
            active &= above > max_above
            px = np.bincount(tid.reshape(-1), minlength=ty * tx)
            reports.append({"fbs": fbs, "tiles_x": tx, "tiles_y": ty, "tiles_active": int(active.sum()),
                            "pixels": rows * width, "pixels_active": int(px[active].sum()),
                            "pixel_fbs": int((px * n_t).sum()), "pixels_above": int(above.sum()),
                            "threshold": float(np.float32(T)), "max_noise": float(nmap.max())})
            maps.append(nmap)
        else:
            raise ValueError(step)
    image = None
    if fbs:
        image = quant(sums / n_t[tid].astype(np.float32)[:, :, None]).astype(np.uint8)
    return {"counts": n_t.reshape(ty, tx).astype(np.int32), "image": image, "noise": noise() if fbs >= 2 else None,
            "reports": reports, "maps": maps, "fbs": fbs}
