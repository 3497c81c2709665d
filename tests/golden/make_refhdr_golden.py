#!/usr/bin/env python3
"""Records tests/golden/refhdr_renders.npz from oracle/_ref/libref_headers.so: the reference's own class
headers compiled for the host (oracle/refhdr/ref_headers.cpp), so it runs only where the reference is.

For every case of tests/refhdr_cases.py's RECORDED, in REF camera mode at flat_cases.py's 40 x 24, 4 spp,
2 frame buffers and the case's depth: `<case>_fb<f>` the frame buffer as uint32 bits (H, W, 3), and
`<case>_segments` the per-pixel world-query count summed over the frame buffers (H, W) int32.  The record
is data the reference's code wrote; the oracle had no part in it.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refhdr_cases  # noqa: E402
from flat_cases import NFB, REF, SPP, H, W  # noqa: E402
from oracle import ref_headers  # noqa: E402


def main() -> None:
    arrs = {}
    for key in refhdr_cases.RECORDED:
        e = refhdr_cases.recorded_entry(key)
        hs = ref_headers.HdrScene(e.scene.soa)
        segs = np.zeros((H, W), np.int32)
        for f in range(NFB):
            fb, sg = hs.render(W, H, SPP, f, e.depth, REF)
            arrs[f"{refhdr_cases.key_name(key)}_fb{f}"] = fb.view(np.uint32)
            segs += sg
        arrs[f"{refhdr_cases.key_name(key)}_segments"] = segs
    np.savez_compressed(refhdr_cases.GOLDEN, **arrs)
    size, cap = os.path.getsize(refhdr_cases.GOLDEN), os.path.getsize(os.path.join(HERE, "ref_images.npz"))
    print(f"wrote {refhdr_cases.GOLDEN}: {size} bytes (ref_images.npz: {cap})")
    assert size <= cap, "larger than ref_images.npz: record one frame buffer per case"


if __name__ == "__main__":
    main()
