#!/usr/bin/env python3
"""Exhaustive check of the device probe: every one of the 2^32 float bit patterns through det_sinf, det_cosf,
det_tanf, det_logf, det_pow5f, det_acosf and quant, hipcc's device pass against hipcc's host pass
(oracle/devprobe.py; tests/test_devprobe_gpu.py is the strided version of this).  Two NaNs count as equal and
are counted apart where their bits differ.  The host side runs on --threads threads (at most 16); minutes.

usage: check_detmath_device.py [--fn NAME ...] [--threads 16] [--chunk-bits 26] [--json OUT]
(scripts/check_checker_sign.cpp is the same kind of run for sin_neg_fast, on the CPU alone.)
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import devprobe as dp  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--fn", nargs="*", default=list(dp.UNARY))
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--chunk-bits", type=int, default=26)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    threads = max(1, min(16, a.threads))
    chunk = 1 << a.chunk_bits
    part = chunk // threads
    assert part * threads == chunk or threads == 1, "--threads must divide the chunk"
    dev, host = np.empty(chunk, np.uint32), np.empty(chunk, np.uint32)
    result = {}
    bad_total = 0
    with ThreadPoolExecutor(threads) as pool:
        for fn in a.fn:
            t0 = time.time()
            differ = nan_pairs = nan_other_bits = 0
            first = []
            for base in range(0, 1 << 32, chunk):
                # ctypes releases the GIL: the host pass of this chunk runs beside the device's
                jobs = [pool.submit(dp.unary_range, "host", fn, base + k * part, part, host[k * part:(k + 1) * part])
                        for k in range(threads)]
                dp.unary_range("dev", fn, base, chunk, dev)
                for j in jobs:
                    j.result()
                ne = dev != host
                if ne.any():
                    idx = np.nonzero(ne)[0]
                    d, h = dev[idx], host[idx]
                    both_nan = ((d & 0x7FFFFFFF) > 0x7F800000) & ((h & 0x7FFFFFFF) > 0x7F800000)
                    nan_other_bits += int(both_nan.sum())
                    differ += int((~both_nan).sum())
                    for i in idx[~both_nan][: max(0, 8 - len(first))]:
                        first.append({"x": f"{base + int(i):#010x}", "device": f"{int(dev[i]):#010x}", "host": f"{int(host[i]):#010x}"})
                if fn != "quant":
                    nan_pairs += int(((host & 0x7FFFFFFF) > 0x7F800000).sum())
            result[fn] = {"checked": 1 << 32, "differ": differ, "nan_results": nan_pairs, "nan_with_other_bits": nan_other_bits,
                          "first": first, "seconds": round(time.time() - t0, 1)}
            bad_total += differ
            print(f"{fn}: checked {1 << 32} bit patterns, device != host pass at {differ}, NaN results {nan_pairs} "
                  f"(of them with other bits on the device {nan_other_bits}), {time.time() - t0:.1f} s", flush=True)
            for e in first:
                print(f"  x {e['x']} device {e['device']} host {e['host']}", flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(result, fh, indent=1)
    return 1 if bad_total else 0


if __name__ == "__main__":
    sys.exit(main())
