"""The chain through mirrors and glass (rt_spec_* of include/rt_hip.h) restated in numpy, for
tests/test_spec_cpu.py: float32 one operation at a time, a segment being rt.cast_host (which tests/test_guide_cpu.py
pins against the oracle).  Returns the hits and paths of the definition and every segment's rays."""
from __future__ import annotations

import numpy as np

import raytracing_gpu_amd as rt

F32 = np.float32
MISS, SURFACE, ESCAPED, LIMIT, ABSORBED = range(5)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _scaled(s, v):
    return s[:, None] * v


def reflect(ud, n):
    return ud - _scaled(F32(2.0) * dot(ud, n), n)


def refract(ud, n, ratio):
    c = np.fmin(dot(-ud, n), F32(1.0))
    perp = _scaled(ratio, ud + _scaled(c, n))
    par = -np.sqrt(np.abs((1.0 - dot(perp, perp).astype(np.float64)).astype(F32)))
    return perp + _scaled(par, n)


def chain(soa, rays, max_bounces: int, max_fuzz: float, glass: int):
    """(hits, paths, segments): segments[k] = (index of the rays still alive, their segment-k rays)."""
    rays = np.ascontiguousarray(rays, F32)
    n = len(rays)
    mtype = np.array([soa.materials[i].type for i in range(soa.n_materials)], np.int32)
    mparam = np.array([soa.materials[i].param for i in range(soa.n_materials)], F32)
    hits, paths = np.zeros(n, rt.GUIDE_HIT_DTYPE), np.zeros(n, rt.SPEC_PATH_DTYPE)
    thr = np.ones((n, 3), F32)
    t0, len0, total, terms = np.zeros(n, F32), np.ones(n, F32), np.zeros(n, F32), np.zeros(n, np.int32)
    status, bounces = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    e = rays.copy()
    segments = []
    k = 0
    with np.errstate(all="ignore"):
        while (status < 0).any():
            idx = np.flatnonzero(status < 0)
            segments.append((idx, e[idx].copy()))
            h = rt.cast_host(soa, e[idx])
            d = e[idx, 3:6]
            ln = np.sqrt(dot(d, d))
            hit = h["prim"] >= 0
            if k == 0:
                hits[idx] = h
                t0[idx], len0[idx] = h["t"], ln
                paths["first_prim"][idx], paths["first_material"][idx] = h["prim"], h["material"]
                status[idx[~hit]] = MISS
            else:
                status[idx[~hit]] = ESCAPED
                hits[idx[hit]] = h[hit]
                term = h["t"] * ln
                j = idx[hit]
                total[j] = np.where(terms[j] > 0, total[j] + term[hit], term[hit])
                terms[j] += 1
            mi = np.where(hit, h["material"], 0)
            metal = hit & (mtype[mi] == rt.MAT_METAL) & (mparam[mi] <= F32(max_fuzz))
            diel = hit & (mtype[mi] == rt.MAT_DIELECTRIC) & bool(glass)
            spec = metal | diel
            status[idx[hit & ~spec]] = SURFACE
            if k == max_bounces:
                status[idx[spec]] = LIMIT
                break
            ud = _scaled(F32(1.0) / ln, d)
            nn = h["n"]
            refl = reflect(ud, nn)
            absorbed = metal & ~(dot(refl, nn) > 0)
            status[idx[absorbed]] = ABSORBED
            go = metal & ~absorbed
            thr[idx[go]] = thr[idx[go]] * h["albedo"][go]
            ratio = np.where(h["front"] != 0, F32(1.0) / mparam[mi], mparam[mi])
            ct = np.fmin(dot(-ud, nn), F32(1.0))
            st = np.sqrt(F32(1.0) - ct * ct)
            tir = ratio * st > F32(1.0)
            direction = np.where((metal | tir)[:, None], refl, refract(ud, nn, ratio))
            assert direction.dtype == F32 and ud.dtype == F32 and ratio.dtype == F32
            nxt = go | diel
            e[idx[nxt], 0:3] = h["p"][nxt]
            e[idx[nxt], 3:6] = direction[nxt]
            bounces[idx[nxt]] += 1
            k += 1
    paths["bounces"], paths["status"] = bounces, status
    paths["throughput"] = thr
    with np.errstate(all="ignore"):
        paths["depth"] = np.where(terms > 0, t0 + total / len0, t0)
    return hits, paths, segments
