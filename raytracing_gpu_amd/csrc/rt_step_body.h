// rt_step_body.h -- internal: the text of render_step_kernel (rt_kernels.hip), from the LDS staging to the
// wave's counter sums.  Not a header in the usual sense: rt_kernels.hip includes it as the body of the
// kernel and of its twin general::render_step_kernel, with RT_STEP_BODY_PLAIN defined as the constant that
// says which body this is (RT_STEP_PLAIN there: which launches run which, and why their frame buffers are
// the same bits).  The text is shared as text, not as a function template, so that a kernel compiles to
// the machine code it had when the text stood in it (scripts/isa_same.py).  In scope: F, P.
// Three blocks of a shading pass that run at more than one place are fragments of their own, for the same
// reason: rt_step_body_heavy.h, rt_step_body_end.h, rt_step_body_query.h.
#ifndef RT_STEP_BODY_PLAIN
#error "rt_step_body.h is the body of render_step_kernel only"
#endif
  const DScene& S = P.S;
  if constexpr ((F & F_LDS) != 0) stage_lds<F>(S);  // nodes, primitives, margins, materials, textures
  if constexpr ((F & F_QLDS) != 0) {  // the quantized traversal tree (24-byte pair records)
    uint32_t* q = (uint32_t*)rt_lds;
    for (int k = threadIdx.x; k < 6 * S.q_pairs; k += render_block<F>()) q[k] = S.qnodes[k];
    // ... and after its stacks the materials, textures and images (lds_mats / lds_texs / lds_imgs)
    float4* m = rt_lds + qlds_mats_at(S);
    const int nm = S.lds_mats, nt = 2 * S.lds_texs, ni = S.lds_imgs;
    for (int k = threadIdx.x; k < nm + nt + ni; k += render_block<F>())
      m[k] = k < nm ? ((const float4*)S.mats)[k]
                    : (k < nm + nt ? ((const float4*)S.texs)[k - nm] : ((const float4*)S.images)[k - nm - nt]);
    __syncthreads();
  }
  constexpr bool PLAIN = RT_STEP_BODY_PLAIN;
  static_assert(!PLAIN || step_has_plain(F), "the plain body hands items out of the pool");
  const unsigned lane = __lane_id();
  RT_STEP_COUNT_BEGIN();
  RT_STAMP_BEGIN();
  const rt_object obj = ro<F>(S.objects)[ro<F>(S.world)[0]];
  const int tbase = (F & F_WORLD) != 0 ? S.wt_fb : obj.c;  // traversal tree of the world's BVH / the world tree
  const float tmin = 0.001f, tmax = __builtin_inff();  // render.h:63
  long long item = -1;  // -1: no item
  bool done = false;
  int mode = 0;  // 0: between queries, 1: traversing, 2: search ended, shading pending
  // Per-item / per-sample state, touched only between queries.  The world-tree variants (PKS) keep it
  // in an LDS locker after the stacks (word k of thread t at [k * block + t]; the RNG state
  // lane-contiguous after them) instead of VGPRs, which the traversal loop needs (C5: the variant
  // needs ~190 VGPRs otherwise, far above the 128 of 4 waves/SIMD); their REF camera offsets come
  // from cam_tab, as in render_kernel, instead of a camera RNG copy, and so do the sphere variants'
  // (TAB below).
  constexpr bool PKS = step_parks_mask(F);
  constexpr int LB = render_block<F>();
  uint32_t* const lk = (uint32_t*)rt_lds + LB * kStackDepth + threadIdx.x;
  int f_r = 0, i_r = 0, r_r = 0, j_r = 0, s_r = 0, depth_r = 0, ck_r = -1, lng_r = 0, fresh_r = 0;
  unsigned nseg_r = 0, nsamp_r = 0, item_segs_r = 0;
  int& f = cold_ref<PKS>(f_r, lk + 0 * LB);
  int& i = cold_ref<PKS>(i_r, lk + 1 * LB);
  int& r = cold_ref<PKS>(r_r, lk + 2 * LB);
  int& j = cold_ref<PKS>(j_r, lk + 3 * LB);
  int& s = cold_ref<PKS>(s_r, lk + 4 * LB);
  int& depth = cold_ref<PKS>(depth_r, lk + 5 * LB);
  unsigned& item_segs = cold_ref<PKS>(item_segs_r, lk + 6 * LB);
  unsigned& nseg = cold_ref<PKS>(nseg_r, lk + 7 * LB);
  unsigned& nsamp = cold_ref<PKS>(nsamp_r, lk + 8 * LB);
  int& ck = cold_ref<PKS>(ck_r, lk + 9 * LB);  // split_mode 1: perm position whose sample-start states are
                                               // recorded; 2: split sample (the item ends after it)
  int& lng = cold_ref<PKS>(lng_r, lk + 10 * LB);  // the item is one of the longest of the previous launch
  int& fresh = cold_ref<PKS>(fresh_r, lk + 11 * LB);  // the item's first sample is next (camera state; !TAB)
  if constexpr (PKS) {
    nseg = 0;
    nsamp = 0;
    ck = -1;
    lng = 0;
  }
  float* const lkf = reinterpret_cast<float*>(lk);
  V att_r = mk(1, 1, 1), col_r = mk(0, 0, 0);
  auto vget = [&](V& reg, int w) -> V {
    if constexpr (PKS) return mk(lkf[w * LB], lkf[(w + 1) * LB], lkf[(w + 2) * LB]);
    else return reg;
  };
  auto vset = [&](V& reg, int w, V a) {
    if constexpr (PKS) {
      lkf[w * LB] = a.x;
      lkf[(w + 1) * LB] = a.y;
      lkf[(w + 2) * LB] = a.z;
    } else {
      reg = a;
    }
  };
  Rng loc_r{}, cam{};
  Rng& loc = cold_ref<PKS>(loc_r, (uint32_t*)rt_lds + LB * (kStackDepth + 18) + 6 * threadIdx.x);
  int s_end_r = 0;  // the lane's item ends after sample s_end - 1 (spp, or one sample of a split item)
  Ray ray{};
  V finv = mk(0, 0, 0), oi = mk(0, 0, 0);
  int cur = 0, sp = 0, best_prim = -1, best_rank = 0x7fffffff;
  int pend = 0;  // deferred leaf pass: the hit leaf child this lane carries, 0: none (leaf_vote)
  float best = 0.0f, bhi = 0.0f, second = 0.0f, qa = 0.0f, rcpa = 0.0f;
  bool overflow = false;
  unsigned nnode = 0, nprim = 0, nfall = 0;
  const bool per_pixel = P.cam_mode == RT_CAM_PER_PIXEL;
  unsigned long long chunk_base = 0;  // wave-uniform: next unclaimed item of the wave's chunk
  unsigned chunk_left = 0;
  // The item pool (step_pools): lane L holds the decoded entry of position L of the wave's chunk -- the
  // item, (f, i) and (r, j) as 16-bit halves, the slot's six state words; the last chunk_left entries
  // (lanes kChunk - chunk_left on, positions chunk_base on) are not handed out yet.
  constexpr bool POOL = step_pools<F>();
  static_assert(!POOL || kChunk == 64, "the item pool holds one entry per lane");
  uint32_t pl_item = 0, pl_fi = 0, pl_rj = 0, pl_s0 = 0, pl_s1 = 0, pl_s2 = 0, pl_s3 = 0, pl_s4 = 0, pl_s5 = 0;
  // what the packed words hold; anything else decodes per lane (wave-uniform, constant over the launch)
  const bool pool_fits = PLAIN || (POOL && step_plain_launch(P));
  // split state: no lane of a plain launch has any
  constexpr bool SPLIT = !PLAIN;
  // REF camera of the sphere variants (step_sphere): the lens offset and time of sample s from cam_tab[s],
  // as in camera_ray, so these variants hold neither `cam` nor `fresh` and run no disk loop in REF mode.
  // The entry is read where s is set (the sample end, the hand-out of an item), ahead of the refill; the
  // camera setup of the same pass consumes it (cam_e).
  constexpr bool TAB = step_sphere(F);
  // The miss-first pass order of the sphere variants (step_miss_first in rt_kernels.hip): blocks A, R, Q, C
  // below.  Lanes share no state and each runs its own float operations and RNG draws in its own order, so
  // only the interleaving between lanes differs from the parent's order.
  constexpr bool MF = step_miss_first<F>();
  RT_WAVE_T0();

  const RenderParams& P0 = P;
  for (;;) {
    // Shading passes: a camera ray answered by its tile's candidate list (mode 2 right after the
    // setup) is shaded in another pass of the same phase, so the traversal loop that follows
    // starts with every lane traversing.  (The miss-first order shades it in block C of the pass that set
    // it up; what its passes leave pending -- listed camera misses, paths that ended in C -- waits through
    // the traversal loop.)
    // Invariants of both orders: the traversal loop starts with no lane holding an untested leaf and `pend`
    // is not live across the phase (the loop's flush pass tests every leaf held before it breaks, and no
    // pass touches `pend`); item_segs and nseg grow once per segment; in split launches a lane writes its
    // `ckpt` record at the same point of its own sequence (the camera setup of sample s > 0, the item's
    // end) with the same `loc` and item_segs, whichever pass that point falls into.
    for (int pass = 0;; ++pass) {
      // The arguments that only the shading passes read (the frame buffer and its layout, spp, max_depth,
      // the image size, the background, the tile lists, the camera, the work counter and the item decode's
      // words, the optional pointers) are re-read from the argument segment where a pass uses them, in the
      // variants of shade_params, instead of being parked in lanes across the traversal loop.  What the
      // traversal steps read too stays in SGPRs: S (the scene's pointers and LDS offsets), tbase, shade_min.
      const RenderParams& P = shade_params<F, PLAIN>(P0);
      const rt_camera& C = P.S.cam;
      RT_STEP_COUNT(2);
      RT_STEP_PASS_RUN(pass);
      float4 cam_e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // TAB: cam_tab[s] of a lane whose sample starts in this pass
      // MF: cam_e holds the lane's entry.  A path that ends in block C sets s after this pass's camera
      // setup; its entry is read at the setup of a later pass instead (rare: no scatter, the depth limit).
      bool cam_have = false;
      // The blocks of a pass are text fragments (rt_step_body_heavy.h, _end.h, _query.h), each written once
      // and included where an order runs it: as lambdas they changed the machine code of the mesh and world-tree variants too.
      // ---- shading phase
      RT_STAMP(7);  // back-to-back pair: phase 7 = the cost of one stamp per loop trip
      RT_STAMP(MF ? 0 : 5);
      if constexpr (MF) {
        // ---- A. end the certain misses (step_sure_miss: bvh_settle would return false at once and draws
        // nothing): one segment, att * bg, the sample end.  Every other waiting lane, an overflowed or
        // uncertain search included, is left for C.  item_segs and nseg grow once per segment: here or at
        // the head of the heavy block, never both -- C takes !step_sure_miss() only, and a lane that A ends
        // leaves mode 2.
        if (mode == 2 && step_sure_miss(S, best_prim, overflow)) {
          RT_STEP_PASS_LANES(pass, 9, true);
          ++nseg;
          ++item_segs;
          const V contrib = vget(att_r, 15) * ld3(P.S.bg);
          constexpr bool END_READS_TAB = true;
#include "rt_step_body_end.h"
          mode = 0;
        }
      } else {
      if (mode == 2) {
#include "rt_step_body_heavy.h"
      }
      }
      RT_STAMP(8);
      // ---- refill lanes without an item from the wave's chunk of the work counter (one atomic
      // per kChunk items: a single counter serialises its atomics in L2)
      const unsigned long long idle = __ballot(item < 0 && !done);
      if (POOL && pool_fits && idle != 0) {  // (step_refill 1: at every idle lane)
        static_assert(!POOL || step_refill<F>() == 1, "the pooled refill runs whenever a lane is idle");
        // From the pool: the lane of rank k among the idle ones takes position chunk_base + k, as
        // claim_items hands them out.  Every lane runs the cross-lane reads (wave-uniform control flow:
        // ds_bpermute returns 0 from a lane that is off); at most two rounds, the second after a claim.
        bool want = item < 0 && !done;
        if (want) {
          RT_STEP_COUNT(8);
        }
        unsigned rk = lane_rank(idle);
        unsigned need = (unsigned)__popcll(idle);
        for (;;) {
          if (chunk_left == 0) {  // claim a chunk and decode it, one position per lane
            RT_STEP_COUNT(10);
            unsigned long long got = 0;
            if (lane == 0) got = atomicAdd(P.work, (unsigned long long)kChunk);
            chunk_base = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(got >> 32)) << 32) |
                         __builtin_amdgcn_readfirstlane((unsigned)got);
            chunk_left = kChunk;
            const unsigned long long pos = chunk_base + lane;
            if (pos < P.total_items) {
              const long long it = P.perm ? (long long)P.perm[pos] : (long long)pos;
              const long long per_row = P.per_row;  // same item order as render_kernel
              const int qi = (int)(it / per_row);
              const long long rem = it - (long long)qi * per_row;
              const int2 rj = P.row_q[qi * P.pstep];
              const int pf = (int)(rem / P.W);
              const int pi = (int)(rem - (long long)pf * P.W) * P.pstep;
              const long long id = P.fb_first + pf;
              const long long p = (long long)rj.y * P.W + pi;
              const long long slot = ((id + 1) * p + id + 1) % P.npix;  // render.h:101 (H3)
              const uint4* st = P.states + 2 * slot;
              const uint4 s0 = st[0], s1 = st[1];
              pl_item = (uint32_t)it;
              pl_fi = ((uint32_t)pf << 16) | (uint32_t)pi;
              pl_rj = ((uint32_t)rj.x << 16) | (uint32_t)rj.y;
              pl_s0 = s0.x; pl_s1 = s0.y; pl_s2 = s0.z; pl_s3 = s0.w; pl_s4 = s1.x; pl_s5 = s1.y;
            }
          }
          const unsigned take = need < chunk_left ? need : chunk_left;
          const int src = (int)(kChunk - chunk_left + rk);
          const uint32_t g_item = __shfl(pl_item, src, 64), g_fi = __shfl(pl_fi, src, 64), g_rj = __shfl(pl_rj, src, 64);
          const uint32_t g0 = __shfl(pl_s0, src, 64), g1 = __shfl(pl_s1, src, 64), g2 = __shfl(pl_s2, src, 64);
          const uint32_t g3 = __shfl(pl_s3, src, 64), g4 = __shfl(pl_s4, src, 64), g5 = __shfl(pl_s5, src, 64);
          if (want && rk < take) {
            const unsigned long long pos = chunk_base + rk;
            if (pos >= P.total_items) {
              done = true;
              RT_WAVE_EXHAUSTED();
            } else {
              item = (long long)g_item;
              lng = pos < P.n_long ? 1 : 0;
              f = (int)(g_fi >> 16);
              i = (int)(g_fi & 0xffffu);
              r = (int)(g_rj >> 16);
              j = (int)(g_rj & 0xffffu);
              loc.d = g0; loc.v[0] = g1; loc.v[1] = g2; loc.v[2] = g3; loc.v[3] = g4; loc.v[4] = g5;
              s = 0;
              if constexpr (!PLAIN) s_end_r = P.spp;
              if constexpr (!TAB) fresh = 1;
              if (TAB && !per_pixel) {
                cam_e = P.S.cam_tab[0];
                cam_have = true;
              }
              depth = 0;
              item_segs = 0;
              col_r = mk(0, 0, 0);
            }
            want = false;
          }
          rk -= take;
          chunk_base += take;
          chunk_left -= take;
          need -= take;
          if (need == 0) break;
        }
      }
      if ((!POOL || !pool_fits) && idle != 0 && (__popcll(idle) >= step_refill<F>() || __ballot(item >= 0) == 0)) {
        const unsigned long long mine = claim_items(P.work, idle, chunk_base, chunk_left);
        if (item < 0 && !done) {
          RT_STEP_COUNT(8);
          if (mine >= P.total_items) {
            done = true;
            RT_WAVE_EXHAUSTED();
          } else {
            unsigned long long pos = mine;
            int sa = 0;
            ck = -1;
            if (P.split_mode == 2) {  // split samples first, then the rest of perm
              const unsigned long long nsub = P.n_split * (unsigned long long)P.spp;
              const unsigned long long v = P.order ? (unsigned long long)P.order[mine] : mine;
              if (v < nsub) {
                pos = v / (unsigned)P.spp;
                sa = (int)(v - pos * (unsigned)P.spp);
                ck = (int)v;
              } else {
                pos = v - nsub + P.n_split;
              }
            } else if (P.split_mode == 1 && mine < P.n_split) {
              ck = (int)mine;
            }
            item = P.perm ? (long long)P.perm[pos] : (long long)pos;
            lng = pos < P.n_long ? 1 : 0;
            const long long per_row = P.per_row;  // same item order as render_kernel
            const int qi = (int)(item / per_row);
            const long long rem = item - (long long)qi * per_row;
            const int2 rj = P.row_q[qi * P.pstep];
            r = rj.x;
            f = (int)(rem / P.W);
            i = (int)(rem - (long long)f * P.W) * P.pstep;
            j = rj.y;
            const long long id = P.fb_first + f;
            const long long p = (long long)j * P.W + i;
            const long long slot = ((id + 1) * p + id + 1) % P.npix;  // render.h:101 (H3)
            const uint4* st = sa > 0 ? P.ckpt + 2 * (long long)ck : P.states + 2 * slot;
            const uint4 s0 = st[0], s1 = st[1];
            loc.d = s0.x; loc.v[0] = s0.y; loc.v[1] = s0.z; loc.v[2] = s0.w; loc.v[3] = s1.x; loc.v[4] = s1.y;
            s = sa;
            if constexpr (!PKS) s_end_r = (P.split_mode == 2 && ck >= 0) ? sa + 1 : P.spp;
            if constexpr (!TAB) fresh = 1;
            if (TAB && !per_pixel) {  // (a split sample needs no camera state)
              cam_e = P.S.cam_tab[sa];
              cam_have = true;
            }
            depth = 0;
            item_segs = 0;
            vset(col_r, 12, mk(0, 0, 0));
          }
        }
      }
      // Waves holding one of the longest items (processed first) issue ahead of the others, so the
      // long items of a small multi-GPU share are not the last to finish.
      if (P.n_long > 0) {
        if (__ballot(item >= 0 && lng != 0) != 0) __builtin_amdgcn_s_setprio(3);
        else __builtin_amdgcn_s_setprio(0);
      }
      // ---- next query: camera ray at a sample's start (render.h:105-108, camera.h:49-58)
      RT_STAMP(1);
      // (Q of the miss-first order: there every lane that comes here starts a sample, a scattered ray's
      // search having started in C.)
      if (item >= 0 && mode == 0) {
        RT_STEP_PASS_LANES(pass, 6, MF || depth == 0);
        // camera ray: its tile's candidate list (count + first entries) is loaded before the ray is
        // generated, so the loads overlap the camera arithmetic
        const bool listed = (F & F_WORLD) == 0 && depth == 0 && P.tile_cnt != nullptr;
        const int32_t* ent = nullptr;
        int tcnt = -1;
        int4 g0 = make_int4(0, 0, 0, 0);
        if (listed) {
          const int t = (j >> kTileShift) * P.tiles_x + (i >> kTileShift);
          ent = P.tile_ent + (size_t)t * P.tile_cap * 2;  // (id, nearest) pairs
          tcnt = P.tile_cnt[t];
          g0 = *reinterpret_cast<const int4*>(ent);
        }
        if (depth == 0 && PKS) {
          if (P.split_mode == 1 && ck >= 0 && s > 0) {  // record the sample-start state for split launches
            uint4* dst = P.ckpt + 2 * ((long long)ck * P.spp + s);
            dst[0] = make_uint4(loc.d, loc.v[0], loc.v[1], loc.v[2]);
            dst[1] = make_uint4(loc.v[3], loc.v[4], item_segs, 0u);
          }
          Rng lr = loc;
          camera_ray(P, C, i, j, s, per_pixel, lr, ray);  // REF offsets from cam_tab
          loc = lr;
          vset(att_r, 15, mk(1.0f, 1.0f, 1.0f));
        } else if (TAB && depth == 0) {
          // camera_ray's text with the table entry read ahead; PER_PIXEL draws from loc exactly as the
          // branch below does (jitter, disk, time: render.h:105-108 order)
          if (SPLIT && P.split_mode == 1 && ck >= 0 && s > 0) {  // record the sample-start state for split launches
            uint4* dst = P.ckpt + 2 * ((long long)ck * P.spp + s);
            dst[0] = make_uint4(loc.d, loc.v[0], loc.v[1], loc.v[2]);
            dst[1] = make_uint4(loc.v[3], loc.v[4], item_segs, 0u);
          }
          const float u = ((float)i + rtx::uniform(loc)) / (float)P.W;
          const float v = ((float)j + rtx::uniform(loc)) / (float)P.H;
          V off;
          if (per_pixel) {
            const V rd = C.lens_radius * in_unit_disk(loc);
            off = rd.x * ld3(C.u) + rd.y * ld3(C.v);
            ray.tm = urange(loc, C.time0, C.time1);
          } else {
            if constexpr (MF)
              if (!cam_have) cam_e = P.S.cam_tab[s];  // the sample before this one ended in C: s < spp, the item goes on
            off = mk(cam_e.x, cam_e.y, cam_e.z);
            ray.tm = cam_e.w;
          }
          ray.o = ld3(C.origin) + off;
          ray.d = ld3(C.lower_left) + u * ld3(C.horizontal) + v * ld3(C.vertical) - ld3(C.origin) - off;
          vset(att_r, 15, mk(1.0f, 1.0f, 1.0f));
        } else if (depth == 0) {
          // REF: the step kernel draws the per-sample lens offset and time from its own copy of the
          // pristine slot-0 state instead of cam_tab: the mesh variants only.  (The sphere variants take the
          // branch above: there the table read, issued early, measured 3.3 % faster than the copy, DESIGN.md
          // 3.1j.)
          if (fresh && !per_pixel) {
            if (s == 0) {
              cam.d = P.cam_state[0];
              for (int k = 0; k < 5; ++k) cam.v[k] = P.cam_state[1 + k];
            } else {  // a split sample: the camera state at its start
              const uint4 c0 = P.cam_st[2 * s], c1 = P.cam_st[2 * s + 1];
              cam.d = c0.x; cam.v[0] = c0.y; cam.v[1] = c0.z; cam.v[2] = c0.w; cam.v[3] = c1.x; cam.v[4] = c1.y;
            }
          }
          fresh = 0;
          if (SPLIT && P.split_mode == 1 && ck >= 0 && s > 0) {  // record the sample-start state for split launches
            uint4* dst = P.ckpt + 2 * ((long long)ck * P.spp + s);
            dst[0] = make_uint4(loc.d, loc.v[0], loc.v[1], loc.v[2]);
            dst[1] = make_uint4(loc.v[3], loc.v[4], item_segs, 0u);
          }
          const float u = ((float)i + rtx::uniform(loc)) / (float)P.W;
          const float v = ((float)j + rtx::uniform(loc)) / (float)P.H;
          Rng& cr = per_pixel ? loc : cam;
          const V rd = C.lens_radius * in_unit_disk(cr);
          const V off = rd.x * ld3(C.u) + rd.y * ld3(C.v);
          ray.o = ld3(C.origin) + off;
          ray.d = ld3(C.lower_left) + u * ld3(C.horizontal) + v * ld3(C.vertical) - ld3(C.origin) - off;
          ray.tm = urange(cr, C.time0, C.time1);
          vset(att_r, 15, mk(1.0f, 1.0f, 1.0f));
        }
#include "rt_step_body_query.h"
        if constexpr ((F & F_WORLD) == 0) {
          if (listed && tcnt >= 0) {  // camera ray: the tile's candidate list instead of the tree
            tile_candidates<F>(S, ent, tcnt, g0, ray, qa, rcpa, tmin, tmax, best, bhi, second, best_prim, best_rank,
                               nprim);
            mode = 2;
            RT_STEP_PASS_LANES(pass, 7, best_prim >= 0);
            RT_STEP_PASS_LANES(pass, 8, best_prim < 0);
          }
        }
      }
      if constexpr (MF) {
        // ---- C. the heavy block, once per pass: bounce hits, camera rays whose list holds a candidate,
        // and the searches A declined (overflow; a world with entries after its BVH).  A camera ray whose
        // list gave none is a certain miss: it keeps mode 2 for block A of the next phase and waits through
        // the traversal loop as a listed camera ray does in the parent's order after the last pass.
        // No ray is copied here or anywhere in the pass: a lane's ray is written in place by Q or by
        // scatter ("the conditional ray copy").
        RT_STAMP(5);
        if (mode == 2 && !step_sure_miss(S, best_prim, overflow)) {
#include "rt_step_body_heavy.h"
        }
        // ---- one pass per phase (rt_kernels.hip, at step_miss_first: more passes measured slower).  Left
        // pending: those camera misses, and the paths that ended inside C (mode 0, not done: with an item
        // whose next sample starts, or without one).
        break;
      } else {
        if (pass + 1 >= kShadePasses || __ballot(mode == 2) == 0) break;
      }
    }
    RT_STAMP(3);
    // Lanes a path's end in C left between queries (MF only: in the parent's order every lane leaves the
    // passes traversing, waiting with mode 2, or done) wait through the traversal loop like mode 2 lanes.
    // Wave-uniform and constant over the loop, which moves lanes from mode 1 to mode 2 only.
    int wait0 = 0;
    if constexpr (MF) wait0 = __popcll(__ballot(mode == 0 && !done));
    if (__ballot(MF ? mode != 0 || !done : mode != 0) == 0) break;  // no item left for any lane of the wave (mode 2: a listed camera ray)
    // ---- traversal steps until shade_min lanes wait (or none traverses)
    for (;;) {
      RT_STEP_COUNT(3);
      // several traversal steps per check of the shading condition, same VGPRs (same box, Mrays/s at
      // 1 / 2 / 3 / 4 steps: C2 14 538 / 14 713 / 14 829 / 14 843, C4 11 180 / 11 247 (before the
      // triangle dedupe) and 14 095 / 14 051 / 13 990 after it); the opt-in world-tree variants keep
      // one (more spills with two)
      // (with the deferred leaf pass, C2 at 2 / 4 / 6 / 8 steps: 16.10 / 15.82 / 15.87 / 15.99 ms)
      constexpr int kUnroll = (F & F_WORLD) != 0 ? 1 : ((F & F_TRI) != 0 ? 2 : 4);
      if constexpr (leaf_pass_min(F) > 0) {
        // deferred leaf pass (leaf_vote): a lane whose search ends holding a leaf waits like any
        // other, and a flush pass before the shading phase tests every leaf still held, so no lane
        // settles with a leaf untested and `pend` is not live across the phase
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          int n0 = 0, n1 = 0;
          if (mode == 1) {
            RT_STEP_COUNT(0);
            if (!trav_node<F>(S, tbase, oi, finv, tmin, tmax, bhi, cur, sp, overflow, nnode, n0, n1)) mode = 2;
          }
          leaf_vote<F>(S, false, pend, n0, n1, ray, qa, rcpa, tmin, tmax, best, bhi, second, best_prim, best_rank,
                       nprim);
        }
        // (the threshold as a kernel argument measured 1.5 % faster than the compile-time constant)
        if (__ballot(mode == 1) == 0 || __popcll(__ballot(mode == 2)) + wait0 >= P.shade_min) {
          leaf_vote<F>(S, true, pend, 0, 0, ray, qa, rcpa, tmin, tmax, best, bhi, second, best_prim, best_rank,
                       nprim);
          break;
        }
      } else {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
        if (mode == 1) {
          RT_STEP_COUNT(0);
          if (!trav_step<F>(S, tbase, ray, oi, finv, qa, rcpa, tmin, tmax, cur, sp, best, bhi, second, best_prim,
                            best_rank, overflow, nnode, nprim))
            mode = 2;
        }
        // (the threshold as a kernel argument measured 1.5 % faster than the compile-time constant)
        if (__ballot(mode == 1) == 0 || __popcll(__ballot(mode == 2)) + wait0 >= P.shade_min) break;
      }
    }
  }

  RT_STEP_COUNT_END();
  RT_STAMP_END();
  RT_WAVE_END();
  const unsigned long long ws = wave_sum(nseg), wm = wave_sum(nsamp);
  unsigned long long wn = 0, wp = 0, wf = 0;
  if constexpr ((F & F_STATS) != 0) {
    wn = wave_sum(nnode);
    wp = wave_sum(nprim);
    wf = wave_sum(nfall);
  }
  if (lane == 0) {
    atomicAdd(&P.counters[0], ws);
    atomicAdd(&P.counters[3], wm);
    if constexpr ((F & F_STATS) != 0) {
      atomicAdd(&P.counters[1], wn);
      atomicAdd(&P.counters[2], wp);
      atomicAdd(&P.counters[4], wf);
    }
  }
