// rt_step_body_heavy.h -- internal: a fragment of rt_step_body.h, shared as text for the reason given there.
// The heavy block of a shading pass: finish an ended query (render.h:60-77) -- settle the search, the
// trailing primitive entries, the hit record, scatter -- for the lanes the includer's `if` lets in.  The
// parent's order runs it at the head of a pass for every waiting lane and leaves mode = 0.  The miss-first
// order (MF) runs it after the camera setup, as block C, for the lanes block A left, and starts a scattered
// ray's search right here (mode = 1); a path that ends here (no scatter, the depth limit, an exact fallback
// that misses, a miss A declined) is left with mode = 0 for a later pass.
#ifndef RT_STEP_BODY_PLAIN
#error "rt_step_body_heavy.h is a fragment of rt_step_body.h"
#endif
        RT_STEP_PASS_LANES(pass, 1, true);
        ++nseg;
        ++item_segs;
        bool ended = false;
        V contrib;
        Hit h;
        bool hit;
        if constexpr ((F & F_WORLD) != 0) {
          // list world: the tree's winner, then the constant media that follow every tree entry in
          // the list, in list order with the closest hit so far (their RNG draws depend on it);
          // anything uncertain -- near ties, a chain the reference may reject, a ray that could
          // make an inert medium draw -- runs the reference's sequential list exactly
          constexpr int FM = F & ~(F_WORLD | F_STEP | F_BVH);  // media boundaries are primitives
          int wobj = -1, wprim = -1;
          int st = world_settle<F>(S, ray, tmin, overflow, bhi, second, best, best_prim, best_rank, wobj, wprim, nnode);
          if (S.w_inert && !ray_sane(ray)) st = 2;
          const bool exact = st == 2;
          if constexpr ((F & F_STATS) != 0) nfall += exact ? 1u : 0u;
          hit = st == 1;
          // exact: every entry in list order (the reference's visit sets); else the media after the tree
          for (int w = exact ? 0 : S.w_media; w < S.n_world; ++w) {
            const int oi = ro<F>(S.world)[w];
            const rt_object o = ro<F>(S.objects)[oi];
            float tq;
            int pq;
            bool hq;
            const float tcl = hit ? best : tmax;
            if (o.kind == RT_OBJ_MEDIUM) {
              hq = object_query<FM>(S, oi, ray, tmin, tcl, tq, pq, loc, nnode, nprim, nfall);
            } else {
              Ray rr = ray;
              int xi = oi;
              if constexpr ((F & F_XFORM) != 0) if (o.kind == RT_OBJ_XFORM) {
                Ray moved;
                rr = xform_ray(o, ray, moved);
                xi = o.a;
              }
              const rt_object x = ro<F>(S.objects)[xi];
              if ((F & F_BVH) != 0 && x.kind == RT_OBJ_BVH) {
                hq = bvh_exact<F>(S, x.a, x.b, rr, mk(1.0f / rr.d.x, 1.0f / rr.d.y, 1.0f / rr.d.z), tmin, tcl, tq, pq,
                                  nnode, nprim, nfall);
              } else {
                pq = x.a;
                hq = prim_t<F>(S, x.a, rr, tmin, tcl, tq, nprim);
              }
            }
            if (hq) {
              hit = true;
              best = tq;
              wobj = oi;
              wprim = pq;
            }
          }
          if (hit) object_record<FM>(S, wobj, wprim, ray, tmin, best, h);
        } else {
          hit = bvh_settle<F>(S, obj.a, obj.b, ray, tmin, tmax, overflow, bhi, second, best, best_prim, best_rank,
                              nnode, nprim, nfall);
          // primitive objects after the BVH in the world list (C4's ground sphere): hittable_list's
          // rule, t_max = the closest hit so far (inclusive), so a later entry wins a tie
          for (int w = 1; w < S.n_world; ++w) {
            const rt_object po = ro<0>(S.objects)[ro<0>(S.world)[w]];  // uniform: scalar loads
            float tq;
            if (prim_t_q<F>(S, load_prim_u<F>(S, po.a), ray, tmin, hit ? best : tmax, tq, nprim)) {
              hit = true;
              best = tq;
              best_prim = po.a;
            }
          }
          if (hit) finalize<F>(S, best_prim, ray, tmin, best, h);
        }
        RT_STEP_PASS_LANES(pass, 2, hit);
        RT_STEP_PASS_LANES(pass, 3, !hit);
        if (!hit) {
          contrib = vget(att_r, 15) * ld3(P.S.bg);
          ended = true;
        } else {
          V a, em;
          RT_STAMP(6);
          bool sc;
          if constexpr (PKS) {  // on a register copy of the parked state
            Rng lr = loc;
            sc = scatter<F>(S, ray, h, a, em, lr);
            loc = lr;
          } else {
            sc = scatter<F>(S, ray, h, a, em, loc);
          }
          RT_STEP_PASS_LANES(pass, 4, !sc);
          if (sc) {
            vset(att_r, 15, vget(att_r, 15) * a);
            if (++depth == P.max_depth) {
              RT_STEP_PASS_LANES(pass, 5, true);
              contrib = mk(0.0f, 0.0f, 0.0f);
              ended = true;
            }
          } else {
            contrib = vget(att_r, 15) * em;
            ended = true;
          }
        }
        RT_STAMP(0);
        if (ended) {
          constexpr bool END_READS_TAB = !MF;  // (MF: this pass's camera setup is behind us)
#include "rt_step_body_end.h"
        }
        mode = 0;
        if constexpr (MF) {
          // a scattered ray's search starts now: no trip through Q, which in this order sees sample starts only
          if (!ended) {
            RT_STAMP(1);
#include "rt_step_body_query.h"
          }
        }
