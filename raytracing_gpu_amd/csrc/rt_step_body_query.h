// rt_step_body_query.h -- internal: a fragment of rt_step_body.h, shared as text for the reason given there.
// The start of a search for the lane's ray, written in place in `ray` just before: a camera ray (Q) or, in
// the miss-first order, a scattered ray (C).  Leaves mode = 1; Q then asks the tile's list where there is one.
#ifndef RT_STEP_BODY_PLAIN
#error "rt_step_body_query.h is a fragment of rt_step_body.h"
#endif
        // traversal reciprocals: hardware v_rcp_f32 (1 ulp; the tree's boxes are padded by 2^-16
        // relative, far above either reciprocal's rounding) instead of three IEEE divides
        const V inv = mk(__builtin_amdgcn_rcpf(ray.d.x), __builtin_amdgcn_rcpf(ray.d.y), __builtin_amdgcn_rcpf(ray.d.z));
        finv = mk(__builtin_fminf(__builtin_fmaxf(inv.x, -1e30f), 1e30f),
                  __builtin_fminf(__builtin_fmaxf(inv.y, -1e30f), 1e30f),
                  __builtin_fminf(__builtin_fmaxf(inv.z, -1e30f), 1e30f));
        oi = mk(ray.o.x * finv.x, ray.o.y * finv.y, ray.o.z * finv.z);
        qa = len2(ray.d);
        rcpa = __builtin_amdgcn_rcpf(qa);
        best = __builtin_inff();
        bhi = __builtin_inff();
        second = __builtin_inff();
        best_prim = -1;
        best_rank = 0x7fffffff;
        cur = 0;
        sp = 0;
        overflow = false;
        mode = 1;
