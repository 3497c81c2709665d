// rt_step_body_end.h -- internal: a fragment of rt_step_body.h, shared as text for the reason given there.
// The end of a path (render.h:69-77 and the sample loop around it): the colour sum, the sample count, the
// next sample's table entry and, at the item's end, its stores, `ckpt` tail included, and item = -1.
// The parent's pass order runs this text once per pass (inside the heavy block); the miss-first order runs
// it in block A and, for the rare endings there, in block C.
// In scope besides the kernel's state: `contrib` (the path's radiance) and the constant END_READS_TAB
// (whether the camera setup that consumes cam_e still follows in this pass: A yes, C of the miss-first order
// no -- there the entry is read at the setup of a later pass, cam_have).
#ifndef RT_STEP_BODY_PLAIN
#error "rt_step_body_end.h is a fragment of rt_step_body.h"
#endif
          const V col = vget(col_r, 12) + contrib;
          vset(col_r, 12, col);
          depth = 0;
          ++nsamp;
          // the item ends after sample spp - 1, a split item's sample (split_mode 2) after itself
          // (parking variants derive it from ck: sample ck % spp)
          if constexpr (PKS) s_end_r = (P.split_mode == 2 && ck >= 0) ? ck - (ck / P.spp) * P.spp + 1 : P.spp;
          const bool item_ends = ++s == (PLAIN ? P.spp : s_end_r);
          if (TAB && !per_pixel && !item_ends && END_READS_TAB) {  // the next sample's, below spp
            cam_e = P.S.cam_tab[s];
            cam_have = true;
          }
          if (item_ends) {
            if (SPLIT && P.split_mode == 2 && ck >= 0) {  // one sample of a split item: its sum, merged later
              float* dst = P.contrib + 3 * (long long)ck;
              dst[0] = col.x;
              dst[1] = col.y;
              dst[2] = col.z;
            } else {
              const V out = (1.0f / (float)P.spp) * col;
              float* dst = P.fb + 3 * (((long long)f * P.rows + r) * P.W + i);
              dst[0] = out.x;
              dst[1] = out.y;
              dst[2] = out.z;
            }
            if (P.row_cost && (i & 15) == 0) atomicAdd(&P.row_cost[j], (unsigned long long)item_segs);
            if (P.item_cost) P.item_cost[item] = (uint16_t)(item_segs < 65535u ? item_segs : 65535u);
            if (SPLIT && P.split_mode == 1 && ck >= 0) P.ckpt[2 * (long long)ck * P.spp + 1] = make_uint4(0u, 0u, item_segs, 0u);
            item = -1;
          }
