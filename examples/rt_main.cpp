// rt_main.cpp — the reference's main.cu (main.cu:8-45) rewritten against the C ABI: a C++ host
// program that owns the scene and calls draw() through include/rt_hip.h (one GPU) or
// include/rt_multi.h (the frame buffer tiled over several GPUs, one RCCL gather).
//
//   rt_main SCENE WIDTH SPP_PER_FB NO_FB OUT.ppm [options]
//     --devices 0,1,...     tile over these devices with rt_multi (default: one GPU, rt_draw)
//     --gather rccl|host    rt_multi's gather (default rccl; host lets ranks share a device)
//     --band-rows B         rows per band for rt_multi (default 4)
//     --repeat K            draw K times (the first draw is cold, later ones reuse the schedule)
//     --depth D             max_depth (default 50)
//     --height H            image height (default: WIDTH / the scene's aspect ratio, render.h:30)
//     --obj PATH            mesh scenes: rt_obj_load (assimp's OBJ import, reference indexing)
//     --tex PATH            texture for the mesh / earth scenes: rt_image_load (stb_image bytes)
//     --progressive K       one GPU: draw through an rt_accum, K frame buffers per step; OUT.ppm is
//                           rewritten after every step (the reference's tmp/<id>.ppm, render.h:152-162)
//                           and each step prints one JSON line with "fbs_done"
//     --checkpoint FILE     one GPU: save the accumulator to FILE after every step (one step of NO_FB
//                           frame buffers without --progressive) and, when FILE exists, continue
//                           from it up to NO_FB (prints a JSON line with "resumed_from")
//     --until-noise T       with --progressive: attach a noise monitor (rt_noise) and stop once at most
//     --noisy-fraction F    floor(F x pixels) pixels (default F = 0.01) have a noise estimate above T
//                           8-bit levels, measured after every step from 2 frame buffers on; NO_FB stays
//                           the upper limit.  Each step's JSON line gains "noise_max" and "pixels_above",
//                           a last line carries "stopped_at".  With --checkpoint FILE the monitor is
//                           saved to FILE.noise before FILE, and resuming needs it
//     --adaptive K          one GPU: draw through an rt_adapt, K frame buffers per step, rendering only the
//     --until-noise T       16 x 16 tiles still active; from max(2, F) frame buffers on (--min-fbs F,
//     --max-above M         default 4) every step retires the tiles with at most M (default 0) pixels of
//     --min-fbs F           noise above T.  Each step prints one JSON line with "fbs", "tiles_active",
//                           "pixel_fbs" and "noise_max"; a last line carries "stopped_at" and "pixel_fbs".
//                           Ends when no tile is active or at NO_FB.  Not with --progressive / --checkpoint
//     --adaptive-checkpoint FILE   with --adaptive: save the rt_adapt to FILE after every step and, when FILE
//                           exists, continue from it (prints a JSON line with "resumed_from")
//     --dilate R            with --adaptive: a tile that passes stays active while an active tile within R
//                           tiles of it (Chebyshev) fails (default 0)
//     --reopen              with --adaptive: on resuming, make the tiles that fail T / M, and those within R
//                           of one, active again, each from its own count (prints a line with "reopened")
//     --denoise OUT2.ppm    with --progressive or --adaptive: also write the denoised image of the final state
//                           (rt_denoise_monitor / rt_denoise_adaptive with the shipped parameters) to OUT2.ppm
//                           and print a JSON line with "denoised" and "denoise_ms"; needs two frame buffers.
//                           With --progressive a noise monitor is attached for it (and saved and needed on
//                           resuming, as with --until-noise) without stopping the draw
//     --guided              with --denoise: the feature-guided filter (rt_guide_denoise_monitor / _adaptive with
//                           the shipped gains) over the planes of an rt_guide of the scene
//     --aov PREFIX          write PREFIX_normal.ppm and PREFIX_albedo.ppm: the noise-free normal and albedo
//                           images of the camera's centre rays (rt_guide_render, rt_guide_image)
//     --guide-samples S     with --guided or --aov: the planes are averages of S rays per pixel spread over the
//                           pixel, the lens and the shutter (rt_aov_render with the other defaults); --aov then
//                           also writes PREFIX_coverage.ppm, the share of a pixel's rays that hit, in grey
//     --guide-specular N    with --guided or --aov: the planes follow mirrors and glass through at most N
//                           continuation rays (rt_spec_render with the other defaults; 0..16), from the centre
//                           ray or, with --guide-samples, from each of the S rays
//
// Writes OUT.ppm (binary P6, top row first) and one JSON line per draw on stdout.  Files written
// more than once go to a temporary name first and are renamed into place.
#include <chrono>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_hip.h"
#include "rt_multi.h"

namespace {

// render.h:21-50 (the reference's render_settings, unchanged in meaning)
struct render_settings {
  float aspect_ratio = 16.0f / 9.0f;
  int image_width = 1200;
  int image_height = 0;
  int samples_per_pixel_per_fb = 100;
  int no_fb = 10;
  int max_depth = 50;
  int rays_per_pixel = 0;
  void calc_all() {
    image_height = static_cast<int>(image_width / (double)aspect_ratio);  // H18
    rays_per_pixel = samples_per_pixel_per_fb * no_fb;
  }
};

rt_guide* g_guide = nullptr;  // --guided: the planes --denoise filters with

int die(const char* what, const char* msg) {
  fprintf(stderr, "rt_main: %s: %s\n", what, msg ? msg : "");
  return 99;  // checkCudaErrors' exit code (common.h:30-38)
}

std::vector<int> parse_devices(const char* s) {
  std::vector<int> d;
  while (*s) {
    d.push_back(atoi(s));
    const char* c = strchr(s, ',');
    if (!c) break;
    s = c + 1;
  }
  return d;
}

// Whole file to path: written under a temporary name, then renamed, so that a reader (or a run that
// dies) never sees half a file.
bool write_file(const std::string& path, const std::string& head, const void* data, size_t n) {
  const std::string tmp = path + ".tmp";
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) return false;
  bool ok = fwrite(head.data(), 1, head.size(), f) == head.size() && fwrite(data, 1, n, f) == n;
  ok = fclose(f) == 0 && ok;
  return ok && rename(tmp.c_str(), path.c_str()) == 0;
}

bool read_file(const char* path, std::vector<unsigned char>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  unsigned char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

// draw() through an accumulator: `step` frame buffers at a time, OUT.ppm and the checkpoint
// rewritten after each step.
int draw_progressive(rt_ctx* ctx, const char* name, const rt_render_args& a, int step, const char* ckpt,
                     const char* out, std::vector<uint8_t>& png, bool until_noise, float noise_t, double noisy_fraction,
                     const char* denoised) {
  rt_accum* acc = nullptr;
  rt_noise* mon = nullptr;
  const bool want_mon = until_noise || denoised;
  const std::string side = std::string(ckpt ? ckpt : "") + ".noise";
  std::vector<unsigned char> blob;
  if (ckpt && read_file(ckpt, blob)) {
    if (rt_accum_load(ctx, blob.data(), blob.size(), step, &acc)) return die("rt_accum_load", rt_last_error(ctx));
    rt_accum_info i = {};
    rt_accum_get_info(acc, &i);
    const rt_render_args& b = i.args;
    if (b.width != a.width || b.height != a.height || b.spp != a.spp || b.fb_first != a.fb_first ||
        b.max_depth != a.max_depth || b.cam_mode != a.cam_mode || b.band_rows != a.band_rows ||
        b.band_first != a.band_first || b.band_stride != a.band_stride || b.seed != a.seed || b.fb_count > a.fb_count)
      return die("checkpoint", "belongs to a draw with other settings");
    if (want_mon) {  // the statistics cover every frame buffer or the draw does not continue
      std::vector<unsigned char> nb;
      if (!read_file(side.c_str(), nb)) return die("--until-noise / --denoise: the checkpoint has no side file", side.c_str());
      if (rt_noise_load(acc, nb.data(), nb.size(), &mon)) return die("rt_noise_load", rt_last_error(ctx));
    }
    printf("{\"resumed_from\": %d, \"checkpoint\": \"%s\"}\n", b.fb_count, ckpt);
    fflush(stdout);
  } else if (rt_accum_create(ctx, &a, step, &acc)) {
    return die("rt_accum_create", rt_last_error(ctx));
  } else if (want_mon && rt_noise_create(acc, &mon)) {
    return die("rt_noise_create", rt_last_error(ctx));
  }
  char head[64];
  snprintf(head, sizeof(head), "P6\n%d %d\n255\n", a.width, a.height);
  rt_accum_info i = {};
  rt_accum_get_info(acc, &i);
  const long long pixels = (long long)a.width * a.height;
  auto converged = [&](const rt_noise_report& r) { return r.pixels_above <= (long long)std::floor(noisy_fraction * (double)pixels); };
  bool stop = false;
  if (until_noise && i.args.fb_count >= 2) {  // resumed: a draw that had converged stays stopped
    rt_noise_report r = {};
    if (rt_noise_measure(mon, noise_t, &r, nullptr, nullptr)) return die("rt_noise_measure", rt_last_error(ctx));
    stop = converged(r);
  }
  for (bool first = true; first || (i.args.fb_count < a.fb_count && !stop); first = false) {
    const auto t0 = std::chrono::steady_clock::now();
    rt_counters c = {};
    const int n = stop ? 0 : std::min(step, a.fb_count - i.args.fb_count);
    if (n > 0 && rt_accum_add(acc, n, &c)) return die("rt_accum_add", rt_last_error(ctx));
    if (rt_accum_image(acc, png.data(), 1)) return die("rt_accum_image", rt_last_error(ctx));
    rt_accum_get_info(acc, &i);
    if (!write_file(out, head, png.data(), png.size())) return die("write", out);
    if (ckpt && n > 0 && mon) {  // before the checkpoint: a checkpoint never lacks its side file
      size_t need = 0;
      rt_noise_save(mon, nullptr, 0, &need);
      blob.resize(need);
      if (rt_noise_save(mon, blob.data(), blob.size(), nullptr)) return die("rt_noise_save", rt_last_error(ctx));
      if (!write_file(side, "", blob.data(), blob.size())) return die("write", side.c_str());
    }
    if (ckpt && n > 0) {
      size_t need = 0;
      rt_accum_save(acc, nullptr, 0, &need);
      blob.resize(need);
      if (rt_accum_save(acc, blob.data(), blob.size(), nullptr)) return die("rt_accum_save", rt_last_error(ctx));
      if (!write_file(ckpt, "", blob.data(), blob.size())) return die("write", ckpt);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    rt_noise_report rep = {};
    const bool measured = until_noise && i.args.fb_count >= 2;
    if (measured) {
      if (rt_noise_measure(mon, noise_t, &rep, nullptr, nullptr)) return die("rt_noise_measure", rt_last_error(ctx));
      stop = converged(rep);
    }
    printf("{\"fbs_done\": %d, \"scene\": \"%s\", \"width\": %d, \"height\": %d, \"wall_ms\": %.3f, "
           "\"segments\": %llu, \"samples\": %llu",
           i.args.fb_count, name, a.width, a.height, ms, (unsigned long long)c.segments, (unsigned long long)c.samples);
    if (measured) printf(", \"noise_max\": %.9g, \"pixels_above\": %lld", rep.max_noise, (long long)rep.pixels_above);
    printf("}\n");
    fflush(stdout);
  }
  if (until_noise) {
    printf("{\"stopped_at\": %d, \"converged\": %s, \"until_noise\": %.9g, \"noisy_fraction\": %.9g}\n", i.args.fb_count,
           stop ? "true" : "false", noise_t, noisy_fraction);
    fflush(stdout);
  }
  if (denoised) {
    if (g_guide ? rt_guide_denoise_monitor(mon, g_guide, nullptr, nullptr, png.data(), nullptr, 1)
                : rt_denoise_monitor(mon, nullptr, png.data(), nullptr, 1))
      return die(g_guide ? "rt_guide_denoise_monitor" : "rt_denoise_monitor", rt_last_error(ctx));
    if (!write_file(denoised, head, png.data(), png.size())) return die("write", denoised);
    printf("{\"denoised\": \"%s\", \"fbs\": %d, \"denoise_ms\": %.3f}\n", denoised, i.args.fb_count, rt_denoise_monitor_last_ms(mon));
    fflush(stdout);
  }
  if (mon) rt_noise_destroy(mon);
  rt_accum_destroy(acc);
  return 0;
}

// draw() through an adaptive accumulator: `step` frame buffers at a time for the tiles still active, none
// beyond NO_FB; with a checkpoint the state is saved after every step and an existing one is continued.
int draw_adaptive(rt_ctx* ctx, const char* name, const rt_render_args& a, int step, const char* out,
                  std::vector<uint8_t>& png, float noise_t, int max_above, int min_fbs, const char* ckpt, int dilate,
                  bool reopen, const char* denoised) {
  rt_adapt* ad = nullptr;
  rt_adapt_report rep = {};
  int done = 0;
  bool measured = false;  // rep describes the current state
  std::vector<unsigned char> blob;
  if (ckpt && read_file(ckpt, blob)) {
    rt_accum_info i = {};
    if (rt_adaptive_load(ctx, blob.data(), blob.size(), step, &ad)) return die("rt_adaptive_load", rt_last_error(ctx));
    rt_adaptive_blob_info(blob.data(), blob.size(), &i);
    const rt_render_args& b = i.args;
    if (b.width != a.width || b.height != a.height || b.spp != a.spp || b.fb_first != a.fb_first ||
        b.max_depth != a.max_depth || b.cam_mode != a.cam_mode || b.band_rows != a.band_rows ||
        b.band_first != a.band_first || b.band_stride != a.band_stride || b.seed != a.seed || b.fb_count > a.fb_count)
      return die("checkpoint", "belongs to a draw with other settings");
    done = b.fb_count;
    printf("{\"resumed_from\": %d, \"checkpoint\": \"%s\"}\n", done, ckpt);
    if (reopen && done >= 2) {
      int before = 0;
      if (rt_adapt_get_report(ad, noise_t, &rep)) return die("rt_adapt_get_report", rt_last_error(ctx));
      before = rep.tiles_active;
      if (rt_adaptive_reopen(ad, noise_t, max_above, dilate, &rep)) return die("rt_adaptive_reopen", rt_last_error(ctx));
      measured = true;
      printf("{\"reopened\": %d, \"tiles_active\": %d, \"until_noise\": %.9g}\n", rep.tiles_active - before, rep.tiles_active,
             noise_t);
    }
    fflush(stdout);
  } else if (rt_adapt_create(ctx, &a, step, &ad)) {
    return die("rt_adapt_create", rt_last_error(ctx));
  }
  char head[64];
  snprintf(head, sizeof(head), "P6\n%d %d\n255\n", a.width, a.height);
  const size_t tiles = (size_t)((a.width + 15) / 16) * (size_t)((a.height + 15) / 16);
  std::vector<int32_t> counts(tiles);
  std::vector<uint8_t> flags(tiles);
  // a step can still render: some active tile is below NO_FB; done = the largest count
  auto more = [&]() {
    rt_adapt_counts(ad, counts.data());
    rt_adaptive_active(ad, flags.data());
    bool any = false;
    for (size_t t = 0; t < tiles; ++t) {
      done = std::max(done, (int)counts[t]);
      any = any || (flags[t] && counts[t] < a.fb_count);
    }
    return any;
  };
  bool stepped = false;
  while (more()) {
    const auto t0 = std::chrono::steady_clock::now();
    rt_counters c = {};
    if (rt_adaptive_add(ad, step, a.fb_count, &c)) return die("rt_adaptive_add", rt_last_error(ctx));
    stepped = true;
    (void)more();
    const bool retire = done >= std::max(2, min_fbs);
    if (retire && rt_adaptive_retire(ad, noise_t, max_above, dilate, &rep)) return die("rt_adaptive_retire", rt_last_error(ctx));
    measured = retire;
    if (rt_adapt_image(ad, png.data(), 1)) return die("rt_adapt_image", rt_last_error(ctx));
    if (!write_file(out, head, png.data(), png.size())) return die("write", out);
    if (ckpt) {
      size_t need = 0;
      rt_adaptive_save(ad, nullptr, 0, &need);
      blob.resize(need);
      if (rt_adaptive_save(ad, blob.data(), blob.size(), nullptr)) return die("rt_adaptive_save", rt_last_error(ctx));
      if (!write_file(ckpt, "", blob.data(), blob.size())) return die("write", ckpt);
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"fbs\": %d, \"scene\": \"%s\", \"width\": %d, \"height\": %d, \"wall_ms\": %.3f, \"segments\": %llu, "
           "\"samples\": %llu",
           done, name, a.width, a.height, ms, (unsigned long long)c.segments, (unsigned long long)c.samples);
    if (retire)
      printf(", \"tiles_active\": %d, \"pixel_fbs\": %lld, \"noise_max\": %.9g, \"pixels_above\": %lld", rep.tiles_active,
             (long long)rep.pixel_fbs, rep.max_noise, (long long)rep.pixels_above);
    printf("}\n");
    fflush(stdout);
  }
  if (!stepped && done > 0) {  // a resumed draw with nothing left to render still leaves its image
    if (rt_adapt_image(ad, png.data(), 1)) return die("rt_adapt_image", rt_last_error(ctx));
    if (!write_file(out, head, png.data(), png.size())) return die("write", out);
    if (!measured && done >= 2 && rt_adapt_get_report(ad, noise_t, &rep) == 0) measured = true;
  }
  const long long pixel_fbs = measured ? (long long)rep.pixel_fbs : (long long)a.width * a.height * done;
  printf("{\"stopped_at\": %d, \"pixel_fbs\": %lld, \"tiles_active\": %d, \"until_noise\": %.9g, \"max_above\": %d}\n", done,
         pixel_fbs, measured ? rep.tiles_active : -1, noise_t, max_above);
  fflush(stdout);
  if (denoised) {
    if (g_guide ? rt_guide_denoise_adaptive(ad, g_guide, nullptr, nullptr, png.data(), nullptr, 1)
                : rt_denoise_adaptive(ad, nullptr, png.data(), nullptr, 1))
      return die(g_guide ? "rt_guide_denoise_adaptive" : "rt_denoise_adaptive", rt_last_error(ctx));
    if (!write_file(denoised, head, png.data(), png.size())) return die("write", denoised);
    printf("{\"denoised\": \"%s\", \"fbs\": %d, \"denoise_ms\": %.3f}\n", denoised, done, rt_denoise_adaptive_last_ms(ad));
    fflush(stdout);
  }
  rt_adapt_destroy(ad);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: rt_main SCENE WIDTH SPP_PER_FB NO_FB OUT.ppm [--devices 0,1] [--gather rccl|host] "
                    "[--band-rows B] [--repeat K] [--depth D] [--height H] [--obj PATH] [--tex PATH] [--progressive K] [--checkpoint FILE] "
                    "[--until-noise T [--noisy-fraction F]] [--adaptive K --until-noise T [--max-above M] [--min-fbs F] "
                    "[--adaptive-checkpoint FILE] [--dilate R] [--reopen]] [--denoise OUT2.ppm [--guided]] [--aov PREFIX] [--guide-samples S] [--guide-specular N]\n");
    return 2;
  }
  const char* name = argv[1];
  render_settings s;
  s.image_width = atoi(argv[2]);
  s.samples_per_pixel_per_fb = atoi(argv[3]);
  s.no_fb = atoi(argv[4]);
  const char* out = argv[5];
  std::vector<int> devices;
  int gather = RT_GATHER_RCCL, band_rows = 4, repeat = 1;
  const char *obj_path = nullptr, *tex_path = nullptr, *ckpt_path = nullptr, *adaptive_ckpt = nullptr, *denoised = nullptr, *aov = nullptr;
  bool guided = false, have_guide_samples = false;
  int guide_samples = 0;
  bool have_guide_specular = false;
  int guide_specular = 0;
  int dilate = 0;
  bool reopen = false, have_resume_opts = false;
  int height = 0;
  int progressive = 0, adaptive = 0, max_above = 0, min_fbs = 4;
  bool have_adaptive = false, have_adaptive_opts = false;
  bool until_noise = false, have_fraction = false;
  float noise_t = 0.0f;
  double noisy_fraction = 0.01;
  for (int k = 6; k < argc; ++k) {
    const std::string a = argv[k];
    const char* v = k + 1 < argc ? argv[k + 1] : "";
    if (a == "--devices") devices = parse_devices(v), ++k;
    else if (a == "--gather") gather = strcmp(v, "host") == 0 ? RT_GATHER_HOST : RT_GATHER_RCCL, ++k;
    else if (a == "--band-rows") band_rows = atoi(v), ++k;
    else if (a == "--repeat") repeat = atoi(v), ++k;
    else if (a == "--depth") s.max_depth = atoi(v), ++k;
    else if (a == "--height") height = atoi(v), ++k;
    else if (a == "--obj") obj_path = v, ++k;
    else if (a == "--tex") tex_path = v, ++k;
    else if (a == "--progressive") progressive = atoi(v), ++k;
    else if (a == "--checkpoint") ckpt_path = v, ++k;
    else if (a == "--adaptive") have_adaptive = true, adaptive = atoi(v), ++k;
    else if (a == "--max-above") have_adaptive_opts = true, max_above = atoi(v), ++k;
    else if (a == "--min-fbs") have_adaptive_opts = true, min_fbs = atoi(v), ++k;
    else if (a == "--adaptive-checkpoint") have_resume_opts = true, adaptive_ckpt = v, ++k;
    else if (a == "--dilate") have_resume_opts = true, dilate = atoi(v), ++k;
    else if (a == "--reopen") have_resume_opts = true, reopen = true;
    else if (a == "--until-noise") until_noise = true, noise_t = (float)atof(v), ++k;
    else if (a == "--denoise") denoised = v, ++k;
    else if (a == "--guided") guided = true;
    else if (a == "--aov") aov = v, ++k;
    else if (a == "--guide-samples") have_guide_samples = true, guide_samples = atoi(v), ++k;
    else if (a == "--guide-specular") have_guide_specular = true, guide_specular = atoi(v), ++k;
    else if (a == "--noisy-fraction") have_fraction = true, noisy_fraction = atof(v), ++k;
    else return die("unknown option", argv[k]);
  }

  if (have_adaptive) {
    if (progressive != 0 || ckpt_path) return die("--adaptive", "cannot be combined with --progressive or --checkpoint");
    if (have_fraction) return die("--adaptive", "retires tiles by --max-above, not --noisy-fraction");
    if (!until_noise) return die("--adaptive", "needs --until-noise T");
    if (adaptive < 1 || s.no_fb < 1) return die("--adaptive", "K and NO_FB must be at least 1");
    if (max_above < 0) return die("--max-above", "must be at least 0");
    if (dilate < 0) return die("--dilate", "must be at least 0");
  } else if (have_resume_opts) {
    return die("--adaptive-checkpoint / --dilate / --reopen", "need --adaptive K");
  } else if (have_adaptive_opts) {
    return die("--max-above / --min-fbs", "need --adaptive K");
  }
  if (!have_adaptive && (until_noise || have_fraction) && progressive <= 0) return die("--until-noise / --noisy-fraction", "need --progressive K");
  if (have_fraction && !until_noise) return die("--noisy-fraction", "needs --until-noise T");
  if (denoised && !have_adaptive && progressive <= 0) return die("--denoise", "needs --progressive K or --adaptive K");
  if (guided && !denoised) return die("--guided", "needs --denoise OUT2.ppm");
  if (have_guide_samples && !guided && !aov) return die("--guide-samples", "needs --guided or --aov PREFIX");
  if (have_guide_samples && (guide_samples < 1 || guide_samples > 256)) return die("--guide-samples", "S must be 1..256");
  if (have_guide_specular && !guided && !aov) return die("--guide-specular", "needs --guided or --aov PREFIX");
  if (have_guide_specular && (guide_specular < 0 || guide_specular > 16)) return die("--guide-specular", "N must be 0..16");
  if ((guided || aov) && !devices.empty()) return die("--guided / --aov", "one GPU only (no --devices)");
  if (denoised && s.no_fb > 32768) return die("--denoise", "a noise monitor accepts at most 32768 frame buffers");
  if (until_noise && s.no_fb > 32768) return die("--until-noise", "a noise monitor accepts at most 32768 frame buffers");

  // ---- scene: the reference's `door_scene curr_scene;` etc. (main.cu:17-18) as the host library
  rt_scene_host* scene = nullptr;
  rt_obj_mesh* obj = nullptr;
  rt_image_host* tex = nullptr;
  if (obj_path || tex_path) {
    rt_image_asset img = {};
    rt_mesh_asset mesh = {};
    rt_scene_assets assets = {};
    if (tex_path) {  // make_image(): stbi_load(path, .., 0) bytes
      if (rt_image_load(tex_path, &tex)) return die("rt_image_load", tex_path);
      img = *rt_image_view(tex);
      assets.n_images = 1;
      assets.images = &img;
    }
    if (obj_path) {  // create_meshes(): assimp Triangulate | GenNormals, create_meshes_d indexing (H16)
      if (rt_obj_load(obj_path, RT_OBJ_INDEX_REFERENCE, &obj)) return die("rt_obj_load", obj_path);
      const rt_obj_info* oi = rt_obj_view(obj);
      mesh = rt_mesh_asset{oi->n_triangles, 1, 0, 0, oi->triangles};
      assets.n_meshes = 1;
      assets.meshes = &mesh;
    }
    if (rt_scene_build_ex(name, &assets, &scene)) return die("rt_scene_build_ex", name);
    if (obj) rt_obj_free(obj);  // the scene owns copies
    if (tex) rt_image_free(tex);
  } else if (rt_scene_build(name, &scene)) {
    return die("rt_scene_build", name);
  }
  const rt_scene_soa* soa = rt_scene_view(scene);
  s.aspect_ratio = soa->aspect;  // main.cu:27
  s.calc_all();
  if (height > 0) s.image_height = height;

  rt_render_args a = {};
  a.width = s.image_width;
  a.height = s.image_height;
  a.spp = s.samples_per_pixel_per_fb;
  a.fb_first = 0;
  a.fb_count = s.no_fb;
  a.max_depth = s.max_depth;
  a.cam_mode = RT_CAM_REF_SLOT0;
  a.band_rows = devices.empty() ? a.height : band_rows;
  a.band_first = 0;
  a.band_stride = 1;
  a.seed = 1984;  // render.h:91
  std::vector<uint8_t> png(3 * (size_t)a.width * a.height);
  rt_counters c = {};

  rt_ctx* ctx = nullptr;
  rt_multi* multi = nullptr;
  if (devices.empty()) {
    if (rt_ctx_create(0, &ctx)) return die("rt_ctx_create", "device 0");
    if (rt_scene_upload(ctx, soa)) return die("rt_scene_upload", rt_last_error(ctx));
  } else {
    int rc = rt_multi_create((int)devices.size(), devices.data(), gather, &multi);
    if (rc) return die("rt_multi_create", gather == RT_GATHER_RCCL ? "RCCL communicator (distinct devices?)" : "");
    if (rt_multi_upload(multi, soa)) return die("rt_multi_upload", rt_multi_last_error(multi));
  }
  rt_guide* guide = nullptr;
  if (guided || aov) {  // the feature planes of the camera's centre rays, from the guide's own copy of the scene
    if (rt_guide_create(soa, 0, &guide)) return die("rt_guide_create", name);
    rt_aov_params ap;
    rt_aov_params_default(&ap);
    ap.samples = guide_samples;
    if (have_guide_specular) {  // ... of what mirrors and glass show, from the centre ray or from S rays
      rt_spec_params sp;
      rt_spec_params_default(&sp);
      sp.max_bounces = guide_specular;
      if (rt_spec_render(guide, a.width, a.height, have_guide_samples ? &ap : nullptr, &sp)) return die("rt_spec_render", name);
    } else if (have_guide_samples) {  // ... or of S rays per pixel, averaged
      if (rt_aov_render(guide, a.width, a.height, &ap)) return die("rt_aov_render", name);
    } else if (rt_guide_render(guide, a.width, a.height)) {
      return die("rt_guide_render", name);
    }
    if (guided) g_guide = guide;
    char head[64];
    snprintf(head, sizeof(head), "P6\n%d %d\n255\n", a.width, a.height);
    for (int which = 0; aov && which < 2; ++which) {
      const std::string path = std::string(aov) + (which == RT_GUIDE_NORMAL ? "_normal.ppm" : "_albedo.ppm");
      if (rt_guide_image(guide, which, png.data(), 1)) return die("rt_guide_image", path.c_str());
      if (!write_file(path, head, png.data(), png.size())) return die("write", path.c_str());
    }
    if (aov && have_guide_samples) {  // quant(coverage) as write_frame_buffer quantises (color.h:40-44), in grey
      const std::string path = std::string(aov) + "_coverage.ppm";
      std::vector<float> cov((size_t)a.width * a.height);
      if (rt_aov_coverage(guide, cov.data(), 1)) return die("rt_aov_coverage", path.c_str());
      for (size_t p = 0; p < cov.size(); ++p) {
        const float r = std::sqrt(cov[p]);
        png[3 * p] = png[3 * p + 1] = png[3 * p + 2] = (uint8_t)(int)(256.0f * (r > 0.999f ? 0.999f : r));
      }
      if (!write_file(path, head, png.data(), png.size())) return die("write", path.c_str());
      if (have_guide_specular)
        printf("{\"aov\": \"%s\", \"guide_ms\": %.3f, \"guide_samples\": %d, \"guide_specular\": %d}\n", aov, rt_spec_last_ms(guide),
               guide_samples, guide_specular);
      else
        printf("{\"aov\": \"%s\", \"guide_ms\": %.3f, \"guide_samples\": %d}\n", aov, rt_aov_last_ms(guide), guide_samples);
    } else if (aov && have_guide_specular) {
      printf("{\"aov\": \"%s\", \"guide_ms\": %.3f, \"guide_specular\": %d}\n", aov, rt_spec_last_ms(guide), guide_specular);
    } else if (aov) {
      printf("{\"aov\": \"%s\", \"guide_ms\": %.3f}\n", aov, rt_guide_last_ms(guide));
    }
  }
  if (have_adaptive) {
    if (!ctx) return die("--adaptive", "one GPU only (no --devices)");
    const int rc = draw_adaptive(ctx, name, a, adaptive, out, png, noise_t, max_above, min_fbs, adaptive_ckpt, dilate, reopen, denoised);
    if (guide) rt_guide_destroy(guide);
    rt_ctx_destroy(ctx);
    rt_scene_free(scene);
    return rc;
  }
  if (progressive != 0 || ckpt_path) {
    if (!ctx) return die("--progressive / --checkpoint", "one GPU only (no --devices)");
    if (progressive < 0 || a.fb_count < 1) return die("--progressive", "K and NO_FB must be at least 1");
    const int rc = draw_progressive(ctx, name, a, progressive > 0 ? progressive : a.fb_count, ckpt_path, out, png,
                                      until_noise, noise_t, noisy_fraction, denoised);
    if (guide) rt_guide_destroy(guide);
    rt_ctx_destroy(ctx);
    rt_scene_free(scene);
    return rc;
  }
  for (int k = 0; k < repeat; ++k) {
    const auto t0 = std::chrono::steady_clock::now();
    rt_multi_timing tm = {};
    if (ctx) {
      if (rt_draw(ctx, &a, png.data(), &c)) return die("rt_draw", rt_last_error(ctx));
    } else if (rt_multi_draw(multi, &a, png.data(), &c, &tm)) {
      return die("rt_multi_draw", rt_multi_last_error(multi));
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"draw\": %d, \"scene\": \"%s\", \"width\": %d, \"height\": %d, \"ranks\": %d, \"wall_ms\": %.3f, "
           "\"segments\": %llu, \"samples\": %llu",
           k, name, a.width, a.height, ctx ? 1 : (int)devices.size(), ms, (unsigned long long)c.segments,
           (unsigned long long)c.samples);
    if (multi) {
      printf(", \"warm\": %d, \"render_ms_max\": %.3f, \"gather_ms\": %.3f, \"gather_bytes\": %.0f, \"kernel_ms\": [",
             tm.warm, tm.render_ms_max, tm.gather_ms, tm.gather_bytes);
      for (size_t r = 0; r < devices.size(); ++r) printf("%s%.3f", r ? ", " : "", tm.kernel_ms[r]);
      printf("]");
    }
    printf("}\n");
    fflush(stdout);
  }
  // average_images wrote the PNG with png++ (color.h:125-170); a binary PPM carries the same bytes
  FILE* f = fopen(out, "wb");
  if (!f) return die("open", out);
  fprintf(f, "P6\n%d %d\n255\n", a.width, a.height);
  fwrite(png.data(), 1, png.size(), f);
  fclose(f);
  if (guide) rt_guide_destroy(guide);
  if (ctx) rt_ctx_destroy(ctx);
  if (multi) rt_multi_destroy(multi);
  rt_scene_free(scene);
  return 0;
}
