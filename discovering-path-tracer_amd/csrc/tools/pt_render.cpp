// pt_render — headless C++ driver: the role VulkanRayTracer::initComputePipeline
// + mainLoop (src/Vulkan/VulkanRayTracer.cpp:41-865) play in the reference,
// minus the Qt window.  Loads an OBJ, builds the BVH, uploads, renders
// `spp` progressive 1-spp batches (or one fused launch) and writes a PFM.
//
//   pt_render scene.obj [-w 1920] [-h 1080] [-spp 8] [-depth 4] [-sss 3]
//             [-fused] [-o out.pfm] [-png out.png] [-device 0 | -devices 0,1,..]
//             [-cache scene.ptscene] [-progressive N [-chunk K] [-orbit-at B]]
//             [-denoise | -denoise-var] [-guide normals.pfm] [-temporal K [-temporal-spatial]]
//             [-adaptive MIN MAX STEP THRESHOLD [-lum-floor F] [-adaptive-wf]]
//             [-display clamp|reinhard|aces] [-exposure X] [-auto-exposure KEY] [-pick X Y]
//             [-upsample S] [-radiance IN OUT [-samples S] [-seed-stride K]]
//
// -radiance IN OUT reads n pt_ray records (32 B each: o, d, -, seed) from the file IN, path-traces them in the
// scene under the driver's light, -depth and -sss (pt_trace_radiance_sync; -samples S samples a query from the
// seeds seed + s * K, default 1 and 1) and writes n float4 {r, g, b, a} to OUT; nothing is rendered after it
// (-spp is taken as 0).  A single-device context.
// -pick X Y prints, before anything is rendered, the closest hit of the guide ray of pixel (X, Y)
// (pt_guide_ray, pt_trace_rays_sync): t, the triangle's index, u, v, the normal and the position o + d * t,
// floats with nine significant digits (which name their bits), or "miss".  A single-device context.
// -progressive runs the reference's interactive loop (mainLoop, :717-865)
// headless: up to N batches (cap 1024, :719) in launches of K, a readback of
// every launch overlapped with the next one (double-buffered), and, with
// -orbit-at, a camera change after B batches that restarts at batch 0.
// -cache loads/saves the built scene (pt_scene_save) next to the OBJ.
// -devices renders on several GPUs from this one thread (pt_create_multi:
// each renders its screen tiles straight into the frame on the first one);
// every other call is unchanged.
// -denoise filters the final image on the device (pt_denoise, default
// parameters) before -o / -png are written; -guide writes the first-hit
// normals of the guide image as a PFM.  -denoise-var turns PT_OPT_MOMENTS on
// before rendering and filters with the variance-guided filter
// (pt_denoise_var, default parameters; at least 2 spp).  All three need a
// single-device context.
// -temporal K runs K frames of the temporal loop (pt_temporal_advance) at -spp
// samples each instead of one render: camera k (k = 0 .. K-1) is the default
// camera rotated k times about +y by the float32 step x' = x*c + z*s,
// z' = z*c - x*s with c = 0.99939083f, s = 0.0348995f (2 degrees), applied to
// the position and the direction.  -o / -png then hold the temporal colour,
// or, with -denoise-var, pt_temporal_denoise's result at the default
// parameters.  -temporal-spatial (with -temporal K) filters the final frame with
// pt_temporal_denoise_spatial instead, both parameter sets at their defaults:
// pixels with a short history take the spatial variance estimate.
// -adaptive MIN MAX STEP THRESHOLD renders adaptively instead (pt_adaptive_begin,
// then pt_adaptive_advance four rounds at a time, looking at pt_adaptive_info
// after each four until no tile is live) and prints the samples it spent against
// MAX samples for every pixel; -lum-floor sets the rule's floor (default: the
// library's).  With -denoise-var the image written is pt_adaptive_denoise's.
// -adaptive-wf runs the rounds on the wavefront pipeline (PT_OPT_ADAPTIVE_WF 1).
// -display, -exposure and -auto-exposure send whatever image -png writes (raw,
// filtered, temporal, ...) through the display transform on the device
// (pt_display: tone map, exposure, metering with the given key; the other
// parameters at their defaults) and write its bytes with pt_write_png8; a
// filter then writes into an image of the driver's own.  Without any of the
// three -png is pt_write_image's encode of the floats, as ever.
// -upsample S (2 to 8) renders at -w / -h and writes the (S*w) x (S*h) frame: whatever image the other flags
// produced (raw, -denoise, -denoise-var, -temporal, -adaptive) goes through pt_upsample at the default sigmas
// before -o / -png are written, and with the display flags -png holds pt_upsample_display's bytes (the fused
// kernel; metering sees the rendered pixels).  A single-device context.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "pathtracer.h"

static int check(int rc, const char* what) {
  if (rc != PT_OK) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, pt_last_error());
    exit(1);
  }
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr,
            "usage: %s scene.obj [-w W] [-h H] [-spp N] [-depth D] [-sss S] [-fused] [-o out.pfm] [-png out.png]\n"
            "       [-denoise | -denoise-var] [-guide normals.pfm] [-temporal K [-temporal-spatial]] [-device D | -devices D0,D1,..] [-cache scene.ptscene]\n"
            "       [-progressive N [-chunk K] [-orbit-at B]] [-adaptive MIN MAX STEP THRESHOLD [-lum-floor F] [-adaptive-wf]]\n"
            "       [-display clamp|reinhard|aces] [-exposure X] [-auto-exposure KEY] [-pick X Y] [-upsample S]\n",
            argv[0]);
    return 2;
  }
  std::string scene_path = argv[1], out_path;
  int W = 1024, H = 1024, spp = 8, device = 0;   // VulkanRayTracer.cpp:21-22
  pt_params params{4, 3};
  bool fused = false;
  int progressive = 0, chunk = 8, orbit_at = -1, temporal = 0;
  std::string cache_path, png_path, guide_path;
  bool denoise = false, denoise_var = false, temporal_spatial = false;
  bool adaptive = false, adaptive_wf = false;
  pt_adaptive_params ad;
  pt_adaptive_default_params(&ad);
  bool display = false;
  pt_display_params dp;
  pt_display_default_params(&dp);
  bool pick = false;
  int pick_x = 0, pick_y = 0;
  int upsample = 0;   // -upsample: the scale, 0 = off
  std::string radiance_in, radiance_out;   // -radiance: the queries' file and the answers'
  pt_radiance_params rad;
  pt_radiance_default_params(&rad);
  std::vector<int> devices;   // -devices: a multi-device context
  for (int i = 2; i < argc; ++i) {
    auto next = [&](void) { return (i + 1 < argc) ? argv[++i] : (char*)"0"; };
    if (!strcmp(argv[i], "-w")) W = atoi(next());
    else if (!strcmp(argv[i], "-h")) H = atoi(next());
    else if (!strcmp(argv[i], "-spp")) spp = atoi(next());
    else if (!strcmp(argv[i], "-depth")) params.max_depth = atoi(next());
    else if (!strcmp(argv[i], "-sss")) params.sss_bounces = atoi(next());
    else if (!strcmp(argv[i], "-device")) device = atoi(next());
    else if (!strcmp(argv[i], "-devices")) {
      for (const char* p = next(); *p;) {
        devices.push_back(atoi(p));
        while (*p && *p != ',') ++p;
        if (*p == ',') ++p;
      }
    }
    else if (!strcmp(argv[i], "-fused")) fused = true;
    else if (!strcmp(argv[i], "-o")) out_path = next();
    else if (!strcmp(argv[i], "-cache")) cache_path = next();
    else if (!strcmp(argv[i], "-png")) png_path = next();
    else if (!strcmp(argv[i], "-denoise")) denoise = true;
    else if (!strcmp(argv[i], "-denoise-var")) denoise_var = true;
    else if (!strcmp(argv[i], "-guide")) guide_path = next();
    else if (!strcmp(argv[i], "-progressive")) progressive = atoi(next());
    else if (!strcmp(argv[i], "-chunk")) chunk = atoi(next());
    else if (!strcmp(argv[i], "-orbit-at")) orbit_at = atoi(next());
    else if (!strcmp(argv[i], "-temporal")) temporal = atoi(next());
    else if (!strcmp(argv[i], "-temporal-spatial")) temporal_spatial = true;
    else if (!strcmp(argv[i], "-adaptive")) {
      adaptive = true;
      ad.min_batches = (uint32_t)atoi(next());
      ad.max_batches = (uint32_t)atoi(next());
      ad.step = (uint32_t)atoi(next());
      ad.threshold = (float)atof(next());
    }
    else if (!strcmp(argv[i], "-lum-floor")) ad.lum_floor = (float)atof(next());
    else if (!strcmp(argv[i], "-adaptive-wf")) adaptive_wf = true;
    else if (!strcmp(argv[i], "-display")) {
      const char* op = next();
      display = true;
      dp.tonemap = !strcmp(op, "reinhard") ? PT_TONEMAP_REINHARD : !strcmp(op, "aces") ? PT_TONEMAP_ACES
                   : !strcmp(op, "clamp") ? PT_TONEMAP_CLAMP : -1;
    }
    else if (!strcmp(argv[i], "-exposure")) {
      display = true;
      dp.exposure = (float)atof(next());
    }
    else if (!strcmp(argv[i], "-pick")) {
      pick = true;
      pick_x = atoi(next());
      pick_y = atoi(next());
    }
    else if (!strcmp(argv[i], "-upsample")) upsample = atoi(next());
    else if (!strcmp(argv[i], "-radiance")) {
      radiance_in = next();
      radiance_out = next();
      spp = 0;
    }
    else if (!strcmp(argv[i], "-samples")) rad.n_samples = (uint32_t)atoi(next());
    else if (!strcmp(argv[i], "-seed-stride")) rad.seed_stride = (uint32_t)strtoul(next(), nullptr, 0);
    else if (!strcmp(argv[i], "-auto-exposure")) {
      display = true;
      dp.auto_exposure = 1;
      dp.key = (float)atof(next());
    }
  }
  if (temporal_spatial && temporal <= 0) {
    fprintf(stderr, "-temporal-spatial needs -temporal K\n");
    return 2;
  }
  if (adaptive && (temporal > 0 || progressive > 0 || denoise)) {
    fprintf(stderr, "-adaptive goes with neither -temporal, -progressive nor -denoise\n");
    return 2;
  }
  pt_scene* scene = nullptr;
  auto t0 = std::chrono::steady_clock::now();
  bool cached = false;
  if (!cache_path.empty() && pt_scene_load_cache(cache_path.c_str(), &scene) == PT_OK) {
    cached = true;
  } else {
    check(pt_scene_load_obj(scene_path.c_str(), &scene), "load obj");
    check(pt_scene_build_bvh(scene, 0, 0), "build bvh");
    if (!cache_path.empty()) check(pt_scene_save(scene, cache_path.c_str()), "save cache");
  }
  auto t1 = std::chrono::steady_clock::now();
  size_t nvf, ni, nn;
  pt_scene_counts(scene, &nvf, &ni, &nn, nullptr, nullptr);
  printf("scene: %zu vertices, %zu triangles, %zu nodes, %s %.3f s\n", nvf / 3, ni / 3, nn,
         cached ? "cache load" : "OBJ parse + BVH build", std::chrono::duration<double>(t1 - t0).count());

  pt_context* ctx = nullptr;
  if (devices.empty()) {
    check(pt_create(device, &ctx), "create");
  } else {
    check(pt_create_multi(devices.data(), (int)devices.size(), &ctx), "create_multi");
    int peer = 0;
    check(pt_group_info(ctx, nullptr, nullptr, 0, &peer), "group_info");
    printf("devices: %zu (%s)\n", devices.size(), peer ? "peer stores into the first device's frame" : "packed tile copies");
  }
  if (denoise_var || temporal > 0 || adaptive) check(pt_set_option(ctx, PT_OPT_MOMENTS, 1), "moments");
  if (adaptive_wf) check(pt_set_option(ctx, PT_OPT_ADAPTIVE_WF, 1), "adaptive-wf");
  check(pt_scene_upload(ctx, scene), "upload scene");
  const float pos[3] = {0.0f, 2.0f, 0.0f}, nrm[3] = {0.0f, -1.0f, 0.0f}, inten[3] = {10.0f, 10.0f, 10.0f},
              size[2] = {2.5f, 2.5f};   // VulkanRayTracer.cpp:149-162
  pt_area_light light;
  pt_pack_light(pos, nrm, inten, size, &light);
  check(pt_upload_lights(ctx, &light, 1), "upload lights");
  float ubo[16];
  pt_default_camera(ubo);
  check(pt_set_camera(ctx, ubo), "camera");
  check(pt_set_params(ctx, &params), "params");
  check(pt_resize_and_clear(ctx, W, H), "resize");
  check(pt_synchronize(ctx), "sync");
  if (pick) {
    pt_ray ray = {};
    pt_hit hit = {};
    check(pt_guide_ray(ubo, W, H, pick_x, pick_y, ray.o, ray.d), "guide ray");
    check(pt_trace_rays_sync(ctx, PT_RAYS_CLOSEST, &ray, 1, &hit), "trace rays");
    if (hit.tri < 0) {
      printf("pick (%d, %d): miss\n", pick_x, pick_y);
    } else {
      float pos[3];
      for (int k = 0; k < 3; ++k) pos[k] = ray.o[k] + ray.d[k] * hit.t;
      printf("pick (%d, %d): t %.9g tri %d u %.9g v %.9g n %.9g %.9g %.9g p %.9g %.9g %.9g\n", pick_x, pick_y,
             hit.t, hit.tri, hit.u, hit.v, hit.n[0], hit.n[1], hit.n[2], pos[0], pos[1], pos[2]);
    }
  }
  if (!radiance_in.empty()) {
    FILE* f = fopen(radiance_in.c_str(), "rb");
    if (!f) {
      fprintf(stderr, "-radiance: cannot read %s\n", radiance_in.c_str());
      return 1;
    }
    std::vector<pt_ray> queries;
    pt_ray q;
    while (fread(&q, sizeof q, 1, f) == 1) queries.push_back(q);
    fclose(f);
    std::vector<float> answers(4 * queries.size());
    check(pt_trace_radiance_sync(ctx, &rad, queries.data(), queries.size(), answers.data()), "trace radiance");
    f = fopen(radiance_out.c_str(), "wb");
    if (!f || fwrite(answers.data(), 16, queries.size(), f) != queries.size() || fclose(f) != 0) {
      fprintf(stderr, "-radiance: cannot write %s\n", radiance_out.c_str());
      return 1;
    }
    printf("radiance: %zu queries x %u samples -> %s\n", queries.size(), rad.n_samples, radiance_out.c_str());
    pt_destroy(ctx);
    pt_scene_free(scene);
    return 0;
  }
  if (progressive > 0) {
    // orbit: the default camera rotated 30 degrees about +y around the origin
    float orbit[16];
    memcpy(orbit, ubo, sizeof orbit);
    const float c30 = 0.8660254f, s30 = 0.5f;
    orbit[0] = ubo[0] * c30 + ubo[2] * s30;
    orbit[2] = -ubo[0] * s30 + ubo[2] * c30;
    orbit[4] = ubo[4] * c30 + ubo[6] * s30;
    orbit[6] = -ubo[4] * s30 + ubo[6] * c30;
    std::vector<float> frame((size_t)W * H * 4);
    int pending = 0, frames = 0, done = 0;
    auto p0 = std::chrono::steady_clock::now();
    for (;;) {
      int reset = 0;
      check(pt_progressive_camera(ctx, (orbit_at >= 0 && done >= orbit_at) ? orbit : ubo, &reset), "camera");
      uint32_t first = 0, count = 0;
      const uint32_t want = (uint32_t)std::min(chunk, progressive - done);
      check(pt_progressive_advance(ctx, want, 1024, &first, &count), "advance");
      if (count == 0) break;
      done += (int)count;
      int t = 0;
      check(pt_readback_begin(ctx, &t), "readback");
      if (pending) {   // the previous launch's image, copied while this one renders
        check(pt_readback_end(ctx, pending, frame.data(), frame.size()), "readback end");
        ++frames;
      }
      pending = t;
      if (reset) printf("camera changed: restarting at batch %u\n", first);
      if (done >= progressive) break;
    }
    if (pending) {
      check(pt_readback_end(ctx, pending, frame.data(), frame.size()), "readback end");
      ++frames;
    }
    auto p1 = std::chrono::steady_clock::now();
    printf("progressive: %d batches, %d frames read back, %.3f ms\n", done, frames,
           std::chrono::duration<double, std::milli>(p1 - p0).count());
  }
  auto r0 = std::chrono::steady_clock::now();
  if (progressive > 0) {
    // the accumulation buffer already holds the progressive result
  } else if (temporal > 0) {
    float cam[16];
    memcpy(cam, ubo, sizeof cam);
    const float c2 = 0.99939083f, s2 = 0.0348995f;
    for (int k = 0; k < temporal; ++k) {
      if (k > 0)
        for (int o = 0; o <= 4; o += 4) {   // the position, then the direction
          const float x = cam[o], z = cam[o + 2];
          cam[o] = x * c2 + z * s2;
          cam[o + 2] = z * c2 - x * s2;
        }
      check(pt_temporal_advance(ctx, cam, (uint32_t)spp), "temporal advance");
    }
  } else if (adaptive) {
    check(pt_adaptive_begin(ctx, &ad), "adaptive begin");
    uint32_t rounds = 0, live = 0;
    unsigned long long spent = 0;
    do {   // nothing is waited for inside the four rounds; the look at the counts is the only wait
      check(pt_adaptive_advance(ctx, 4), "adaptive advance");
      check(pt_adaptive_info(ctx, &rounds, &live, &spent), "adaptive info");
    } while (live > 0);
    const double full = (double)ad.max_batches * W * H;
    printf("adaptive: %u rounds, %llu samples spent of %.0f at %u spp everywhere (%.1f %%)\n", rounds, spent, full,
           ad.max_batches, 100.0 * (double)spent / full);
  } else if (fused) {
    check(pt_render(ctx, 0, (uint32_t)spp), "render");
  } else {
    for (int b = 0; b < spp; ++b) check(pt_dispatch(ctx, (uint32_t)b), "dispatch");   // mainLoop, 1 spp per batch
  }
  check(pt_synchronize(ctx), "sync");
  auto r1 = std::chrono::steady_clock::now();
  if (temporal > 0 && progressive == 0)
    printf("temporal: %d frames of %dx%d x %d spp in %.3f ms\n", temporal, W, H, spp,
           std::chrono::duration<double, std::milli>(r1 - r0).count());
  else if (adaptive)
    printf("rendered %dx%d adaptively in %.3f ms\n", W, H, std::chrono::duration<double, std::milli>(r1 - r0).count());
  else if (progressive == 0)
    printf("rendered %dx%d x %d spp in %.3f ms\n", W, H, spp, std::chrono::duration<double, std::milli>(r1 - r0).count());
  if (!out_path.empty() || !png_path.empty()) {
    std::vector<float> rgba((size_t)W * H * 4);
    // With the display transform a filter writes into this image, which pt_display then reads
    // (null: the library-owned one, read back as ever); src is the device image -png shows.
    const bool shown = display && !png_path.empty();
    void* filtered = nullptr;
    const void* src = nullptr;   // null: the accumulation image
    const bool filters = (temporal > 0 && progressive == 0) ? (temporal_spatial || denoise_var)
                                                            : (denoise_var || denoise);
    if ((shown || upsample) && filters && hipMalloc(&filtered, rgba.size() * sizeof(float)) != hipSuccess) {
      fprintf(stderr, "no device memory for the filtered image\n");
      return 1;
    }
    if (temporal > 0 && progressive == 0) {
      if (temporal_spatial) check(pt_temporal_denoise_spatial(ctx, nullptr, nullptr, filtered), "temporal denoise spatial");
      else if (denoise_var) check(pt_temporal_denoise(ctx, nullptr, filtered), "temporal denoise");
      else src = pt_temporal_device_ptr(ctx, 0);
      if (!filters) check(pt_read_temporal(ctx, rgba.data(), nullptr, nullptr), "read temporal");
    } else if (adaptive && denoise_var) {
      check(pt_adaptive_denoise(ctx, nullptr, filtered), "adaptive denoise");
    } else if (denoise_var) {
      check(pt_denoise_var(ctx, nullptr, filtered), "denoise-var");
    } else if (denoise) {
      check(pt_denoise(ctx, nullptr, nullptr, filtered), "denoise");
    } else {
      check(pt_read_accum(ctx, rgba.data(), rgba.size()), "read");
    }
    if (filters && !filtered) check(pt_read_denoised(ctx, rgba.data(), rgba.size()), "read denoised");
    if (filtered) {
      src = filtered;
      check(pt_synchronize(ctx), "sync");
      if (hipMemcpy(rgba.data(), filtered, rgba.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        fprintf(stderr, "copy of the filtered image failed\n");
        return 1;
      }
    }
    // the frame written: the rendered one, or with -upsample the full-size one of the image src names
    int FW = W, FH = H;
    if (upsample) {
      pt_upsample_params up;
      pt_upsample_default_params(&up);
      up.scale = upsample;
      FW = W * upsample;
      FH = H * upsample;
      if (!out_path.empty() || !shown) {
        check(pt_upsample(ctx, &up, src, nullptr), "upsample");
        rgba.resize((size_t)FW * FH * 4);
        check(pt_read_upsampled(ctx, rgba.data(), rgba.size()), "read upsampled");
      }
      if (shown) check(pt_upsample_display(ctx, &up, &dp, src, nullptr), "upsample display");
      printf("upsampled %dx%d to %dx%d\n", W, H, FW, FH);
    }
    if (!out_path.empty()) check(pt_write_image(out_path.c_str(), rgba.data(), FW, FH, PT_IMAGE_PFM), "write pfm");
    if (shown) {
      std::vector<unsigned char> rgba8((size_t)FW * FH * 4);
      if (upsample) {
        check(pt_read_display_upsampled(ctx, rgba8.data(), rgba8.size()), "read upsampled display");
      } else {
        check(pt_display(ctx, &dp, src, nullptr), "display");
        check(pt_read_display(ctx, rgba8.data(), rgba8.size()), "read display");
      }
      check(pt_write_png8(png_path.c_str(), rgba8.data(), FW, FH), "write png");
      if (dp.auto_exposure) {
        float scale = 0.0f;
        uint32_t n = 0;
        check(pt_display_exposure(ctx, &scale, &n), "display exposure");
        printf("display: auto exposure %.6g from %u metered pixels\n", scale, n);
      }
    } else if (!png_path.empty()) {
      check(pt_write_image(png_path.c_str(), rgba.data(), FW, FH, PT_IMAGE_PNG), "write png");
    }
    if (filtered) (void)hipFree(filtered);
  }
  if (!guide_path.empty()) {
    std::vector<float> guide((size_t)W * H * 4);
    check(pt_render_guide(ctx), "render guide");
    check(pt_read_guide(ctx, guide.data(), guide.size()), "read guide");
    check(pt_write_image(guide_path.c_str(), guide.data(), W, H, PT_IMAGE_PFM), "write guide pfm");
  }
  pt_destroy(ctx);
  pt_scene_free(scene);
  return 0;
}
