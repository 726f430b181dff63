// pt_scene_api.cpp — the host scene layer behind the C ABI (include/pathtracer.h):
// pt_scene_* (OBJ loading, the BVH build, the binary scene cache), the image
// writer and the light and camera helpers.  Nothing here touches a context
// but pt_scene_upload, which goes through the public pt_upload_scene.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pt_context.h"
#include "pt_display.h"
#include "scene/bvh.h"
#include "scene/camera.h"
#include "scene/light.h"
#include "scene/obj_loader.h"

struct pt_scene {
  pt::ObjScene obj;
  std::vector<uint32_t> bvh_indices;
  std::vector<pt::BVHNode> nodes;
  uint32_t flags = 0;
};

extern "C" {

int pt_scene_load_obj(const char* path, pt_scene** out) {
  if (!path || !out) return fail(PT_ERR_INVALID, "null argument");
  pt_scene* s = new pt_scene();
  std::string err;
  if (pt::load_obj_file(path, &s->obj, &err) != 0) {
    delete s;
    return fail(PT_ERR_IO, err);
  }
  *out = s;
  return PT_OK;
}

int pt_scene_parse_obj(const char* text, size_t len, pt_scene** out) {
  if (!text || !out) return fail(PT_ERR_INVALID, "null argument");
  pt_scene* s = new pt_scene();
  std::string err;
  if (pt::parse_obj(text, len, &s->obj, &err) != 0) {
    delete s;
    return fail(PT_ERR_IO, err);
  }
  *out = s;
  return PT_OK;
}

int pt_scene_from_arrays(const float* v, size_t nvf, const uint32_t* idx, size_t ni, pt_scene** out) {
  if (!out || (nvf && !v) || (ni && !idx)) return fail(PT_ERR_INVALID, "null argument");
  if (nvf % 3 || ni % 3) return fail(PT_ERR_SCENE, "sizes must be multiples of 3");
  pt_scene* s = new pt_scene();
  s->obj.vertices.assign(v, v + nvf);
  s->obj.indices.assign(idx, idx + ni);
  s->obj.materialIds.assign(ni / 3, 0u);
  *out = s;
  return PT_OK;
}

int pt_scene_build_bvh(pt_scene* s, uint32_t flags, int threads) {
  if (!s) return fail(PT_ERR_INVALID, "null scene");
  const size_t ni = s->obj.indices.size();
  if (ni == 0 || ni % 3) return fail(PT_ERR_SCENE, "scene has no triangles");
  pt::BVHOptions o;
  o.encoding = (flags & PT_NODES_INT_BITS) ? pt::BVHEncoding::kIntBits : pt::BVHEncoding::kFloat;
  o.threads = threads;
  s->bvh_indices.assign(ni, 0);
  s->nodes.assign(2 * (ni / 3) - 1, pt::BVHNode{});
  std::string err;
  if (pt::build_bvh(s->obj.vertices.data(), s->obj.vertices.size(), s->obj.indices.data(), ni,
                    s->bvh_indices.data(), s->nodes.data(), o, &err) != 0) {
    s->bvh_indices.clear();
    s->nodes.clear();
    return fail(PT_ERR_SCENE, err);
  }
  s->flags = flags;
  return PT_OK;
}

int pt_scene_counts(const pt_scene* s, size_t* nvf, size_t* ni, size_t* nn, size_t* nuv, size_t* nmat) {
  if (!s) return fail(PT_ERR_INVALID, "null scene");
  if (nvf) *nvf = s->obj.vertices.size();
  if (ni) *ni = s->obj.indices.size();
  if (nn) *nn = s->nodes.size();
  if (nuv) *nuv = s->obj.texcoords.size();
  if (nmat) *nmat = s->obj.materialIds.size();
  return PT_OK;
}

int pt_scene_copy(const pt_scene* s, float* v, uint32_t* idx, pt_bvh_node* nodes, float* uvs, uint32_t* mat) {
  if (!s) return fail(PT_ERR_INVALID, "null scene");
  if (v) memcpy(v, s->obj.vertices.data(), s->obj.vertices.size() * 4);
  if (idx) {
    const auto& src = s->nodes.empty() ? s->obj.indices : s->bvh_indices;   // BVH order once built
    memcpy(idx, src.data(), src.size() * 4);
  }
  if (nodes) memcpy(nodes, s->nodes.data(), s->nodes.size() * sizeof(pt_bvh_node));
  if (uvs) memcpy(uvs, s->obj.texcoords.data(), s->obj.texcoords.size() * 4);
  if (mat) memcpy(mat, s->obj.materialIds.data(), s->obj.materialIds.size() * 4);
  return PT_OK;
}

int pt_scene_upload(pt_context* c, const pt_scene* s) {
  if (!c || !s) return fail(PT_ERR_INVALID, "null argument");
  if (s->nodes.empty()) return fail(PT_ERR_INVALID, "build the BVH first (pt_scene_build_bvh)");
  return pt_upload_scene(c, s->obj.vertices.data(), s->obj.vertices.size(), s->bvh_indices.data(),
                         s->bvh_indices.size(), (const pt_bvh_node*)s->nodes.data(), s->nodes.size(),
                         s->obj.texcoords.data(), s->obj.texcoords.size(), s->obj.materialIds.data(),
                         s->obj.materialIds.size(), s->flags);
}

// ---- binary scene cache ---------------------------------
// Skips OBJ parsing and the BVH build for large meshes.  Layout: "PTSCENE1",
// u32 version, u32 flags (PT_NODES_INT_BITS), u64 counts of vertex floats,
// OBJ indices, BVH-order indices, nodes, uv floats, material ids, u64 shapes,
// then the six arrays, then a u64 FNV-1a hash of everything before it (taken
// over 8-byte words, the tail bytewise).
namespace {
constexpr char kCacheMagic[8] = {'P', 'T', 'S', 'C', 'E', 'N', 'E', '1'};
constexpr uint32_t kCacheVersion = 1;

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void add(const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
      uint64_t w;
      memcpy(&w, b + i, 8);
      h = (h ^ w) * 1099511628211ull;
    }
    for (; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
};
}  // namespace

int pt_scene_save(const pt_scene* s, const char* path) {
  if (!s || !path) return fail(PT_ERR_INVALID, "null argument");
  if (s->nodes.empty()) return fail(PT_ERR_INVALID, "build the BVH first (pt_scene_build_bvh)");
  FILE* f = fopen(path, "wb");
  if (!f) return fail(PT_ERR_IO, std::string("cannot create ") + path);
  Fnv h;
  bool ok = true;
  auto put = [&](const void* p, size_t n) {
    if (n && ok) ok = fwrite(p, 1, n, f) == n;
    h.add(p, n);
  };
  const uint64_t counts[7] = {s->obj.vertices.size(), s->obj.indices.size(), s->bvh_indices.size(), s->nodes.size(),
                              s->obj.texcoords.size(), s->obj.materialIds.size(), (uint64_t)s->obj.shapes};
  put(kCacheMagic, 8);
  put(&kCacheVersion, 4);
  put(&s->flags, 4);
  put(counts, sizeof counts);
  put(s->obj.vertices.data(), counts[0] * 4);
  put(s->obj.indices.data(), counts[1] * 4);
  put(s->bvh_indices.data(), counts[2] * 4);
  put(s->nodes.data(), counts[3] * sizeof(pt::BVHNode));
  put(s->obj.texcoords.data(), counts[4] * 4);
  put(s->obj.materialIds.data(), counts[5] * 4);
  const uint64_t digest = h.h;
  if (ok) ok = fwrite(&digest, 1, 8, f) == 8;
  if (fclose(f) != 0) ok = false;
  if (!ok) return fail(PT_ERR_IO, std::string("write failed: ") + path);
  return PT_OK;
}

int pt_scene_load_cache(const char* path, pt_scene** out) {
  if (!path || !out) return fail(PT_ERR_INVALID, "null argument");
  *out = nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) return fail(PT_ERR_IO, std::string("cannot open ") + path);
  Fnv h;
  bool ok = true;
  auto get = [&](void* p, size_t n) {
    if (n && ok) ok = fread(p, 1, n, f) == n;
    if (ok) h.add(p, n);
  };
  char magic[8];
  uint32_t version = 0, flags = 0;
  uint64_t counts[7] = {0};
  get(magic, 8);
  get(&version, 4);
  get(&flags, 4);
  get(counts, sizeof counts);
  if (!ok || memcmp(magic, kCacheMagic, 8) != 0 || version != kCacheVersion) {
    fclose(f);
    return fail(PT_ERR_IO, std::string("not a scene cache (or another version): ") + path);
  }
  const uint64_t nt = counts[1] / 3;
  if (counts[0] % 3 || counts[1] % 3 || counts[1] == 0 || counts[2] != counts[1] || counts[3] != 2 * nt - 1 ||
      counts[5] > (1ull << 34) || counts[0] > (1ull << 36) || counts[4] > (1ull << 36)) {
    fclose(f);
    return fail(PT_ERR_IO, std::string("inconsistent scene cache header: ") + path);
  }
  pt_scene* s = new pt_scene();
  s->flags = flags;
  s->obj.vertices.resize(counts[0]);
  s->obj.indices.resize(counts[1]);
  s->bvh_indices.resize(counts[2]);
  s->nodes.resize(counts[3]);
  s->obj.texcoords.resize(counts[4]);
  s->obj.materialIds.resize(counts[5]);
  s->obj.shapes = (size_t)counts[6];
  get(s->obj.vertices.data(), counts[0] * 4);
  get(s->obj.indices.data(), counts[1] * 4);
  get(s->bvh_indices.data(), counts[2] * 4);
  get(s->nodes.data(), counts[3] * sizeof(pt::BVHNode));
  get(s->obj.texcoords.data(), counts[4] * 4);
  get(s->obj.materialIds.data(), counts[5] * 4);
  uint64_t digest = 0;
  const uint64_t want = h.h;
  if (ok) ok = fread(&digest, 1, 8, f) == 8;
  fclose(f);
  if (!ok || digest != want) {
    delete s;
    return fail(PT_ERR_IO, std::string("scene cache truncated or corrupt: ") + path);
  }
  *out = s;
  return PT_OK;
}

// ---- image output ----------------------------------------
namespace {
uint32_t crc32_update(uint32_t crc, const unsigned char* p, size_t n) {
  static uint32_t table[256];
  static bool init = false;
  if (!init) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      table[i] = c;
    }
    init = true;
  }
  for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
  return crc;
}

void put_be32(std::vector<unsigned char>* o, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) o->push_back((unsigned char)(v >> s));
}

void png_chunk(FILE* f, const char* type, const std::vector<unsigned char>& data, bool* ok) {
  std::vector<unsigned char> buf;
  put_be32(&buf, (uint32_t)data.size());
  buf.insert(buf.end(), type, type + 4);
  buf.insert(buf.end(), data.begin(), data.end());
  const uint32_t crc = crc32_update(0xffffffffu, buf.data() + 4, buf.size() - 4) ^ 0xffffffffu;
  put_be32(&buf, crc);
  if (*ok) *ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
}

// An 8-bit RGB PNG of a W x H image, zlib stream of stored (uncompressed) deflate blocks; rows
// top-to-bottom, so the buffer's last row comes first.  channel(pixel, c): the byte of channel c.
extern "C++" template <class Channel>
bool write_png(FILE* f, int w, int h, const Channel& channel) {
  bool ok = true;
  static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  ok = fwrite(sig, 1, 8, f) == 8;
  std::vector<unsigned char> ihdr;
  put_be32(&ihdr, (uint32_t)w);
  put_be32(&ihdr, (uint32_t)h);
  ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});   // 8-bit, truecolour, deflate, filter 0, no interlace
  png_chunk(f, "IHDR", ihdr, &ok);
  std::vector<unsigned char> raw;
  raw.reserve((size_t)h * (1 + 3 * (size_t)w));
  for (int y = h - 1; y >= 0; --y) {
    raw.push_back(0);   // filter: none
    for (int x = 0; x < w; ++x)
      for (int c = 0; c < 3; ++c) raw.push_back(channel((size_t)y * w + x, c));
  }
  std::vector<unsigned char> z = {0x78, 0x01};
  uint32_t a = 1, b = 0;   // Adler-32
  for (size_t i = 0; i < raw.size(); ++i) {
    a = (a + raw[i]) % 65521u;
    b = (b + a) % 65521u;
  }
  for (size_t off = 0; off < raw.size() || off == 0; off += 65535) {
    const size_t n = std::min<size_t>(65535, raw.size() - off);
    z.push_back(off + n >= raw.size() ? 1 : 0);
    z.push_back((unsigned char)(n & 0xff));
    z.push_back((unsigned char)(n >> 8));
    z.push_back((unsigned char)(~n & 0xff));
    z.push_back((unsigned char)((~n >> 8) & 0xff));
    z.insert(z.end(), raw.begin() + (long)off, raw.begin() + (long)(off + n));
    if (raw.empty()) break;
  }
  put_be32(&z, (b << 16) | a);
  png_chunk(f, "IDAT", z, &ok);
  png_chunk(f, "IEND", {}, &ok);
  return ok;
}
}  // namespace

int pt_write_image(const char* path, const float* rgba, int w, int h, int format) {
  if (!path || !rgba) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0) return fail(PT_ERR_INVALID, "bad resolution");
  if (format != PT_IMAGE_PFM && format != PT_IMAGE_PNG) return fail(PT_ERR_INVALID, "unknown image format");
  FILE* f = fopen(path, "wb");
  if (!f) return fail(PT_ERR_IO, std::string("cannot create ") + path);
  bool ok = true;
  if (format == PT_IMAGE_PFM) {
    // rows bottom-to-top: row y = 0 of the accumulation buffer is written first
    ok = fprintf(f, "PF\n%d %d\n-1.0\n", w, h) > 0;
    std::vector<float> rgb((size_t)w * 3);
    for (int y = 0; y < h && ok; ++y) {
      for (int x = 0; x < w; ++x)
        for (int c = 0; c < 3; ++c) rgb[(size_t)x * 3 + c] = rgba[((size_t)y * w + x) * 4 + c];
      ok = fwrite(rgb.data(), 4, rgb.size(), f) == rgb.size();
    }
  } else {
    // the sRGB code of the colours clamped to [0,1] (pt_display.h srgb8_pow)
    ok = write_png(f, w, h, [&](size_t i, int c) { return ptdp::srgb8_pow(rgba[i * 4 + c]); });
  }
  if (fclose(f) != 0) ok = false;
  if (!ok) return fail(PT_ERR_IO, std::string("write failed: ") + path);
  return PT_OK;
}

int pt_write_png8(const char* path, const unsigned char* rgba8, int w, int h) {
  if (!path || !rgba8) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0) return fail(PT_ERR_INVALID, "bad resolution");
  FILE* f = fopen(path, "wb");
  if (!f) return fail(PT_ERR_IO, std::string("cannot create ") + path);
  bool ok = write_png(f, w, h, [&](size_t i, int c) { return rgba8[i * 4 + c]; });
  if (fclose(f) != 0) ok = false;
  if (!ok) return fail(PT_ERR_IO, std::string("write failed: ") + path);
  return PT_OK;
}

int pt_scene_free(pt_scene* s) {
  delete s;
  return PT_OK;
}

int pt_pack_light(const float pos[3], const float nrm[3], const float inten[3], const float size[2],
                  pt_area_light* out) {
  if (!pos || !nrm || !inten || !size || !out) return fail(PT_ERR_INVALID, "null argument");
  pt::Light l({{pos[0], pos[1], pos[2]}}, {{nrm[0], nrm[1], nrm[2]}}, {{inten[0], inten[1], inten[2]}},
              {{size[0], size[1]}});
  memcpy(out, &l.getLights()[0], sizeof *out);
  return PT_OK;
}

int pt_default_camera(float ubo[16]) {
  if (!ubo) return fail(PT_ERR_INVALID, "null argument");
  pt::Camera cam;
  cam.toUBO(ubo);
  return PT_OK;
}

}  // extern "C"
