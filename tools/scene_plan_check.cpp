// tools/scene_plan_check.cpp -- the host-only decisions of a scene upload (fredholm_amd/csrc/scene_plan_host.h) as a stand-alone program, for the tests and the host
// sanitizers.  From the repository root:
//   g++ -std=c++17 -O1 -Wall -Werror -ffp-contract=off tools/scene_plan_check.cpp -o scene_plan_check && ./scene_plan_check
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/scene_plan_check.cpp -o scene_plan_check && ./scene_plan_check
// Needs no GPU and no library.  (a) the cases the code's own comments state, derived by hand; (b) every row of tests/golden/scene_plan_cases.json (or of the file given
// as the argument): inputs and what the same lines gave while they were still inside capi.hip's rebuild_device_scene and upload_textures, equal to the last bit
// (tools/README.md says how the file was made).  Every value of the file is an unsigned integer; a float is its IEEE-754 bit pattern, a texture id its 32-bit
// pattern, the value of an environment variable its index in `vocab` below.  Textures and whole scenes are not in the file: a row names the seed and the kind that
// gen_texture / gen_scene below make them from, and holds the FNV-1a hashes of what the plan must give for them.  Prints "scene_plan_check: ok" or the number of failures.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../fredholm_amd/csrc/scene_plan_host.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

typedef unsigned long long u64;
static float as_float(u64 bits) { const uint32_t u = (uint32_t)bits; float f; std::memcpy(&f, &u, 4); return f; }
static u64 float_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// values of the environment variables in the table (0: not set)
static const char* const vocab[] = {nullptr, "", "0", "1", "00", "01", "no", "off"};
static const u64 n_vocab = sizeof vocab / sizeof vocab[0];
static const uint32_t kMaxClasses = 8u;  // fh_device.h
static const char* const messages[] = {nullptr, "fh_scene_upload: missing arrays", "fh_scene_upload: material references a texture id outside [0, n_textures)",
                                       "fh_scene_upload: n_textures > 0 but textures == NULL", "fh_scene_upload: empty texture", "instance id out of range", "material id out of range",
                                       "vertex index out of range"};
static const u64 n_messages = sizeof messages / sizeof messages[0];

// ---- what the rows name instead of holding it: textures and scenes from a seed
static uint32_t rng(u64& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

static std::vector<uint8_t> gen_texture(uint32_t w, uint32_t h, u64 seed, uint32_t mode)
{
  std::vector<uint8_t> t((size_t)w * h * 4);
  u64 s = seed;
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x)
      for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t r = rng(s);
        uint32_t b = 0;
        switch (mode) {
          case 0: b = r & 255u; break;                                  // anything
          case 1: b = 128u + (r & 127u); break;                         // every byte passes
          case 2: b = r & 127u; break;                                  // no byte passes
          case 3: b = 126u + (r & 3u); break;                           // around the threshold of a linear channel
          case 4: b = x < w / 2 ? 200u + (r & 31u) : (r & 63u); break;  // the left half passes, the right half does not
          case 5: b = y < h / 2 ? 255u : 0u; break;                     // the upper half passes
          case 6: b = 186u + (r & 3u); break;                           // around the threshold of an sRGB channel
          default: b = ((x / 8 + y / 8) & 1u) ? 255u : 0u; break;       // 8 x 8 blocks
        }
        t[((size_t)y * w + x) * 4 + c] = (uint8_t)b;
      }
  return t;
}

static fh_material plain_material()
{
  fh_material m;
  std::memset(&m, 0, sizeof m);
  m.base_color_texture_id = m.specular_color_texture_id = m.specular_roughness_texture_id = m.metalness_texture_id = m.metallic_roughness_texture_id = m.coat_texture_id = -1;
  m.coat_roughness_texture_id = m.emission_texture_id = m.heightmap_texture_id = m.normalmap_texture_id = m.alpha_texture_id = -1;
  return m;
}

struct Scene {  // owns what its descriptor points to
  std::vector<float> vertices, normals, texcoords, o2w, w2o;
  std::vector<uint32_t> indices, material_ids, instance_ids;
  std::vector<fh_material> materials;
  std::vector<std::vector<uint8_t>> texels;
  std::vector<fh_texture_desc> textures;
  fh_scene_desc desc;
};

// kind 0: a valid scene; 1-9: the same scene with one thing wrong (or several: the first in the order of the checks is reported)
static void gen_scene(u64 seed, uint32_t kind, Scene& sc)
{
  u64 s = seed;
  static const float levels[] = {0.0f, 0.0f, 0.5f, 1.0f, 1.0f, 2.0f, -1.0f, 0.25f};
  static const uint32_t sizes[] = {1u, 3u, 8u, 16u, 64u};
  static const float wild[] = {1e31f, -1e31f, 1e7f, -2e6f, INFINITY, NAN, 3e38f, 9.9e5f};
  auto level = [&]() { return levels[rng(s) & 7u]; };
  const uint32_t n_tex = rng(s) % 4u;
  sc.texels.resize(n_tex);
  sc.textures.resize(n_tex);
  for (uint32_t i = 0; i < n_tex; ++i) {
    const uint32_t w = sizes[rng(s) % 5u], h = sizes[rng(s) % 5u], mode = rng(s) % 8u;
    sc.texels[i] = gen_texture(w, h, rng(s), mode);
    sc.textures[i] = fh_texture_desc{w, h, sc.texels[i].data(), (int32_t)(rng(s) & 1u)};
  }
  auto tex_id = [&](uint32_t one_in) { return (n_tex && rng(s) % one_in == 0) ? (int32_t)(rng(s) % n_tex) : -1; };
  const uint32_t nm = 1u + rng(s) % 12u;
  sc.materials.assign(nm, plain_material());
  for (fh_material& m : sc.materials) {
    m.diffuse = level(); m.specular = level(); m.metalness = level(); m.coat = level(); m.transmission = level(); m.sheen = level(); m.subsurface = level(); m.thin_walled = level();
    for (int k = 0; k < 3; ++k) { m.base_color[k] = level(); m.specular_color[k] = level(); m.sheen_color[k] = level(); m.coat_color[k] = level(); }
    if (rng(s) % 5u == 0) for (int k = 0; k < 3; ++k) m.emission_color[k] = level();
    m.base_color_texture_id = tex_id(2); m.alpha_texture_id = tex_id(3); m.metalness_texture_id = tex_id(6); m.metallic_roughness_texture_id = tex_id(8);
    m.specular_color_texture_id = tex_id(6); m.coat_texture_id = tex_id(6); m.emission_texture_id = tex_id(9); m.normalmap_texture_id = tex_id(9);
  }
  const uint32_t nv = 3u + rng(s) % 40u, nf = rng(s) % 60u;
  const bool some_wild = rng(s) % 4u == 0;
  const float spread = (rng(s) & 1u) ? 0.25f : 3.0f;
  sc.vertices.resize(3ull * nv); sc.normals.resize(3ull * nv); sc.texcoords.resize(2ull * nv);
  for (float& v : sc.vertices) v = (float)(rng(s) & 1023u) / 64.0f - 8.0f;
  for (float& v : sc.normals) v = (float)(rng(s) & 1023u) / 512.0f - 1.0f;
  for (float& v : sc.texcoords) v = (some_wild && rng(s) % 16u == 0) ? wild[rng(s) & 7u] : ((float)(rng(s) & 0xffffu) / 65536.0f - 0.4f) * spread;
  const uint32_t ni_given = rng(s) % 4u;  // 0: no transforms, one identity
  sc.o2w.assign(12ull * ni_given, 0.0f); sc.w2o.assign(12ull * ni_given, 0.0f);
  for (uint32_t i = 0; i < ni_given; ++i)
    for (int k = 0; k < 3; ++k) sc.o2w[12 * i + 5 * k] = sc.w2o[12 * i + 5 * k] = 1.0f;
  const uint32_t ni = ni_given ? ni_given : 1u;
  const bool with_instance_ids = (rng(s) & 1u) != 0;
  sc.indices.resize(3ull * nf); sc.material_ids.resize(nf); sc.instance_ids.resize(with_instance_ids ? nf : 0u);
  for (uint32_t& v : sc.indices) v = rng(s) % nv;
  for (uint32_t& v : sc.material_ids) v = rng(s) % nm;
  for (uint32_t& v : sc.instance_ids) v = rng(s) % ni;
  const uint32_t where = nf ? rng(s) % nf : 0u, corner = rng(s) % 3u;
  if (nf) {
    if (kind == 1 || kind == 8) sc.indices[3ull * where + corner] = nv;
    if (kind == 2 || kind == 8) sc.material_ids[where] = nm;
    if ((kind == 3 || kind == 8) && with_instance_ids) sc.instance_ids[where] = ni;
    if (kind == 8 && where) sc.indices[3ull * (where - 1u)] = nv + 7u;  // (an earlier face's fault comes first)
  }
  if (kind == 4 && n_tex) sc.textures[rng(s) % n_tex].width = 0;
  if (kind == 6) sc.materials[rng(s) % nm].normalmap_texture_id = (int32_t)n_tex;
  if (kind == 9) sc.materials[rng(s) % nm].coat_roughness_texture_id = -2;
  fh_scene_desc& d = sc.desc;
  d.n_vertices = nv; d.vertices = kind == 5 ? nullptr : sc.vertices.data(); d.normals = sc.normals.data(); d.texcoords = sc.texcoords.data();
  d.n_faces = nf; d.indices = sc.indices.data(); d.material_ids = sc.material_ids.data(); d.instance_ids = with_instance_ids ? sc.instance_ids.data() : nullptr;
  d.n_materials = nm; d.materials = sc.materials.data();
  d.n_instances = ni_given; d.object_to_world = ni_given ? sc.o2w.data() : nullptr; d.world_to_object = ni_given ? sc.w2o.data() : nullptr;
  d.n_textures = n_tex; d.textures = (kind == 7 || !n_tex) ? nullptr : sc.textures.data();
}

static u64 fnv(const void* p, size_t n, u64 h = 1469598103934665603ull)
{
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return (h ^ (h >> 32)) & 0xffffffffull;  // (folded to 32 bits: the table stays small)
}
template <typename T> static u64 fnv_of(const std::vector<T>& v, u64 h = 1469598103934665603ull) { return v.empty() ? h : fnv(v.data(), v.size() * sizeof(T), h); }

static fh::SceneSwitches no_switches() { return fh::scene_switches(nullptr, nullptr, nullptr); }

// one face over the unit square of texture coordinates scaled by `scale` and moved by (du, dv), with the given material; the plan of that one-face scene
static fh::ScenePlan one_face_plan(const fh_material& m, const std::vector<fh_texture_desc>& tex, const float uv[6], const fh::SceneSwitches& sw)
{
  const float pos[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, nrm[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1};
  const uint32_t idx[3] = {0, 1, 2}, mid[1] = {0};
  fh_scene_desc d;
  std::memset(&d, 0, sizeof d);
  d.n_vertices = 3; d.vertices = pos; d.normals = nrm; d.texcoords = uv;
  d.n_faces = 1; d.indices = idx; d.material_ids = mid;
  d.n_materials = 1; d.materials = &m;
  d.n_textures = (uint32_t)tex.size(); d.textures = tex.empty() ? nullptr : tex.data();
  return fh::plan_scene(&d, sw, kMaxClasses);
}

static void hand_derived()
{
  const fh::SceneSwitches off = no_switches();
  EXPECT(off.opacity_classes && off.micromap && !off.debug);
  EXPECT(!fh::scene_switches("0", nullptr, nullptr).opacity_classes && !fh::scene_switches("0", "1", nullptr).micromap);  // no classes, no micromap
  EXPECT(fh::scene_switches(nullptr, "0", "").opacity_classes && !fh::scene_switches(nullptr, "0", "").micromap && fh::scene_switches(nullptr, "0", "").debug);

  // byte 128 (0.50196) passes, byte 127 (0.49804) does not: a 4 x 4 texture of one byte, any footprint
  std::vector<uint8_t> t128(64, 128), t127(64, 127), mixed(64, 128);
  mixed[4 * 5 + 3] = 127;  // texel (1, 1), alpha
  const float mid_uv[6] = {0.3f, 0.3f, 0.6f, 0.3f, 0.3f, 0.6f};
  EXPECT(fh::footprint_class(t128.data(), 4, 4, 3, nullptr, mid_uv, 3) == 1u && fh::footprint_class(t127.data(), 4, 4, 3, nullptr, mid_uv, 3) == 2u);
  EXPECT(fh::footprint_class(mixed.data(), 4, 4, 3, nullptr, mid_uv, 3) == 0u && fh::footprint_class(mixed.data(), 4, 4, 0, nullptr, mid_uv, 3) == 1u);
  EXPECT(fh::footprint_class(nullptr, 4, 4, 3, nullptr, mid_uv, 3) == 0u && fh::footprint_class(t128.data(), 0, 4, 3, nullptr, mid_uv, 3) == 0u);
  // a whole texture of 128 can cut by the 0.501 rule (0.50196 < 0.501 is false: it cannot); 127 can
  EXPECT(fh::texture_cuts(fh_texture_desc{4, 4, t128.data(), 0}).alpha == 0 && fh::texture_cuts(fh_texture_desc{4, 4, t127.data(), 0}).alpha == 1);
  EXPECT(fh::texture_cuts(fh_texture_desc{4, 4, t128.data(), 0}).red == 0 && fh::texture_cuts(fh_texture_desc{4, 4, t128.data(), 1}).red == 1);  // (sRGB 128 decodes to 0.216)
  // an sRGB-decoded value between the two thresholds decides nothing
  float between[256];
  for (int i = 0; i < 256; ++i) between[i] = 0.5f;
  EXPECT(fh::footprint_class(t128.data(), 4, 4, 0, between, mid_uv, 3) == 0u);
  // huge or infinite coordinates are left to the test (a NaN never gets here: a face that has one is wild, plan_faces)
  const float huge_uv[6] = {0.3f, 0.3f, 1e6f, 0.3f, 0.3f, 0.6f}, inf_uv[6] = {0.3f, 0.3f, 0.6f, -INFINITY, 0.3f, 0.6f};
  EXPECT(fh::footprint_class(t128.data(), 4, 4, 3, nullptr, huge_uv, 3) == 0u && fh::footprint_class(t128.data(), 4, 4, 3, nullptr, inf_uv, 3) == 0u);

  // texel columns of [lo, hi] on n texels: floor(u n - 0.5 - slack) .. floor(u n - 0.5 + slack) + 1.  u in [0.3, 0.6] of 16: 4.3 -> 4, 9.1 -> 9 + 1: columns 4 .. 10
  int first = -1, count = -1;
  fh::texel_span(0.3f, 0.6f, 16u, first, count);
  EXPECT(first == 4 && count == 7);
  // a footprint that wraps: u in [0.95, 1.1] of 16 texels: 14.7 -> 14, 17.1 -> 17 + 1: columns 14, 15, 0, 1, 2
  fh::texel_span(0.95f, 1.1f, 16u, first, count);
  EXPECT(first == 14 && count == 5);
  fh::texel_span(-0.05f, 0.02f, 16u, first, count);  // -1.3 - slack -> -2 = column 14; -0.18 + slack -> -1, + 1 -> 0
  EXPECT(first == 14 && count == 3);
  // a span as wide as the texture or wider: all of it, from column 0
  fh::texel_span(0.0f, 1.0f, 16u, first, count);
  EXPECT(first == 0 && count == 16);
  fh::texel_span(-3.0f, 5.5f, 16u, first, count);
  EXPECT(first == 0 && count == 16);
  fh::texel_span(0.2f, 0.2f, 1u, first, count);
  EXPECT(first == 0 && count == 1);
  // the wrapped footprint reads the texels it names: a 16 x 1 texture that fails in column 1 only
  std::vector<uint8_t> stripe(64, 255);
  stripe[4 * 1 + 3] = 0;
  const float wrap_uv[6] = {0.95f, 0.5f, 1.1f, 0.5f, 1.0f, 0.5f}, short_uv[6] = {0.95f, 0.5f, 1.0f, 0.5f, 0.97f, 0.5f}, clear_uv[6] = {0.3f, 0.5f, 0.6f, 0.5f, 0.4f, 0.5f};
  EXPECT(fh::footprint_class(stripe.data(), 16, 1, 3, nullptr, wrap_uv, 3) == 0u);   // columns 14 .. 2
  EXPECT(fh::footprint_class(stripe.data(), 16, 1, 3, nullptr, short_uv, 3) == 1u);  // 1.0 -> 15.5 + slack -> 15, + 1 -> 16: columns 14, 15, 0 and not 1
  EXPECT(fh::footprint_class(stripe.data(), 16, 1, 3, nullptr, clear_uv, 3) == 1u);
  // more than 2^18 texels are left to the test: 1024 x 1024 opaque texels, a face over all of them against one over a 512 x 512 corner
  std::vector<uint8_t> big((size_t)1024 * 1024 * 4, 255);
  const float all_uv[6] = {0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f}, corner_uv[6] = {0.01f, 0.01f, 0.49f, 0.01f, 0.01f, 0.49f};
  EXPECT(fh::footprint_class(big.data(), 1024, 1024, 3, nullptr, all_uv, 3) == 0u);
  EXPECT(fh::footprint_class(big.data(), 1024, 1024, 3, nullptr, corner_uv, 3) == 1u);  // (492 + 2 columns) x (492 + 2 rows) < 2^18

  // two textures: one the face does not test passes by itself; never wins over mixed
  const fh::CutTexture pass{t128.data(), 4, 4, false}, fail{t127.data(), 4, 4, false}, mix{mixed.data(), 4, 4, false};
  EXPECT(fh::footprint_verdict(1u, &pass, nullptr, nullptr, mid_uv, 3) == 1u && fh::footprint_verdict(2u, nullptr, &fail, nullptr, mid_uv, 3) == 2u);
  EXPECT(fh::footprint_verdict(3u, &pass, &fail, nullptr, mid_uv, 3) == 2u && fh::footprint_verdict(3u, &mix, &fail, nullptr, mid_uv, 3) == 2u);
  EXPECT(fh::footprint_verdict(3u, &mix, &pass, nullptr, mid_uv, 3) == 0u && fh::footprint_verdict(0u, nullptr, nullptr, nullptr, mid_uv, 3) == 1u);
  EXPECT(fh::footprint_verdict(2u, &mix, &pass, nullptr, mid_uv, 3) == 1u);  // (red of `pass`; `mix` is not looked at)

  // micromap cells: cell (ci, cj) spans barycentrics [ci / 16 - 1e-4, (ci + 1) / 16 + 1e-4]; the last cell of a row or column reaches 1 + 1e-4
  const float unit_uv[6] = {0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f};
  float c[8];
  fh::cell_corners(0, 0, unit_uv, c);
  EXPECT(c[0] == (float)-1e-4 && c[1] == (float)-1e-4 && c[2] == (float)(1.0 / 16.0 + 1e-4) && c[7] == (float)(1.0 / 16.0 + 1e-4));
  fh::cell_corners(15, 0, unit_uv, c);
  EXPECT(c[0] == (float)(15.0 / 16.0 - 1e-4) && c[2] == (float)(1.0 + 1e-4) && c[6] == (float)(1.0 + 1e-4) && c[1] == (float)-1e-4);
  fh::cell_corners(3, 15, unit_uv, c);
  EXPECT(c[5] == (float)(1.0 + 1e-4) && c[7] == (float)(1.0 + 1e-4) && c[4] == (float)(3.0 / 16.0 - 1e-4));
  // a face over a texture whose left half passes and right half does not: cells of the rows near v = 0 pass on the left, never pass on the right; 136 + 15 cells are decided
  // (ci + cj <= 16, ci < 16: rows of 16, 16, 15, 14, ... 2 cells)
  std::vector<uint8_t> halves((size_t)64 * 64 * 4);
  for (uint32_t y = 0; y < 64; ++y)
    for (uint32_t x = 0; x < 64; ++x)
      for (uint32_t k = 0; k < 4; ++k) halves[((size_t)y * 64 + x) * 4 + k] = x < 32 ? 255 : 0;
  const fh::CutTexture half{halves.data(), 64, 64, false};
  const float inner_uv[6] = {0.1f, 0.1f, 0.9f, 0.1f, 0.1f, 0.9f};
  uint32_t words[16] = {};
  u64 counts[3] = {0, 0, 0};
  fh::micromap_words(1u, &half, nullptr, nullptr, inner_uv, words, counts);
  EXPECT(counts[0] == 16u + 16u + 15u + 14u + 13u + 12u + 11u + 10u + 9u + 8u + 7u + 6u + 5u + 4u + 3u + 2u);
  EXPECT((words[0] & 3u) == 1u);             // cell (0, 0): u in [0.1, 0.15]: left half
  EXPECT(((words[0] >> 30) & 3u) == 2u);     // cell (15, 0), the last of its row: u in [0.85, 0.9]: right half
  EXPECT(((words[0] >> 14) & 3u) == 0u);     // cell (7, 0): u in [0.45, 0.5] with the taps' margin: both halves
  EXPECT(((words[1] >> 30) & 3u) == 2u);     // cell (15, 1) lies on the hypotenuse (15 + 1 <= 16) and is decided
  EXPECT(((words[2] >> 30) & 3u) == 0u && ((words[2] >> 28) & 3u) == 2u);  // cell (15, 2) is beyond it and stays 0; (14, 2) is the last of row 2
  EXPECT((words[15] & 3u) == 1u && ((words[15] >> 2) & 3u) == 1u && ((words[15] >> 4) & 3u) == 0u);  // row 15: cells 0 and 1 only (u near 0.1)
  EXPECT(counts[1] + counts[2] < counts[0] && counts[1] > counts[2]);

  // lobe masks.  A full metal seen from behind refracts: transmission and diffuse transmission stay, specular / sheen / diffuse go
  fh_material m = plain_material();
  m.metalness = 1.0f; m.transmission = 0.5f; m.subsurface = 0.5f; m.thin_walled = 1.0f; m.diffuse = 1.0f; m.specular = 1.0f; m.sheen = 1.0f;
  for (int k = 0; k < 3; ++k) m.specular_color[k] = m.sheen_color[k] = 1.0f;
  EXPECT(fh::material_lobes(m) == (fh::L_METAL | fh::L_TRANS | fh::L_DT));
  m.metalness = 0.5f;
  EXPECT(fh::material_lobes(m) == (fh::L_METAL | fh::L_TRANS | fh::L_DT | fh::L_SPEC | fh::L_SHEEN | fh::L_DIFF));
  m.metalness = 1.0f; m.metalness_texture_id = 0;  // a texture on metalness: unknowable, everything stays
  EXPECT(fh::material_lobes(m) == (fh::L_METAL | fh::L_TRANS | fh::L_DT | fh::L_SPEC | fh::L_SHEEN | fh::L_DIFF));
  fh_material gltf = plain_material();  // a glTF material: coat? + metal + specular + diffuse, never the generic seven lobes
  gltf.diffuse = 1.0f; gltf.specular = 1.0f; gltf.metallic_roughness_texture_id = 0; gltf.base_color_texture_id = 1;
  for (int k = 0; k < 3; ++k) gltf.specular_color[k] = 1.0f;
  EXPECT(fh::material_lobes(gltf) == (fh::L_METAL | fh::L_SPEC | fh::L_DIFF));
  gltf.coat = 2.0f;
  EXPECT(fh::material_lobes(gltf) == (fh::L_COAT | fh::L_METAL | fh::L_SPEC | fh::L_DIFF));
  fh_material sheen = plain_material();  // sheen is "!= 0": a negative product keeps it
  sheen.sheen = -1.0f; sheen.sheen_color[1] = 1.0f;
  EXPECT(fh::material_lobes(sheen) == fh::L_SHEEN && fh::material_lobes(plain_material()) == 0u);
  EXPECT(!fh::material_emissive(plain_material()));
  fh_material em = plain_material();
  em.emission_texture_id = 0;
  EXPECT(fh::material_emissive(em));
  em.emission_texture_id = -1; em.emission_color[2] = 1e-30f;
  EXPECT(fh::material_emissive(em));

  // nine distinct lobe masks in eight classes: the ninth folds into the last class, which becomes the generic one; a tenth material with the first mask keeps class 0
  fh::MaterialRecord mats[11];
  std::memset(mats, 0, sizeof mats);
  for (uint32_t i = 0; i < 9; ++i) mats[i].lobes = i + 1u;
  mats[9].lobes = 1u; mats[10].lobes = 8u;  // (the mask class 7 had before it became generic: no class has it any more, it folds too)
  uint32_t class_lobes[8] = {};
  EXPECT(fh::shading_classes(mats, 11, kMaxClasses, class_lobes) == 8u);
  for (uint32_t i = 0; i < 7; ++i) EXPECT(mats[i].cls == i && class_lobes[i] == i + 1u);
  EXPECT(mats[7].cls == 7u && mats[8].cls == 7u && mats[9].cls == 0u && mats[10].cls == 7u && class_lobes[7] == fh::L_ALL);
  // exactly eight masks: no fold, the last class keeps its own mask
  std::memset(class_lobes, 0, sizeof class_lobes);
  EXPECT(fh::shading_classes(mats, 8, kMaxClasses, class_lobes) == 8u && class_lobes[7] == 8u && mats[7].cls == 7u);
  std::memset(class_lobes, 0, sizeof class_lobes);
  EXPECT(fh::shading_classes(mats, 3, kMaxClasses, class_lobes) == 3u && class_lobes[3] == 0u);

  // the alpha word: 1 where a texture of the material can cut, 2 where it has textures that cannot, 0 without
  const uint8_t cuts[2] = {1, 0}, none[2] = {0, 0};
  fh_material am = plain_material();
  EXPECT(fh::material_alpha(am, cuts, cuts) == 0u);
  am.base_color_texture_id = 0;
  EXPECT(fh::material_alpha(am, cuts, none) == 1u && fh::material_alpha(am, none, cuts) == 2u);
  am.base_color_texture_id = 1; am.alpha_texture_id = 0;
  EXPECT(fh::material_alpha(am, cuts, none) == 2u && fh::material_alpha(am, none, cuts) == 1u);

  // one face, one texture: the class byte and the counters of each verdict, and a wild coordinate that brings the test back for an opaque texture
  fh_material fm = plain_material();
  fm.base_color_texture_id = 0; fm.diffuse = 1.0f;
  const std::vector<fh_texture_desc> th = {fh_texture_desc{64, 64, halves.data(), 0}}, t_opaque = {fh_texture_desc{4, 4, t128.data(), 0}};
  const float left_uv[6] = {0.1f, 0.1f, 0.4f, 0.1f, 0.1f, 0.4f}, right_uv[6] = {0.6f, 0.1f, 0.9f, 0.1f, 0.6f, 0.4f}, wild_uv[6] = {0.1f, 0.1f, 0.4f, INFINITY, 0.1f, 0.4f};
  fh::ScenePlan p = one_face_plan(fm, th, left_uv, off);
  EXPECT(!p.error && p.face_cls[0] == 0x00 && !p.any_alpha && p.alpha_rec.empty() && p.alpha_face_counts[0] == 1u && p.alpha_face_counts[1] == 1u && p.alpha_face_counts[3] == 0u);
  p = one_face_plan(fm, th, right_uv, off);
  EXPECT(!p.error && p.face_cls[0] == 0x20 && !p.any_alpha && p.alpha_face_counts[2] == 1u);
  p = one_face_plan(fm, th, inner_uv, off);
  EXPECT(!p.error && p.face_cls[0] == 0x40 && p.any_alpha && p.alpha_rec.size() == 8u && p.alpha_face_counts[3] == 1u && p.alpha_cell_counts[0] == 151u);
  EXPECT(p.alpha_rec[1].z == 1u && p.alpha_rec[2].x == 0u && p.alpha_rec[2].y == 0u && p.alpha_rec[2].z == 64u && p.alpha_rec[2].w == 64u && p.alpha_rec[3].z == 0u);
  EXPECT(p.alpha_rec[0].x == float_bits(0.1f) && p.alpha_rec[0].z == float_bits(0.9f) && p.alpha_rec[1].y == float_bits(0.9f) && (p.alpha_rec[4].x & 3u) == 1u);
  p = one_face_plan(fm, th, inner_uv, fh::scene_switches(nullptr, "0", nullptr));
  EXPECT(p.any_alpha && p.alpha_cell_counts[0] == 0u && p.alpha_rec[4].x == 0u);
  p = one_face_plan(fm, th, left_uv, fh::scene_switches("0", nullptr, nullptr));
  EXPECT(p.face_cls[0] == 0x40 && p.alpha_face_counts[1] == 0u && p.alpha_face_counts[3] == 1u && p.alpha_cell_counts[0] == 0u);
  p = one_face_plan(fm, t_opaque, left_uv, off);
  EXPECT(p.materials[0].alpha == 2u && p.face_cls[0] == 0x00 && p.alpha_face_counts[0] == 0u);
  p = one_face_plan(fm, t_opaque, wild_uv, off);
  EXPECT(p.face_cls[0] == 0x40 && p.any_alpha && p.alpha_face_counts[0] == 1u && p.alpha_face_counts[3] == 1u && p.alpha_rec[1].z == 1u && p.alpha_cell_counts[0] == 0u);
  // the second texture's texels begin behind the first's: the byte offset is in the record's slot
  fh_material two = plain_material();
  two.alpha_texture_id = 1;
  const std::vector<fh_texture_desc> tt = {fh_texture_desc{4, 4, t128.data(), 0}, fh_texture_desc{64, 64, halves.data(), 1}};
  p = one_face_plan(two, tt, inner_uv, off);
  EXPECT(p.tex_offset[1] == 64u && p.texel_bytes == 64u + 16384u && p.alpha_rec[1].z == 6u && p.alpha_rec[3].x == 64u && p.alpha_rec[3].z == 64u && p.alpha_rec[2].z == 0u);
  // refusals, in their order
  EXPECT(!std::strcmp(fh::plan_scene(nullptr, off, kMaxClasses).error, messages[1]));
  fm.base_color_texture_id = 1;
  EXPECT(!std::strcmp(one_face_plan(fm, th, left_uv, off).error, messages[2]));
}

struct Row { std::string fn; std::vector<u64> in, out; };

// the fixture's own small format: a list of {"fn": name, "in": [unsigned integers], "out": [unsigned integers]}
static bool read_rows(const char* path, std::vector<Row>& rows)
{
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::string text;
  char buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
  std::fclose(f);
  auto numbers = [&](size_t& at, const char* key, std::vector<u64>& out) {
    at = text.find(key, at);
    if (at == std::string::npos) return false;
    at = text.find('[', at);
    if (at == std::string::npos) return false;
    for (++at; at < text.size() && text[at] != ']';) {
      if (text[at] >= '0' && text[at] <= '9') {
        char* end = nullptr;
        out.push_back(std::strtoull(text.c_str() + at, &end, 10));
        at = (size_t)(end - text.c_str());
      } else if (text[at] == ',' || text[at] == ' ' || text[at] == '\n') ++at;
      else return false;
    }
    return at < text.size();
  };
  for (size_t at = 0; (at = text.find("\"fn\": \"", at)) != std::string::npos;) {
    Row r;
    at += 7;
    const size_t end = text.find('"', at);
    if (end == std::string::npos) return false;
    r.fn = text.substr(at, end - at);
    at = end;
    if (!numbers(at, "\"in\":", r.in) || !numbers(at, "\"out\":", r.out)) return false;
    rows.push_back(r);
  }
  return true;
}

static const char* env_value(u64 code) { return code < n_vocab ? vocab[code] : nullptr; }
static bool texture_sane(u64 w, u64 h) { return w >= 1 && w <= 1024 && h >= 1 && h <= 1024; }
static fh_material material_of(const u64* words)
{
  fh_material m;
  uint32_t w[45];
  for (int k = 0; k < 45; ++k) w[k] = (uint32_t)words[k];
  std::memcpy(&m, w, 180);
  return m;
}

// one row against the header; false: the row's shape is wrong or a value differs
static bool replay(const Row& r)
{
  const std::vector<u64>& in = r.in;
  const std::vector<u64>& out = r.out;
  if (r.fn == "scene_switches") {  // FH_OPACITY_CLASSES, FH_OPACITY_MICROMAP, FH_DEBUG_BVH
    if (in.size() != 3 || out.size() != 3 || in[0] >= n_vocab || in[1] >= n_vocab || in[2] >= n_vocab) return false;
    const fh::SceneSwitches sw = fh::scene_switches(env_value(in[0]), env_value(in[1]), env_value(in[2]));
    return sw.opacity_classes == (out[0] != 0) && sw.micromap == (out[1] != 0) && sw.debug == (out[2] != 0);
  }
  if (r.fn == "material_emissive") return in.size() == 45 && out.size() == 1 && fh::material_emissive(material_of(in.data())) == (out[0] != 0);
  if (r.fn == "material_lobes") return in.size() == 45 && out.size() == 1 && fh::material_lobes(material_of(in.data())) == out[0];
  if (r.fn == "material_alpha") {  // base-colour texture id, alpha texture id, textures, their alpha flags, their red flags
    if (in.size() < 3 || in.size() != 3 + 2 * in[2] || out.size() != 1) return false;
    const int32_t bt = (int32_t)(uint32_t)in[0], at = (int32_t)(uint32_t)in[1];
    if (bt < -1 || at < -1 || bt >= (int32_t)in[2] || at >= (int32_t)in[2]) return false;
    std::vector<uint8_t> a(in[2] + 1), d(in[2] + 1);
    for (u64 i = 0; i < in[2]; ++i) { a[i] = (uint8_t)in[3 + i]; d[i] = (uint8_t)in[3 + in[2] + i]; }
    fh_material m = plain_material();
    m.base_color_texture_id = bt; m.alpha_texture_id = at;
    return fh::material_alpha(m, a.data(), d.data()) == out[0];
  }
  if (r.fn == "shading_classes") {  // the lobe masks of the materials; out: classes used, their masks, the class of every material
    if (in.empty() || in.size() > 64 || out.size() != 1 + in.size() || (out[0] & 15u) > kMaxClasses) return false;
    std::vector<fh::MaterialRecord> mats(in.size());
    for (size_t i = 0; i < in.size(); ++i) { std::memset(&mats[i], 0, sizeof mats[i]); mats[i].lobes = (uint32_t)in[i]; }
    uint32_t class_lobes[kMaxClasses] = {};
    const uint32_t n = fh::shading_classes(mats.data(), (uint32_t)mats.size(), kMaxClasses, class_lobes);
    u64 packed = 0;  // (eight 7-bit masks)
    for (uint32_t c = 0; c < n; ++c) packed |= (u64)class_lobes[c] << (7 * c);
    bool ok = n == (out[0] & 15u) && packed == out[0] >> 4;
    for (size_t i = 0; i < in.size(); ++i) ok = ok && mats[i].cls == out[1 + i];
    return ok;
  }
  if (r.fn == "texture_cuts") {  // width, height, seed, kind, sRGB
    if (in.size() != 5 || out.size() != 2 || !texture_sane(in[0], in[1])) return false;
    const std::vector<uint8_t> t = gen_texture((uint32_t)in[0], (uint32_t)in[1], in[2], (uint32_t)in[3]);
    const fh::TextureCuts c = fh::texture_cuts(fh_texture_desc{(uint32_t)in[0], (uint32_t)in[1], t.data(), (int32_t)in[4]});
    return c.alpha == out[0] && c.red == out[1];
  }
  if (r.fn == "texel_span") {  // lo, hi, texels
    if (in.size() != 3 || out.size() != 2 || in[2] == 0 || in[2] > (1u << 20)) return false;
    int first = -1, count = -1;
    fh::texel_span(as_float(in[0]), as_float(in[1]), (uint32_t)in[2], first, count);
    return (u64)(uint32_t)first == out[0] && (u64)(uint32_t)count == out[1];
  }
  if (r.fn == "footprint_class") {  // width, height, seed, kind, channel, sRGB decode?, points, their coordinates
    if (in.size() < 7 || in[6] < 1 || in[6] > 4 || in.size() != 7 + 2 * in[6] || out.size() != 1 || !texture_sane(in[0], in[1]) || in[4] > 3) return false;
    const std::vector<uint8_t> t = gen_texture((uint32_t)in[0], (uint32_t)in[1], in[2], (uint32_t)in[3]);
    float table[256], uv[8];
    fh::srgb_decode_table(table);
    for (u64 k = 0; k < 2 * in[6]; ++k) uv[k] = as_float(in[7 + k]);
    return fh::footprint_class(t.data(), (uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[4], in[5] ? table : nullptr, uv, (int)in[6]) == out[0];
  }
  if (r.fn == "footprint_verdict" || r.fn == "micromap_words") {  // flags, the base-colour texture (width, height, seed, kind), the alpha texture (the same, sRGB), a face's coordinates
    if (in.size() != 16 || !texture_sane(in[1], in[2]) || !texture_sane(in[5], in[6]) || in[0] > 3) return false;
    const std::vector<uint8_t> tb = gen_texture((uint32_t)in[1], (uint32_t)in[2], in[3], (uint32_t)in[4]), ta = gen_texture((uint32_t)in[5], (uint32_t)in[6], in[7], (uint32_t)in[8]);
    const fh::CutTexture base{tb.data(), (uint32_t)in[1], (uint32_t)in[2], false}, alpha{ta.data(), (uint32_t)in[5], (uint32_t)in[6], in[9] != 0};
    float table[256], uv[6];
    fh::srgb_decode_table(table);
    for (int k = 0; k < 6; ++k) uv[k] = as_float(in[10 + k]);
    if (r.fn == "footprint_verdict") return out.size() == 1 && fh::footprint_verdict((uint32_t)in[0], &base, &alpha, table, uv, 3) == out[0];
    uint32_t words[16] = {};
    u64 counts[3] = {0, 0, 0};
    fh::micromap_words((uint32_t)in[0], &base, &alpha, table, uv, words, counts);
    if (out.size() != 19) return false;
    bool ok = counts[0] == out[16] && counts[1] == out[17] && counts[2] == out[18];
    for (int k = 0; k < 16; ++k) ok = ok && words[k] == out[k];
    return ok;
  }
  if (r.fn == "cell_corners") {  // ci, cj, a face's coordinates
    if (in.size() != 8 || out.size() != 8 || in[0] > 15 || in[1] > 15) return false;
    float uv[6], c[8];
    for (int k = 0; k < 6; ++k) uv[k] = as_float(in[2 + k]);
    fh::cell_corners((int)in[0], (int)in[1], uv, c);
    bool ok = true;
    for (int k = 0; k < 8; ++k) ok = ok && float_bits(c[k]) == out[k];
    return ok;
  }
  if (r.fn == "plan_scene") {  // seed, kind, FH_OPACITY_CLASSES, FH_OPACITY_MICROMAP; out: the refusal (0: none), then the hashes and counters of every part of the plan
    if (in.size() != 4 || out.size() != 18 || in[1] > 9 || in[2] >= n_vocab || in[3] >= n_vocab || out[0] >= n_messages) return false;
    Scene sc;
    gen_scene(in[0], (uint32_t)in[1], sc);
    const fh::ScenePlan p = fh::plan_scene(&sc.desc, fh::scene_switches(env_value(in[2]), env_value(in[3]), nullptr), kMaxClasses);
    if (out[0]) return p.error && !std::strcmp(p.error, messages[out[0]]);
    if (p.error) return false;
    std::vector<uint32_t> classes(p.class_lobes.begin(), p.class_lobes.begin() + p.n_classes);
    return p.n_instances == out[1] && fnv_of(p.tex_offset, fnv_of(p.tex_red_cuts, fnv_of(p.tex_alpha_cuts))) == out[2] && p.texel_bytes == out[3] && fnv_of(p.materials) == out[4] &&
           p.n_classes == out[5] && fnv_of(classes) == out[6] && fnv_of(p.face_cls) == out[7] && fnv_of(p.face_meta) == out[8] && fnv_of(p.lights) == out[9] && p.lights.size() == out[10] &&
           p.alpha_face_counts[0] == out[11] && p.alpha_face_counts[1] == out[12] && p.alpha_face_counts[2] == out[13] && p.alpha_face_counts[3] == out[14] &&
           (u64)p.any_alpha + 2 * p.alpha_rec.size() == out[15] && fnv_of(p.alpha_rec) == out[16] &&
           fnv(p.alpha_cell_counts, sizeof p.alpha_cell_counts) == out[17];
  }
  return false;  // (a function this program does not know)
}

int main(int argc, char** argv)
{
  hand_derived();
  std::string path = argc > 1 ? argv[1] : "";
  if (path.empty()) {  // beside this file: ../tests/golden
    path = __FILE__;
    const size_t slash = path.find_last_of('/');
    path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/../tests/golden/scene_plan_cases.json";
  }
  std::vector<Row> rows;
  if (!read_rows(path.c_str(), rows) || rows.size() < 100u) { std::printf("FAILED: cannot read the cases of %s\n", path.c_str()); ++failures; }
  const char* const names[] = {"scene_switches", "material_emissive", "material_lobes", "material_alpha", "shading_classes", "texture_cuts", "texel_span", "footprint_class", "footprint_verdict",
                               "cell_corners", "micromap_words", "plan_scene"};
  for (const char* name : names) {  // (a table without rows for a function would pass for nothing)
    size_t n = 0;
    for (const Row& r : rows) n += r.fn == name ? 1u : 0u;
    if (!n) { std::printf("FAILED: no case of %s\n", name); ++failures; }
  }
  for (size_t i = 0; i < rows.size(); ++i)
    if (!replay(rows[i])) { std::printf("FAILED case %zu (%s)\n", i, rows[i].fn.c_str()); ++failures; }
  if (failures) std::printf("scene_plan_check: %d failures\n", failures);
  else std::printf("scene_plan_check: ok (%zu cases)\n", rows.size());
  return failures ? 1 : 0;
}
