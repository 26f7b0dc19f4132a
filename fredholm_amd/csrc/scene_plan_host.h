// scene_plan_host.h -- everything fh_scene_upload (scene.hip) decides on the host, as pure functions of the caller's fh_scene_desc and of plain values: the switches
// of an upload, the derived words and the shading class of every material, which textures can cut, the opacity class of a face and of a micromap cell from the
// texels it can address, the per-face pass with its validation, and the any-hit records with their micromaps.  plan_scene puts them together into one ScenePlan,
// made before the context is touched: a refused scene changes nothing.  Plain C++ without HIP like bvh_plan_host.h, so that it also compiles into a stand-alone
// program (tools/scene_plan_check.cpp) for the tests and the host sanitizers.  Every expression keeps the integer widths, the order and the floating-point type it
// had inside capi.hip's rebuild_device_scene and upload_textures: tests/golden/scene_plan_cases.json holds what those lines gave.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/fh_texture_unit.h"
#include "../../include/fredholm_hip.h"

namespace fh {

// the lobes of the layered BSDF (fh_bsdf.h), in the reference's order; a material's mask names the lobes it can ever enable
enum : uint32_t { L_COAT = 1, L_METAL = 2, L_SPEC = 4, L_TRANS = 8, L_SHEEN = 16, L_DT = 32, L_DIFF = 64, L_ALL = 127 };

// The layouts the plan fills, as the device reads them (scene.hip asserts that they match uint2, uint4, MaterialDev and AreaLightDev of fh_device.h).
struct Word2 { uint32_t x, y; };
struct Word4 { uint32_t x, y, z, w; };
struct MaterialRecord { float w[45]; uint32_t lobes, emissive, alpha, cls; };  // the 180-byte reference record + derived words
struct LightRecord { uint32_t face, material; };
static_assert(sizeof(fh_material) == 180, "fh_material must match the reference Material (shared.h:100-142)");

// The developer switches of an upload, from the values of their environment variables (null: not set).  Read at EVERY upload (scene.hip: read_scene_switches):
// the tests set and clear them between uploads of one process.
struct SceneSwitches {
  bool opacity_classes;  // FH_OPACITY_CLASSES=0: every face whose textures can cut keeps its any-hit test
  bool micromap;         // FH_OPACITY_MICROMAP=0 (or no opacity classes): all micromap cells 0
  bool debug;            // FH_DEBUG_BVH (any value): the [alpha] lines on stderr
};
inline SceneSwitches scene_switches(const char* classes, const char* micromap, const char* debug)
{
  SceneSwitches sw;
  sw.opacity_classes = classes ? classes[0] != '0' : true;
  sw.micromap = sw.opacity_classes && !(micromap && micromap[0] == '0');
  sw.debug = debug != nullptr;
  return sw;
}

// ---- per-material words
inline bool material_emissive(const fh_material& m) { return m.emission_color[0] > 0 || m.emission_color[1] > 0 || m.emission_color[2] > 0 || m.emission_texture_id != -1; }

inline float plan_lum(const float c[3]) { return c[0] * 0.2126729f + c[1] * 0.7151522f + c[2] * 0.0721750f; }  // fh_vec.h: lum, same constants and order

// lobes a material can ever enable (see fh_bsdf.h).  Seen from the FRONT, metalness == 1 zeroes the weight and the layering
// multiplier of every lobe after the metal one.  Seen from BEHIND the reference resets metalness, specular, sheen and diffuse to 0
// (bsdf.cu:56-62), so transmission and diffuse transmission get their full weight back (weights[3], weights[5], bsdf.cu:74-84): those
// two stay whenever their own parameters enable them.  specular / sheen / diffuse are zero on both sides of a full metal and are dropped.
inline uint32_t material_lobes(const fh_material& m)
{
  // A texture on metalness (or the glTF metallic-roughness texture) makes metalness unknowable on the host: the metal lobe AND the lobes
  // a non-metal needs are kept.  Lobes whose OWN switch is a constant zero stay dropped whatever the textures say: transmission, sheen and
  // subsurface have no texture slot (shared.h:100-142), so a glTF material (scene.cpp:487-549 sets none of them) shades with
  // coat? + metal + specular + diffuse instead of the generic seven-lobe kernel.
  const bool metal_unknown = m.metalness_texture_id >= 0 || m.metallic_roughness_texture_id >= 0;
  uint32_t l = 0;
  const float coat = fmaxf(0.0f, fminf(m.coat, 1.0f));
  if (coat > 0.0f || m.coat_texture_id >= 0) l |= L_COAT;
  if (m.metalness > 0.0f || metal_unknown) l |= L_METAL;
  const bool metal_full = m.metalness == 1.0f && !metal_unknown;
  if (m.transmission > 0.0f) l |= L_TRANS;
  if (m.subsurface * m.thin_walled > 0.0f) l |= L_DT;
  if (!metal_full) {
    if (m.specular_color_texture_id >= 0 || m.specular * plan_lum(m.specular_color) > 0.0f) l |= L_SPEC;
    if (m.sheen * plan_lum(m.sheen_color) != 0.0f) l |= L_SHEEN;
    if (m.diffuse > 0.0f) l |= L_DIFF;
  }
  return l;
}

// alpha: 1 = some fetch of the material's textures can fail the any-hit test; 2 = only a non-finite texture coordinate can (the texture unit returns 0 for it)
inline uint32_t material_alpha(const fh_material& m, const uint8_t* tex_alpha_cuts, const uint8_t* tex_red_cuts)
{
  const int32_t bt = m.base_color_texture_id, at = m.alpha_texture_id;
  const bool cuts = (bt >= 0 && tex_alpha_cuts[(size_t)bt]) || (at >= 0 && tex_red_cuts[(size_t)at]);
  return cuts ? 1u : ((bt >= 0 || at >= 0) ? 2u : 0u);
}

// Shading classes: one per distinct lobe mask, in the order the materials bring them; from max_classes masks on, new masks fold into the last class, which
// becomes the generic one.  Fills mats[i].cls from mats[i].lobes; class_lobes has room for max_classes (kMaxClasses of fh_device.h) masks.  Returns the classes used.
inline uint32_t shading_classes(MaterialRecord* mats, uint32_t nm, uint32_t max_classes, uint32_t* class_lobes)
{
  uint32_t n_classes = 0;
  for (uint32_t i = 0; i < nm; ++i) {
    const uint32_t lobes = mats[i].lobes;
    uint32_t c = 0;
    for (; c < n_classes; ++c)
      if (class_lobes[c] == lobes) break;
    if (c == n_classes) {
      if (n_classes < max_classes) class_lobes[n_classes++] = lobes;
      else { c = max_classes - 1; class_lobes[c] = L_ALL; }  // overflow: fold into one generic class
    }
    mats[i].cls = c;
  }
  if (n_classes == max_classes)  // materials folded into the generic class must see the generic mask
    for (uint32_t i = 0; i < nm; ++i)
      if (mats[i].cls == max_classes - 1) class_lobes[max_classes - 1] |= mats[i].lobes;
  return n_classes;
}

// ---- per-texture cut flags.  The any-hit programs discard a hit when the filtered alpha (base-colour texture) or red (alpha texture) is below 0.5 (pt.cu:545-678).
// A filtered value is a convex combination of texel values (weights are multiples of 2^-16 that sum to exactly 1), so a texture whose every texel decodes to
// >= 0.501 can never discard a hit: faces that only reference such textures need no any-hit test at all (most base-colour maps are opaque).
struct TextureCuts { uint8_t alpha, red; };
inline TextureCuts texture_cuts(const fh_texture_desc& d)
{
  const uint8_t* px = d.rgba8;
  const size_t n_px = (size_t)d.width * d.height;
  uint8_t min_a = 255, min_r = 255;
  for (size_t k = 0; k < n_px; ++k) { min_r = px[4 * k] < min_r ? px[4 * k] : min_r; min_a = px[4 * k + 3] < min_a ? px[4 * k + 3] : min_a; }
  const float red = d.srgb ? fht_srgb_to_linear((float)min_r * (1.0f / 255.0f)) : (float)min_r * (1.0f / 255.0f);
  return TextureCuts{(uint8_t)((float)min_a * (1.0f / 255.0f) < 0.501f ? 1 : 0), (uint8_t)(red < 0.501f ? 1 : 0)};
}

// ---- Opacity classes of cut-out faces (round 5).  The any-hit programs (pt.cu:545-678) discard a candidate hit when the filtered alpha of the base-colour texture or the
// filtered red of the alpha texture is below 0.5 at the hit's texture coordinate.  A filtered value is a convex combination of the four texels around the coordinate (weights
// are products of 1.8 fixed-point fractions and sum to exactly 1, include/fh_texture_unit.h), so over the part of a texture a FACE can ever address the outcome is known in
// advance when all of those texels agree: every byte >= 128 (0.50196) -- the test always passes, the face needs no test at all -- or every byte <= 127 (0.49804) -- it never
// passes, the face can never be hit.  The footprint is the rectangle of texels the face's three texture coordinates span, one texel wider on every side for the bilinear taps
// and a sixteenth more for the rounding of the interpolated coordinate, wrapped like the texture unit wraps; faces with a footprint of more than 2^18 texels are left to the
// test.  0 = test as before, 1 = always passes, 2 = never passes.  FH_OPACITY_CLASSES=0 (read at upload): everything 0.
inline void texel_span(float lo, float hi, uint32_t n, int& first, int& count)
{
  // texel columns (rows) a fetch at normalised coordinates in [lo, hi] can read: floor(u * n - 0.5) and its successor, before wrapping
  const double a = (double)lo * n - 0.5, b = (double)hi * n - 0.5;
  const double slack = 0.0625 + 1e-5 * (std::fabs(a) > std::fabs(b) ? std::fabs(a) : std::fabs(b));
  const double f0 = std::floor(a - slack), f1 = std::floor(b + slack) + 1.0;
  if (!(f1 - f0 < (double)n)) { first = 0; count = (int)n; return; }
  first = (int)(((long long)f0 % (long long)n + (long long)n) % (long long)n);
  count = (int)(f1 - f0) + 1;
}
// 1: every texel of the footprint passes the 0.5 threshold, 2: none does, 0: mixed (or not decided).  uv: n_pts texture coordinates whose bounding rectangle is the footprint
inline uint32_t footprint_class(const uint8_t* rgba8, uint32_t w, uint32_t h, uint32_t channel, const float* decode, const float* uv, int n_pts)
{
  if (!rgba8 || w == 0 || h == 0) return 0u;
  float ulo = uv[0], uhi = uv[0], vlo = uv[1], vhi = uv[1];
  for (int k = 1; k < n_pts; ++k) { ulo = std::fmin(ulo, uv[2 * k]); uhi = std::fmax(uhi, uv[2 * k]); vlo = std::fmin(vlo, uv[2 * k + 1]); vhi = std::fmax(vhi, uv[2 * k + 1]); }
  if (!(std::fabs(ulo) < 1e6f) || !(std::fabs(uhi) < 1e6f) || !(std::fabs(vlo) < 1e6f) || !(std::fabs(vhi) < 1e6f)) return 0u;  // (huge or non-finite coordinates: left to the test)
  int x0, nx, y0, ny;
  texel_span(ulo, uhi, w, x0, nx);
  texel_span(vlo, vhi, h, y0, ny);
  if ((long long)nx * ny > (1ll << 18)) return 0u;
  bool all_pass = true, none_pass = true;
  for (int j = 0; j < ny && (all_pass || none_pass); ++j) {
    const size_t row = (size_t)((y0 + j) % (int)h) * w;
    for (int i = 0; i < nx; ++i) {
      const uint8_t b = rgba8[(row + (size_t)((x0 + i) % (int)w)) * 4u + channel];
      const float v = decode ? decode[b] : (float)b * (1.0f / 255.0f);
      if (v >= 0.50196f) none_pass = false;       // (byte 128 of a linear channel)
      else if (v <= 0.49804f) all_pass = false;   // (byte 127)
      else { all_pass = none_pass = false; }      // an sRGB-decoded value between the two: not decided
    }
  }
  return all_pass ? 1u : (none_pass ? 2u : 0u);
}

// a texture as the footprints read it: the caller's texels where the texture can cut at all (null otherwise: nothing is ever decided from it)
struct CutTexture { const uint8_t* rgba8; uint32_t width, height; bool srgb; };
inline void srgb_decode_table(float table[256])
{
  for (int i = 0; i < 256; ++i) table[i] = fht_srgb_to_linear((float)i * (1.0f / 255.0f));
}
// What the any-hit test says over the footprint of n texture coordinates (a face's three, a cell's four).  flags bit 0: it tests the alpha of `base`, bit 1: the
// red of `alpha`; a texture it does not test passes by itself.  1: always passes, 2: never passes, 0: mixed
inline uint32_t footprint_verdict(uint32_t flags, const CutTexture* base, const CutTexture* alpha, const float* srgb_table, const float* uv, int n)
{
  uint32_t cb = 1u, ca = 1u;
  if (flags & 1u) cb = footprint_class(base->rgba8, base->width, base->height, 3u, nullptr, uv, n);
  if (flags & 2u) ca = footprint_class(alpha->rgba8, alpha->width, alpha->height, 0u, alpha->srgb ? srgb_table : nullptr, uv, n);
  return (cb == 1u && ca == 1u) ? 1u : ((cb == 2u || ca == 2u) ? 2u : 0u);
}

// the texture coordinates of a face's three vertices
inline void face_texcoords(const fh_scene_desc& s, uint32_t f, float uv[6])
{
  for (int k = 0; k < 3; ++k) { const size_t v = s.indices[3ull * f + k]; uv[2 * k] = s.texcoords[2 * v]; uv[2 * k + 1] = s.texcoords[2 * v + 1]; }
}

// The OPACITY MICROMAP of a face: the face cut into 16 x 16 cells of its barycentrics (cell = (floor(16 u), floor(16 v)), the v1 / v2 weights of a hit), two bits per
// cell -- 0: test, 1: the test passes everywhere in the cell, 2: nowhere -- decided like the per-face classes from the texels the cell can address (the cell's four
// corners, moved out by 10^-4 for the rounding of the barycentrics and of the cell index).  out: the texture coordinates of the four corners of cell (ci, cj)
inline void cell_corners(int ci, int cj, const float uv[6], float out[8])
{
  const double u0 = uv[0], w0 = uv[1], du1 = (double)uv[2] - u0, dw1 = (double)uv[3] - w0, du2 = (double)uv[4] - u0, dw2 = (double)uv[5] - w0;
  // barycentric range of the cell, widened: the last cell of a row / column also takes weights of 1 (and a hair more), the first a hair below 0
  const double a0 = ci / 16.0 - 1e-4, a1 = (ci == 15 ? 1.0 : (ci + 1) / 16.0) + 1e-4, b0 = cj / 16.0 - 1e-4, b1 = (cj == 15 ? 1.0 : (cj + 1) / 16.0) + 1e-4;
  const double cb[4][2] = {{a0, b0}, {a1, b0}, {a0, b1}, {a1, b1}};
  for (int k = 0; k < 4; ++k) { out[2 * k] = (float)(u0 + cb[k][0] * du1 + cb[k][1] * du2); out[2 * k + 1] = (float)(w0 + cb[k][0] * dw1 + cb[k][1] * dw2); }
}
// the 16 words of a face's micromap; counts: cells decided, of them always pass, never pass (added to)
inline void micromap_words(uint32_t flags, const CutTexture* base, const CutTexture* alpha, const float* srgb_table, const float uv[6], uint32_t words[16], unsigned long long counts[3])
{
  for (int cj = 0; cj < 16; ++cj)
    for (int ci = 0; ci + cj <= 16 && ci < 16; ++ci) {  // (cells beyond the hypotenuse are never addressed: they stay 0)
      float corners[8];
      cell_corners(ci, cj, uv, corners);
      const uint32_t st = footprint_verdict(flags, base, alpha, srgb_table, corners, 4);
      const int cell = cj * 16 + ci;
      words[cell >> 4] |= st << (2 * (cell & 15));
      ++counts[0]; counts[1] += st == 1u; counts[2] += st == 2u;
    }
}

// ---- the plan of one upload
struct ScenePlan {
  const char* error = nullptr;  // why the scene is refused (FH_E_INVALID); everything below is then unfinished
  SceneSwitches sw{};
  uint32_t n_instances = 0;     // transforms the scene brings; a scene without any has one identity
  // textures: the cut flags, and where each texture's texels begin in the one blob of texel_bytes bytes
  std::vector<uint8_t> tex_alpha_cuts, tex_red_cuts;
  std::vector<unsigned long long> tex_offset;
  unsigned long long texel_bytes = 0;
  std::vector<MaterialRecord> materials;
  uint32_t n_classes = 0;
  std::vector<uint32_t> class_lobes;  // the first n_classes of max_classes
  // per face: class | 0x80 emissive | 0x40 keeps its any-hit test | 0x20 can never be hit; (material, instance); bit 0: test the base-colour texture's alpha, bit 1: the alpha texture's red
  std::vector<uint8_t> face_cls;
  std::vector<Word2> face_meta;
  std::vector<uint8_t> alpha_bits;
  std::vector<LightRecord> lights;        // emissive faces in face order (renderer.h:388-402)
  uint32_t alpha_face_counts[4] = {0, 0, 0, 0};  // faces whose textures can cut; of them: always pass, never pass, still tested
  bool any_alpha = false;
  // 8 x 16 bytes per face when any face keeps its test, else empty.  Words 0-5 of a face: its texture coordinates, 6: flags (alpha_bits | 4: the alpha texture is sRGB);
  // vectors 2 and 3: the base-colour / alpha texture (BYTE OFFSET of its texels in the blob -- the upload adds the blob's address --, width, height); 4-7: the micromap
  std::vector<Word4> alpha_rec;
  unsigned long long alpha_cell_counts[3] = {0, 0, 0};  // micromap cells of the faces that keep their test; of them: always pass, never pass
};

// The refusals of fh_scene_upload that need no look at the faces, in their order; null: none
inline const char* scene_arguments_error(const fh_scene_desc* s)
{
  if (!s || !s->vertices || !s->normals || !s->texcoords || !s->indices || !s->material_ids || !s->materials || s->n_materials == 0) return "fh_scene_upload: missing arrays";
  for (uint32_t i = 0; i < s->n_materials; ++i) {
    const fh_material& m = s->materials[i];
    const int32_t ids[11] = {m.base_color_texture_id, m.specular_color_texture_id, m.specular_roughness_texture_id, m.metalness_texture_id, m.metallic_roughness_texture_id, m.coat_texture_id,
                             m.coat_roughness_texture_id, m.emission_texture_id, m.heightmap_texture_id, m.normalmap_texture_id, m.alpha_texture_id};
    for (int32_t id : ids)
      if (id < -1 || id >= (int32_t)s->n_textures) return "fh_scene_upload: material references a texture id outside [0, n_textures)";
  }
  if (s->n_textures && !s->textures) return "fh_scene_upload: n_textures > 0 but textures == NULL";
  for (uint32_t i = 0; i < s->n_textures; ++i)
    if (!s->textures[i].rgba8 || s->textures[i].width == 0 || s->textures[i].height == 0) return "fh_scene_upload: empty texture";
  return nullptr;
}

inline void plan_textures(const fh_scene_desc& s, ScenePlan& p)
{
  p.tex_alpha_cuts.assign(s.n_textures, 0);
  p.tex_red_cuts.assign(s.n_textures, 0);
  p.tex_offset.assign(s.n_textures, 0);
  p.texel_bytes = 0;
  for (uint32_t i = 0; i < s.n_textures; ++i) {
    const TextureCuts c = texture_cuts(s.textures[i]);
    p.tex_alpha_cuts[i] = c.alpha;
    p.tex_red_cuts[i] = c.red;
    p.tex_offset[i] = p.texel_bytes;
    p.texel_bytes += (size_t)s.textures[i].width * s.textures[i].height * 4;
  }
}

inline void plan_materials(const fh_scene_desc& s, uint32_t max_classes, ScenePlan& p)
{
  p.materials.resize(s.n_materials);
  for (uint32_t i = 0; i < s.n_materials; ++i) {
    std::memcpy(p.materials[i].w, &s.materials[i], 180);
    p.materials[i].lobes = material_lobes(s.materials[i]);
    p.materials[i].emissive = material_emissive(s.materials[i]) ? 1u : 0u;
    p.materials[i].alpha = material_alpha(s.materials[i], p.tex_alpha_cuts.data(), p.tex_red_cuts.data());
  }
  p.class_lobes.assign(max_classes, 0u);
  p.n_classes = shading_classes(p.materials.data(), s.n_materials, max_classes, p.class_lobes.data());
}

// Per face, in face order: the validation (instance id, then material id, then the three vertex indices), the class byte, the light list and which textures the
// any-hit test of the face has to look at.  Cheap integer work, except for the footprints of the faces whose textures can cut.  Returns the refusal, or null.
inline const char* plan_faces(const fh_scene_desc& s, const CutTexture* tex, const float* srgb_table, ScenePlan& p)
{
  const uint32_t nf = s.n_faces, nv = s.n_vertices, nm = s.n_materials, ni = p.n_instances;
  const std::vector<MaterialRecord>& mats = p.materials;
  p.face_cls.assign(nf, 0);
  p.face_meta.assign(nf, Word2{0u, 0u});
  p.alpha_bits.assign(nf, 0);
  for (uint32_t f = 0; f < nf; ++f) {
    const uint32_t inst = s.instance_ids ? s.instance_ids[f] : 0u;
    if (inst >= ni) return "instance id out of range";
    const uint32_t mid = s.material_ids[f];
    if (mid >= nm) return "material id out of range";
    for (int k = 0; k < 3; ++k)
      if (s.indices[3ull * f + k] >= nv) return "vertex index out of range";
    p.face_meta[f] = Word2{mid, inst};
    bool alpha = mats[mid].alpha == 1u, never = false;
    if (mats[mid].alpha) {
      float uv[6];
      face_texcoords(s, f, uv);
      bool wild = false;  // opaque textures: the test can only fail where the interpolated coordinate is NaN or overflows
      for (int k = 0; k < 6; ++k)
        if (!(std::fabs(uv[k]) < 1e30f)) wild = true;
      alpha = alpha || wild;
      const int32_t bt = s.materials[mid].base_color_texture_id, at = s.materials[mid].alpha_texture_id;
      p.alpha_bits[f] = (uint8_t)(((bt >= 0 && (wild || p.tex_alpha_cuts[(size_t)bt])) ? 1u : 0u) | ((at >= 0 && (wild || p.tex_red_cuts[(size_t)at])) ? 2u : 0u));
      if (alpha) p.alpha_face_counts[0]++;
      if (alpha && !wild && p.sw.opacity_classes) {  // what the face's own footprint says (above)
        const uint32_t verdict = footprint_verdict(p.alpha_bits[f], bt >= 0 ? &tex[bt] : nullptr, at >= 0 ? &tex[at] : nullptr, srgb_table, uv, 3);
        if (verdict == 1u) { alpha = false; p.alpha_bits[f] = 0; p.alpha_face_counts[1]++; }                     // always passes: an ordinary opaque face
        else if (verdict == 2u) { never = true; alpha = false; p.alpha_bits[f] = 0; p.alpha_face_counts[2]++; }  // never passes: no ray can hit it
      }
    }
    p.face_cls[f] = (uint8_t)(mats[mid].cls | (mats[mid].emissive ? 0x80u : 0u) | (alpha ? 0x40u : 0u) | (never ? 0x20u : 0u));
    if (alpha) p.any_alpha = true;
    if (mats[mid].emissive) p.lights.push_back({f, mid});  // renderer.h:388-402, face order
  }
  p.alpha_face_counts[3] = p.alpha_face_counts[0] - p.alpha_face_counts[1] - p.alpha_face_counts[2];
  return nullptr;
}

// Everything the any-hit test of a face reads, in one 64-byte line: the three texture coordinates and the two textures it may have to look at; and, behind them
// (second 64-byte line), the face's opacity micromap (above).  alpha_pass (fh_trace.h) looks the cell of a candidate up before anything else (one dword).
// Exact: same hits, same images.
inline void plan_alpha_records(const fh_scene_desc& s, const CutTexture* tex, const float* srgb_table, ScenePlan& p)
{
  if (!p.any_alpha) return;
  const uint32_t nf = s.n_faces;
  p.alpha_rec.assign(8ull * nf, Word4{0u, 0u, 0u, 0u});
  auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
  for (uint32_t f = 0; f < nf; ++f) {
    if (!p.alpha_bits[f]) continue;
    const fh_material& m = s.materials[s.material_ids[f]];
    float uv[6];
    face_texcoords(s, f, uv);
    Word4* rec = &p.alpha_rec[8ull * f];
    rec[0] = Word4{bits(uv[0]), bits(uv[1]), bits(uv[2]), bits(uv[3])};
    uint32_t flags = p.alpha_bits[f];
    if ((flags & 2u) && s.textures[m.alpha_texture_id].srgb) flags |= 4u;
    rec[1] = Word4{bits(uv[4]), bits(uv[5]), flags, 0u};
    if (flags & 1u) {
      const unsigned long long off = p.tex_offset[(size_t)m.base_color_texture_id];
      rec[2] = Word4{(uint32_t)off, (uint32_t)(off >> 32), tex[m.base_color_texture_id].width, tex[m.base_color_texture_id].height};
    }
    if (flags & 2u) {
      const unsigned long long off = p.tex_offset[(size_t)m.alpha_texture_id];
      rec[3] = Word4{(uint32_t)off, (uint32_t)(off >> 32), tex[m.alpha_texture_id].width, tex[m.alpha_texture_id].height};
    }
    bool finite_uv = true;
    for (int k = 0; k < 6; ++k) finite_uv = finite_uv && std::fabs(uv[k]) < 1e6f;
    if (p.sw.micromap && finite_uv) {
      uint32_t words[16] = {};
      micromap_words(flags, (flags & 1u) ? &tex[m.base_color_texture_id] : nullptr, (flags & 2u) ? &tex[m.alpha_texture_id] : nullptr, srgb_table, uv, words, p.alpha_cell_counts);
      for (int k = 0; k < 4; ++k) rec[4 + k] = Word4{words[4 * k], words[4 * k + 1], words[4 * k + 2], words[4 * k + 3]};
    }
  }
}

// The whole plan of an upload, from the caller's descriptor alone (it reads the caller's texels where they are).  max_classes: kMaxClasses of fh_device.h
inline ScenePlan plan_scene(const fh_scene_desc* s, const SceneSwitches& sw, uint32_t max_classes)
{
  ScenePlan p;
  p.sw = sw;
  if ((p.error = scene_arguments_error(s))) return p;
  p.n_instances = (s->n_instances && s->object_to_world && s->world_to_object) ? s->n_instances : 1u;
  plan_textures(*s, p);
  plan_materials(*s, max_classes, p);
  std::vector<CutTexture> tex(s->n_textures);
  for (uint32_t i = 0; i < s->n_textures; ++i) {
    const fh_texture_desc& d = s->textures[i];
    tex[i] = CutTexture{(p.tex_alpha_cuts[i] || p.tex_red_cuts[i]) ? d.rgba8 : nullptr, d.width, d.height, d.srgb != 0};
  }
  float srgb_table[256];
  srgb_decode_table(srgb_table);
  if ((p.error = plan_faces(*s, tex.data(), srgb_table, p))) return p;
  plan_alpha_records(*s, tex.data(), srgb_table, p);
  return p;
}

}  // namespace fh
