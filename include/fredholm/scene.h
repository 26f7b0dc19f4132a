// fredholm/scene.h -- flat scene container with the public members of the reference's fredholm::Scene
// (fredholm/include/fredholm/scene.h:103-135) and a from-scratch Wavefront .obj/.mtl reader that fills them
// the way the reference's tinyobjloader path does (fredholm/src/scene.cpp:119-443): triangulated faces,
// face normals / barycentric texcoords when absent (:361-377), Kd -> base_color, Ks -> specular_color,
// Pr/Pm/Pc, d -> transmission = 1 - d (:245), Tf, Ke, and the custom keys diffuse, diffuse_roughness, sheen*,
// subsurface*, thin_walled (:183-284); coat_roughness takes clearcoat_thickness as in the reference (:240-242).
// Texture statements (map_Kd, map_Ks, map_Pr, map_Pm, map_bump/bump, norm, map_d) load PNG / binary PPM files through
// image_io.h with the reference's conventions (scene.cpp:7-37,144-153: vertical flip, one Texture per distinct file name, its
// first use fixes COLOR / NONCOLOR).  glTF (.gltf, JSON + external or data-URI buffers) goes through json.h and follows
// scene.cpp:445-860 including its quirks (listed in fredholm_amd/scene.py, the Python twin of this file); scene-graph math is
// done in double and rounded to float once, identically in both front ends.  Beyond the reference: a file with a non-empty
// `skins` array also yields m_joints / m_weights, m_skins and joint_matrices_3x4(), and one Animation per animated node, which may
// then be a joint below a root; a file without `skins` loads exactly as before.  Not supported in this build: JPEG files, .glb.
#pragma once
#include <cmath>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <functional>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <algorithm>
#include <array>
#include <memory>

#include "camera.h"
#include "image_io.h"
#include "json.h"
#include "shared.h"

namespace fredholm
{

// fredholm/include/fredholm/scene.h:60-79
enum class TextureType { COLOR, NONCOLOR };

struct Texture {
  uint32_t m_width = 0;
  uint32_t m_height = 0;
  std::vector<uchar4> m_data;
  TextureType m_texture_type = TextureType::NONCOLOR;

  Texture() {}
  Texture(const std::filesystem::path& filepath, const TextureType& texture_type) : m_texture_type(texture_type)
  {
    const image_io::Image8 img = image_io::load_rgba8(filepath, /*flip_vertically=*/true);  // scene.cpp:15-16
    m_width = uint32_t(img.width);
    m_height = uint32_t(img.height);
    m_data.resize(size_t(m_width) * m_height);
    for (size_t i = 0; i < m_data.size(); ++i) m_data[i] = uchar4{img.rgba[4 * i], img.rgba[4 * i + 1], img.rgba[4 * i + 2], img.rgba[4 * i + 3]};
  }
};

struct FloatTexture {
  uint32_t m_width = 0;
  uint32_t m_height = 0;
  std::vector<float4> m_data;

  explicit FloatTexture(const std::filesystem::path& filepath)
  {
    const image_io::ImageF img = image_io::load_hdr(filepath);  // scene.cpp:44-45: no flip
    m_width = uint32_t(img.width);
    m_height = uint32_t(img.height);
    m_data.resize(size_t(m_width) * m_height);
    for (size_t i = 0; i < m_data.size(); ++i) m_data[i] = float4{img.rgba[4 * i], img.rgba[4 * i + 1], img.rgba[4 * i + 2], img.rgba[4 * i + 3]};
  }
};

// scene-graph math in double, row-major m[row][col]
struct Mat4d {
  double m[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  static Mat4d mul(const Mat4d& a, const Mat4d& b)
  {
    Mat4d r;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j] + a.m[i][3] * b.m[3][j];
    return r;
  }
  // glm: translate(I, t) * mat4_cast(q) * scale(s), q = (w, x, y, z)
  static Mat4d trs(const double t[3], const double q[4], const double s[3])
  {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double r[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                            {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                            {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
    Mat4d m;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) m.m[i][j] = r[i][j] * s[j];
      m.m[i][3] = t[i];
    }
    return m;
  }
  // inverse of [A t; 0 1] by cofactors (same expression order as fredholm_amd/scene.py: affine_inverse)
  Mat4d affine_inverse() const
  {
    const double a = m[0][0], b = m[0][1], c = m[0][2], d = m[1][0], e = m[1][1], f = m[1][2], g = m[2][0], h = m[2][1], i = m[2][2];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    const double inv = 1.0 / det;
    const double r[3][3] = {{(e * i - f * h) * inv, (c * h - b * i) * inv, (b * f - c * e) * inv},
                            {(f * g - d * i) * inv, (a * i - c * g) * inv, (c * d - a * f) * inv},
                            {(d * h - e * g) * inv, (b * g - a * h) * inv, (a * e - b * d) * inv}};
    Mat4d out;
    for (int k = 0; k < 3; ++k) {
      for (int j = 0; j < 3; ++j) out.m[k][j] = r[k][j];
      out.m[k][3] = -(r[k][0] * m[0][3] + r[k][1] * m[1][3] + r[k][2] * m[2][3]);
    }
    return out;
  }
  Mat4 to_float() const  // column-major like glm::mat4
  {
    Mat4 r;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) r[j][i] = float(m[i][j]);
    return r;
  }
  static Mat4d from_float(const Mat4& f)
  {
    Mat4d r;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) r.m[i][j] = double(f[j][i]);
    return r;
  }
};

// scene.h:81-101
struct Node {
  int idx = -1;  // glTF node index
  std::vector<Node> children;
  Mat4d transform;
  int camera_id = -1;
  int submesh_id = -1;
  Mat4d global;  // parent chain times transform, kept by update_transform (the joints of a skin need it)
};

// where a node is: its root's index in Scene::m_nodes, then the child index at every level below
using NodePath = std::vector<int>;

struct Skin {
  std::vector<NodePath> joints;
  std::vector<Mat4d> inverse_bind;  // per joint
  uint32_t base = 0;                // index of the skin's first joint in the scene's palette
  NodePath mesh_node;               // the first node that uses the skin (empty: none): the joint matrices are in its object space
};

struct Animation {
  std::vector<float> translation_input, rotation_input, scale_input;
  std::vector<std::array<double, 3>> translation_output, scale_output;
  std::vector<std::array<double, 4>> rotation_output;  // (w, x, y, z)
};

struct Scene {
  bool m_has_camera_transform = false;
  Mat4 m_camera_transform = {};
  std::vector<float3> m_vertices = {};
  std::vector<uint3> m_indices = {};
  std::vector<float2> m_texcoords = {};
  std::vector<float3> m_normals = {};
  std::vector<uint> m_material_ids = {};
  std::vector<Material> m_materials;
  std::vector<Texture> m_textures;
  std::vector<uint> m_submesh_offsets = {};
  std::vector<uint> m_submesh_n_faces = {};
  std::vector<uint> m_instance_ids = {};
  std::vector<Mat4> m_transforms = {};
  std::vector<Mat4d> m_transforms_exact = {};  // the same matrices before rounding to float (scene-graph products are done in double)
  std::vector<Node> m_nodes = {};
  std::vector<Animation> m_animations = {};
  std::vector<std::array<uint16_t, 4>> m_joints = {};  // per vertex: indices into the palette of all skins (palette base of the skin + local index)
  std::vector<std::array<float, 4>> m_weights = {};    // per vertex; zero for the vertices of unskinned meshes
  std::vector<Skin> m_skins = {};

  bool is_valid() const { return !m_vertices.empty() && !m_indices.empty() && !m_normals.empty() && m_vertices.size() == m_normals.size(); }

  void clear()
  {
    m_vertices.clear(); m_indices.clear(); m_texcoords.clear(); m_normals.clear(); m_material_ids.clear(); m_materials.clear(); m_textures.clear();
    m_submesh_offsets.clear(); m_submesh_n_faces.clear(); m_instance_ids.clear(); m_transforms.clear(); m_transforms_exact.clear();
    m_nodes.clear(); m_animations.clear(); m_animation_targets.clear(); m_animation_paths.clear();
    m_joints.clear(); m_weights.clear(); m_skins.clear();
    m_has_camera_transform = false;
    m_camera_transform = Mat4{};
  }

  void load_model(const std::filesystem::path& filepath, bool do_clear)
  {
    if (do_clear) clear();
    const std::string ext = filepath.extension().string();
    if (ext == ".obj") load_obj(filepath);
    else if (ext == ".gltf") load_gltf(filepath);
    else throw std::runtime_error("unsupported model format in this build: " + filepath.generic_string());
  }


  void load_obj(const std::filesystem::path& filepath)
  {
    std::ifstream in(filepath);
    if (!in) throw std::runtime_error("failed to load " + filepath.generic_string());
    std::vector<float3> pos, nrm;
    std::vector<float2> tex;
    std::map<std::string, int> mat_index, unique_textures;
    const size_t material_base = m_materials.size();
    int current_material = -1;
    bool need_default = false;
    const size_t first_face = m_indices.size();
    std::string line;
    auto resolve = [](int idx, size_t n) { return idx > 0 ? idx - 1 : int(n) + idx; };
    while (std::getline(in, line)) {
      std::istringstream ss(line);
      std::string tag;
      if (!(ss >> tag) || tag[0] == '#') continue;
      if (tag == "v") { float3 p; ss >> p.x >> p.y >> p.z; pos.push_back(p); }
      else if (tag == "vn") { float3 n; ss >> n.x >> n.y >> n.z; nrm.push_back(n); }
      else if (tag == "vt") { float2 t{0, 0}; ss >> t.x >> t.y; tex.push_back(t); }
      else if (tag == "mtllib") { std::string name; ss >> name; load_mtl(filepath.parent_path() / name, mat_index, unique_textures); }
      else if (tag == "usemtl") { std::string name; ss >> name; current_material = mat_index.count(name) ? mat_index[name] : -1; }
      else if (tag == "f") {
        struct Corner { int v, t, n; };
        std::vector<Corner> cs;
        std::string tok;
        while (ss >> tok) {
          Corner c{0, 0, 0};
          std::string part[3];
          int k = 0;
          for (char ch : tok) { if (ch == '/') { if (++k > 2) break; } else part[k] += ch; }
          c.v = part[0].empty() ? 0 : std::stoi(part[0]);
          c.t = part[1].empty() ? 0 : std::stoi(part[1]);
          c.n = part[2].empty() ? 0 : std::stoi(part[2]);
          cs.push_back(c);
        }
        for (size_t k = 1; k + 1 < cs.size(); ++k) {  // fan triangulation
          const Corner tri[3] = {cs[0], cs[k], cs[k + 1]};
          float3 p[3];
          for (int c = 0; c < 3; ++c) p[c] = pos.at(resolve(tri[c].v, pos.size()));
          const bool has_n = tri[0].n && tri[1].n && tri[2].n, has_t = tri[0].t && tri[1].t && tri[2].t;
          float3 fn{0, 0, 0};
          if (!has_n) {  // scene.cpp:361-371: normalize(cross(normalize(e1), normalize(e2)))
            const float3 e1 = norm3(sub3(p[1], p[0])), e2 = norm3(sub3(p[2], p[0]));
            fn = norm3(make_float3(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x));
          }
          const float2 bary[3] = {{0, 0}, {1, 0}, {0, 1}};
          const uint base = uint(m_vertices.size());
          for (int c = 0; c < 3; ++c) {
            m_vertices.push_back(p[c]);
            m_normals.push_back(has_n ? nrm.at(resolve(tri[c].n, nrm.size())) : fn);
            m_texcoords.push_back(has_t ? tex.at(resolve(tri[c].t, tex.size())) : bary[c]);
          }
          m_indices.push_back(make_uint3(base, base + 1, base + 2));
          if (current_material < 0) need_default = true;
          m_material_ids.push_back(current_material < 0 ? 0xffffffffu : uint(current_material));
          m_instance_ids.push_back(0);
        }
      }
    }
    if (need_default) {  // faces without usemtl: the reference indexes materials[-1]; give them a default material instead
      const uint id = uint(m_materials.size());
      m_materials.push_back(Material{});
      for (size_t f = first_face; f < m_material_ids.size(); ++f)
        if (m_material_ids[f] == 0xffffffffu) m_material_ids[f] = id;
    }
    (void)material_base;
    m_submesh_offsets.push_back(uint(first_face));
    m_submesh_n_faces.push_back(uint(m_indices.size() - first_face));
    m_transforms.push_back(Mat4{});  // scene.cpp:419-421: one identity per shape; every .obj face uses instance 0 (:424-428)
    m_transforms_exact.push_back(Mat4d{});
    m_joints.resize(m_vertices.size(), std::array<uint16_t, 4>{0, 0, 0, 0});
    m_weights.resize(m_vertices.size(), std::array<float, 4>{0, 0, 0, 0});
  }


  // ------------------------------------------------------------------------------------------ glTF (scene.cpp:445-860)
  void load_gltf(const std::filesystem::path& filepath)
  {
    const std::vector<uint8_t> text = image_io::read_file(filepath);
    const json::Value model = json::parse(std::string(text.begin(), text.end()));
    const std::filesystem::path folder = filepath.parent_path();
    std::vector<std::vector<uint8_t>> buffers;
    if (model.has("buffers"))
      for (const json::Value& b : model.at("buffers").arr) {
        const std::string uri = b.has("uri") ? b.at("uri").string() : std::string();
        if (uri.rfind("data:", 0) == 0) buffers.push_back(base64_decode(uri.substr(uri.find(',') + 1)));
        else buffers.push_back(image_io::read_file(folder / uri));
      }
    struct View { const uint8_t* data; size_t avail; int stride, count; };
    auto get_buffer = [&](int accessor_id) {  // scene.cpp:921-933
      const json::Value& acc = model.at("accessors").at(size_t(accessor_id));
      if (!acc.has("bufferView")) throw std::runtime_error("accessor without bufferView");
      const json::Value& view = model.at("bufferViews").at(size_t(acc.at("bufferView").integer()));
      const int comp = component_size(acc.at("componentType").integer()) * type_count(acc.at("type").string());
      const int bs = view.integer_or("byteStride", 0);
      const std::vector<uint8_t>& buf = buffers.at(size_t(view.at("buffer").integer()));
      const size_t start = size_t(view.integer_or("byteOffset", 0)) + size_t(acc.integer_or("byteOffset", 0));
      if (start > buf.size()) throw std::runtime_error("accessor outside its buffer");
      return View{buf.data() + start, buf.size() - start, bs ? bs : comp, acc.at("count").integer()};
    };
    auto need = [](const View& v, size_t bytes) { if (bytes > v.avail) throw std::runtime_error("accessor outside its buffer"); };

    const uint material_base = uint(m_materials.size());
    const int texture_base = int(m_textures.size());
    if (model.has("materials"))
      for (const json::Value& material : model.at("materials").arr) {
        Material mat;
        const json::Value empty;
        const json::Value& pmr = material.has("pbrMetallicRoughness") ? material.at("pbrMetallicRoughness") : empty;
        if (pmr.has("baseColorFactor")) mat.base_color = make_float3(float(pmr.at("baseColorFactor").at(0).number()), float(pmr.at("baseColorFactor").at(1).number()), float(pmr.at("baseColorFactor").at(2).number()));
        else mat.base_color = make_float3(1, 1, 1);
        if (pmr.has("baseColorTexture")) mat.base_color_texture_id = pmr.at("baseColorTexture").at("index").integer() + texture_base;
        mat.specular_roughness = float(pmr.number_or("roughnessFactor", 1.0));
        mat.metalness = float(pmr.number_or("metallicFactor", 1.0));
        if (pmr.has("metallicRoughnessTexture")) mat.metallic_roughness_texture_id = pmr.at("metallicRoughnessTexture").at("index").integer() + texture_base;
        if (material.has("extensions") && material.at("extensions").has("KHR_materials_clearcoat")) {
          const json::Value& cc = material.at("extensions").at("KHR_materials_clearcoat");
          if (cc.has("clearcoatFactor")) mat.coat = float(cc.at("clearcoatFactor").number());
          if (cc.has("clearcoatTexture")) mat.coat_texture_id = 0;  // scene.cpp:521-523: GetNumberAsInt() of an object
          if (cc.has("clearcoatRoughnessFactor")) mat.coat_roughness = float(cc.at("clearcoatRoughnessFactor").number());
          if (cc.has("clearcoatRoughnessTexture")) mat.coat_roughness_texture_id = 0;
        }
        mat.emission = 1.0f;  // scene.cpp:535-541
        mat.emission_color = make_float3(0, 0, 0);
        if (material.has("emissiveFactor")) mat.emission_color = make_float3(float(material.at("emissiveFactor").at(0).number()), float(material.at("emissiveFactor").at(1).number()), float(material.at("emissiveFactor").at(2).number()));
        if (material.has("emissiveTexture")) mat.emission_texture_id = material.at("emissiveTexture").at("index").integer() + texture_base;
        if (material.has("normalTexture")) mat.normalmap_texture_id = material.at("normalTexture").at("index").integer() + texture_base;
        m_materials.push_back(mat);
      }
    if (model.has("textures"))
      for (const json::Value& texture : model.at("textures").arr) {
        const json::Value& image = model.at("images").at(size_t(texture.at("source").integer()));
        m_textures.push_back(Texture(folder / image.at("uri").string(), TextureType::NONCOLOR));  // scene.cpp:560-567
      }

    // skins: the palette bases first, so that the vertices of a skinned mesh can name their joints in the palette of all skins
    const json::Value no_skins;
    const std::vector<json::Value>& gskins = model.has("skins") ? model.at("skins").arr : no_skins.arr;
    std::vector<uint32_t> skin_base, skin_count;
    {
      uint32_t next = 0;
      for (const Skin& sk : m_skins) next += uint32_t(sk.joints.size());
      for (const json::Value& gs : gskins) { skin_base.push_back(next); skin_count.push_back(uint32_t(gs.at("joints").arr.size())); next += skin_count.back(); }
    }
    std::map<int, NodePath> by_idx;     // glTF node index -> where the node is, for the nodes reachable from the scene's roots
    std::map<int, NodePath> skin_user;  // skin index -> the first node that uses it
    auto read_skin_attributes = [&](const json::Value& prim, int skin_id, int n_pos) {
      const json::Value& attrs = prim.at("attributes");
      if (attrs.has("JOINTS_0") != attrs.has("WEIGHTS_0")) throw std::runtime_error("JOINTS_0 and WEIGHTS_0 must come together");
      if (!attrs.has("JOINTS_0")) throw std::runtime_error("a primitive of a skinned node has no JOINTS_0 / WEIGHTS_0");
      if (model.at("accessors").at(size_t(attrs.at("WEIGHTS_0").integer())).at("componentType").integer() != 5126) throw std::runtime_error("normalised-integer WEIGHTS_0 is not supported");
      const View wv = get_buffer(attrs.at("WEIGHTS_0").integer());
      if (wv.stride != 16) throw std::runtime_error("weights stride is not float4");
      const int jtype = model.at("accessors").at(size_t(attrs.at("JOINTS_0").integer())).at("componentType").integer();
      if (jtype != 5121 && jtype != 5123) throw std::runtime_error("JOINTS_0 is neither unsigned byte nor unsigned short");
      const int jsize = jtype == 5121 ? 1 : 2;
      const View jv = get_buffer(attrs.at("JOINTS_0").integer());
      if (jv.stride != 4 * jsize) throw std::runtime_error("joints are not tightly packed");
      if (wv.count != n_pos || jv.count != n_pos) throw std::runtime_error("JOINTS_0 / WEIGHTS_0 count is not the vertex count");
      need(wv, size_t(wv.count) * 16); need(jv, size_t(jv.count) * 4 * size_t(jsize));
      for (int i = 0; i < 4 * jv.count; ++i) {
        uint16_t j = jv.data[size_t(jsize) * i];
        if (jsize == 2) std::memcpy(&j, jv.data + 2 * size_t(i), 2);
        if (j >= skin_count[size_t(skin_id)]) throw std::runtime_error("joint index outside the skin's joints");
      }
      for (int i = 0; i < n_pos; ++i) {
        std::array<uint16_t, 4> j;
        std::array<float, 4> w;
        for (int k = 0; k < 4; ++k) {
          uint16_t local = jv.data[size_t(jsize) * (4 * i + k)];
          if (jsize == 2) std::memcpy(&local, jv.data + 2 * size_t(4 * i + k), 2);
          j[size_t(k)] = uint16_t(local + skin_base[size_t(skin_id)]);
          std::memcpy(&w[size_t(k)], wv.data + 16 * size_t(i) + 4 * size_t(k), 4);
        }
        m_joints.push_back(j);
        m_weights.push_back(w);
      }
    };

    std::function<Node(int, const NodePath&)> load_node = [&](int node_idx, const NodePath& path) {
      const json::Value& node = model.at("nodes").at(size_t(node_idx));
      Node n;
      n.idx = node_idx;
      by_idx[node_idx] = path;
      double t[3] = {0, 0, 0}, q[4] = {1, 0, 0, 0}, sc[3] = {1, 1, 1};
      if (node.has("translation")) for (int k = 0; k < 3; ++k) t[k] = double(float(node.at("translation").at(size_t(k)).number()));
      if (node.has("rotation")) {
        const json::Value& r = node.at("rotation");
        q[0] = double(float(r.at(3).number())); q[1] = double(float(r.at(0).number())); q[2] = double(float(r.at(1).number())); q[3] = double(float(r.at(2).number()));
      }
      if (node.has("scale")) for (int k = 0; k < 3; ++k) sc[k] = double(float(node.at("scale").at(size_t(k)).number()));
      n.transform = Mat4d::trs(t, q, sc);
      if (node.has("matrix"))  // column-major in the file
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) n.transform.m[r][c] = double(float(node.at("matrix").at(size_t(4 * c + r)).number()));
      n.camera_id = node.integer_or("camera", -1);
      if (node.has("mesh")) {
        const json::Value& mesh = model.at("meshes").at(size_t(node.at("mesh").integer()));
        n.submesh_id = int(m_submesh_offsets.size());
        const size_t prev = m_indices.size();
        const int skin_id = gskins.empty() ? -1 : node.integer_or("skin", -1);
        if (skin_id >= 0 && !skin_user.count(skin_id)) skin_user[skin_id] = path;
        for (const json::Value& prim : mesh.at("primitives").arr) {
          const uint base = uint(m_vertices.size());
          m_joints.resize(base, std::array<uint16_t, 4>{0, 0, 0, 0});
          m_weights.resize(base, std::array<float, 4>{0, 0, 0, 0});
          const View iv = get_buffer(prim.at("indices").integer());
          if (iv.stride != 2) throw std::runtime_error("indices stride is not ushort");
          need(iv, size_t(iv.count) * 2);
          const json::Value& attrs = prim.at("attributes");
          const View pv = get_buffer(attrs.at("POSITION").integer());
          if (pv.stride != 12) throw std::runtime_error("positions stride is not float3");
          const View nv = get_buffer(attrs.at("NORMAL").integer());
          if (nv.stride != 12) throw std::runtime_error("normals stride is not float3");
          const View tv = get_buffer(attrs.at("TEXCOORD_0").integer());
          if (tv.stride != 8) throw std::runtime_error("texcoord stride is not float2");
          need(pv, size_t(pv.count) * 12); need(nv, size_t(nv.count) * 12); need(tv, size_t(tv.count) * 8);
          auto f32 = [](const uint8_t* p) { float v; std::memcpy(&v, p, 4); return v; };
          for (int i = 0; i < pv.count; ++i) m_vertices.push_back(make_float3(f32(pv.data + 12 * i), f32(pv.data + 12 * i + 4), f32(pv.data + 12 * i + 8)));
          for (int i = 0; i < nv.count; ++i) m_normals.push_back(make_float3(f32(nv.data + 12 * i), f32(nv.data + 12 * i + 4), f32(nv.data + 12 * i + 8)));
          for (int i = 0; i < tv.count; ++i) m_texcoords.push_back(float2{f32(tv.data + 8 * i), 1.0f - f32(tv.data + 8 * i + 4)});
          if (skin_id >= 0) read_skin_attributes(prim, skin_id, pv.count);
          const int material = prim.integer_or("material", -1);
          for (int i = 0; i < iv.count / 3; ++i) {
            uint16_t k[3];
            std::memcpy(k, iv.data + 6 * i, 6);
            m_indices.push_back(make_uint3(k[0] + base, k[1] + base, k[2] + base));
            m_material_ids.push_back(material >= 0 ? uint(material) + material_base : 0xffffffffu);
            m_instance_ids.push_back(uint(m_submesh_offsets.size()));
          }
        }
        m_submesh_offsets.push_back(uint(prev));
        m_submesh_n_faces.push_back(uint(m_indices.size() - prev));
      }
      if (node.has("children"))
        for (const json::Value& c : node.at("children").arr) {
          NodePath child = path;
          child.push_back(int(n.children.size()));
          n.children.push_back(load_node(c.integer(), child));
        }
      return n;
    };
    const size_t first_new_node = m_nodes.size();
    for (const json::Value& root : model.at("scenes").at(0).at("nodes").arr) m_nodes.push_back(load_node(root.integer(), NodePath{int(m_nodes.size())}));
    m_transforms.resize(m_submesh_offsets.size());
    m_transforms_exact.resize(m_submesh_offsets.size());
    m_joints.resize(m_vertices.size(), std::array<uint16_t, 4>{0, 0, 0, 0});
    m_weights.resize(m_vertices.size(), std::array<float, 4>{0, 0, 0, 0});
    std::map<int, NodePath> joint_nodes;
    for (size_t k = 0; k < gskins.size(); ++k) {
      const json::Value& gs = gskins[k];
      Skin sk;
      sk.base = skin_base[k];
      for (const json::Value& j : gs.at("joints").arr) {
        if (!by_idx.count(j.integer())) throw std::runtime_error("a joint of a skin is not a node of the scene");
        sk.joints.push_back(by_idx[j.integer()]);
        joint_nodes[j.integer()] = by_idx[j.integer()];
      }
      if (gs.has("inverseBindMatrices")) {
        const json::Value& acc = model.at("accessors").at(size_t(gs.at("inverseBindMatrices").integer()));
        const View v = get_buffer(gs.at("inverseBindMatrices").integer());
        if (acc.at("componentType").integer() != 5126 || acc.at("type").string() != "MAT4" || v.stride != 64 || size_t(v.count) != sk.joints.size())
          throw std::runtime_error("inverseBindMatrices must be tightly packed float MAT4, one per joint");
        need(v, size_t(v.count) * 64);
        for (int i = 0; i < v.count; ++i) {
          Mat4d ib;  // column-major in the file
          for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) { float f; std::memcpy(&f, v.data + 64 * size_t(i) + 4 * size_t(4 * c + r), 4); ib.m[r][c] = double(f); }
          sk.inverse_bind.push_back(ib);
        }
      } else
        sk.inverse_bind.assign(sk.joints.size(), Mat4d{});
      if (skin_user.count(int(k))) sk.mesh_node = skin_user[int(k)];
      m_skins.push_back(sk);
    }
    update_transform();

    if (model.has("animations"))
      for (const json::Value& animation : model.at("animations").arr) {
        // without skins the node named by the FIRST channel drives every channel and must be a root node (find_node_node drops the result of its recursion,
        // scene.cpp:900-919); with skins: one record per distinct target node, in order of first appearance, each a root node or a joint of one of the file's skins
        std::vector<int> targets;
        if (gskins.empty()) targets.push_back(animation.at("channels").at(0).at("target").at("node").integer());
        else
          for (const json::Value& channel : animation.at("channels").arr) {
            const int t = channel.at("target").at("node").integer();
            if (std::find(targets.begin(), targets.end(), t) == targets.end()) targets.push_back(t);
          }
        for (const int target : targets) {
          Animation anim;
          NodePath where;
          for (size_t k = first_new_node; k < m_nodes.size(); ++k)
            if (m_nodes[k].idx == target) { where = NodePath{int(k)}; break; }
          if (where.empty() && joint_nodes.count(target)) where = joint_nodes[target];
          if (where.empty()) throw std::runtime_error("invalid target node");
          for (const json::Value& channel : animation.at("channels").arr) {
            if (!gskins.empty() && channel.at("target").at("node").integer() != target) continue;
            const json::Value& sampler = animation.at("samplers").at(size_t(channel.at("sampler").integer()));
            const std::string path = channel.at("target").at("path").string();
            const View in = get_buffer(sampler.at("input").integer());
            if (in.stride != 4) throw std::runtime_error("unsupported animation input");
            const View out = get_buffer(sampler.at("output").integer());
            if (in.count != out.count) throw std::runtime_error("animation input size is not equal to output size");
            const int per = path == "rotation" ? 4 : ((path == "translation" || path == "scale") ? 3 : 0);
            if (per == 0) continue;
            if (out.stride != 4 * per) throw std::runtime_error("invalid output stride");
            need(in, size_t(in.count) * 4); need(out, size_t(out.count) * 4 * per);
            auto f32 = [](const uint8_t* p) { float v; std::memcpy(&v, p, 4); return v; };
            for (int i = 0; i < in.count; ++i) {
              const float key = f32(in.data + 4 * i);
              const uint8_t* o = out.data + size_t(4 * per) * i;
              if (path == "translation") { anim.translation_input.push_back(key); anim.translation_output.push_back({double(f32(o)), double(f32(o + 4)), double(f32(o + 8))}); }
              else if (path == "scale") { anim.scale_input.push_back(key); anim.scale_output.push_back({double(f32(o)), double(f32(o + 4)), double(f32(o + 8))}); }
              else { anim.rotation_input.push_back(key); anim.rotation_output.push_back({double(f32(o + 12)), double(f32(o)), double(f32(o + 4)), double(f32(o + 8))}); }
            }
          }
          m_animations.push_back(anim);
          m_animation_targets.push_back(where[0]);  // an index, not the reference's Node*: m_nodes grows when files are appended
          m_animation_paths.push_back(where);
        }
      }
  }

  // scene.cpp:836-860
  void update_transform()
  {
    for (Node& node : m_nodes) visit(node, Mat4d{});
  }

  // scene.cpp:862-898
  void update_animation(float time)
  {
    for (size_t ai = 0; ai < m_animations.size(); ++ai) {
      const Animation& a = m_animations[ai];
      double t[3] = {0, 0, 0}, q[4] = {1, 0, 0, 0}, s[3] = {1, 1, 1};
      if (!a.translation_input.empty()) { const auto v = interpolate3(a.translation_input, a.translation_output, time); for (int k = 0; k < 3; ++k) t[k] = v[size_t(k)]; }
      if (!a.rotation_input.empty()) { const auto v = interpolate4(a.rotation_input, a.rotation_output, time); for (int k = 0; k < 4; ++k) q[k] = v[size_t(k)]; }
      if (!a.scale_input.empty()) { const auto v = interpolate3(a.scale_input, a.scale_output, time); for (int k = 0; k < 3; ++k) s[k] = v[size_t(k)]; }
      node_at(m_animation_paths.at(ai)).transform = Mat4d::trs(t, q, s);
    }
    update_transform();
  }

  std::vector<int> m_animation_targets;      // index into m_nodes of the root every animation's node is, or is below
  std::vector<NodePath> m_animation_paths;   // where every animation's node is

  Node& node_at(const NodePath& path)
  {
    Node* n = &m_nodes.at(size_t(path.at(0)));
    for (size_t k = 1; k < path.size(); ++k) n = &n->children.at(size_t(path[k]));
    return *n;
  }

  // the palette as fh_set_joint_matrices takes it, 12 floats per joint of all skins: inverse(global(mesh node)) * global(joint node) * inverseBind, multiplied in
  // double and rounded once.  The instance's own object_to_world stays the mesh node's global transform, so world space is global(joint) * inverseBind as glTF prescribes
  std::vector<float> joint_matrices_3x4()
  {
    std::vector<float> out;
    for (const Skin& sk : m_skins) {
      const Mat4d to_object = sk.mesh_node.empty() ? Mat4d{} : node_at(sk.mesh_node).global.affine_inverse();
      for (size_t k = 0; k < sk.joints.size(); ++k) {
        const Mat4d m = Mat4d::mul(Mat4d::mul(to_object, node_at(sk.joints[k]).global), sk.inverse_bind[k]);
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 4; ++c) out.push_back(float(m.m[r][c]));
      }
    }
    return out;
  }
  uint32_t n_joints() const
  {
    uint32_t n = 0;
    for (const Skin& sk : m_skins) n += uint32_t(sk.joints.size());
    return n;
  }

  // instance transforms as the C ABI takes them: 3x4 row-major float, the inverse taken in double before rounding.  A matrix the
  // caller edited in m_transforms (float) wins over the stored double one.
  void transforms_3x4(std::vector<float>& o2w, std::vector<float>& w2o) const
  {
    for (size_t k = 0; k < m_transforms.size(); ++k) {
      Mat4d m = Mat4d::from_float(m_transforms[k]);
      if (k < m_transforms_exact.size()) {
        const Mat4 f = m_transforms_exact[k].to_float();
        bool same = true;
        for (int c = 0; c < 4 && same; ++c)
          for (int r = 0; r < 4; ++r) same = same && f[c][r] == m_transforms[k][c][r];
        if (same) m = m_transforms_exact[k];
      }
      const Mat4d inv = m.affine_inverse();
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) { o2w.push_back(float(m.m[r][c])); w2o.push_back(float(inv.m[r][c])); }
    }
  }

 private:
  void visit(Node& node, const Mat4d& parent)
  {
    const Mat4d m = Mat4d::mul(parent, node.transform);
    node.global = m;
    if (node.camera_id != -1) { m_has_camera_transform = true; m_camera_transform = m.to_float(); }
    if (node.submesh_id != -1) { m_transforms_exact[size_t(node.submesh_id)] = m; m_transforms[size_t(node.submesh_id)] = m.to_float(); }
    for (Node& c : node.children) visit(c, m);
  }
  // scene.h:164-178: t = fmod(time, last key); h = t - input[idx0] (not divided by the key interval)
  static void bracket(const std::vector<float>& input, float time, size_t n_out, size_t& idx0, size_t& idx1, double& h)
  {
    const float last = input.back();
    const float t = last != 0.0f ? std::fmod(time, last) : 0.0f;
    const size_t lb = size_t(std::lower_bound(input.begin(), input.end(), t) - input.begin());
    idx0 = lb > 0 ? lb - 1 : 0;
    idx1 = std::min(lb, n_out - 1);
    h = double(t - input[idx0]);
  }
  static std::array<double, 3> interpolate3(const std::vector<float>& input, const std::vector<std::array<double, 3>>& output, float time)
  {
    size_t i0, i1;
    double h;
    bracket(input, time, output.size(), i0, i1, h);
    std::array<double, 3> r;
    for (size_t k = 0; k < 3; ++k) r[k] = output[i0][k] * (1.0 - h) + output[i1][k] * h;
    return r;
  }
  // glm::mix(quat, quat, a): spherical interpolation without the shortest-path flip; linear when nearly parallel
  static std::array<double, 4> interpolate4(const std::vector<float>& input, const std::vector<std::array<double, 4>>& output, float time)
  {
    size_t i0, i1;
    double a;
    bracket(input, time, output.size(), i0, i1, a);
    const std::array<double, 4>&x = output[i0], &y = output[i1];
    const double cos_theta = x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
    std::array<double, 4> r;
    if (cos_theta > 1.0 - 1.1920928955078125e-07) {
      for (size_t k = 0; k < 4; ++k) r[k] = x[k] * (1.0 - a) + y[k] * a;
      return r;
    }
    const double angle = std::acos(cos_theta);
    const double s0 = std::sin((1.0 - a) * angle), s1 = std::sin(a * angle), sn = std::sin(angle);
    for (size_t k = 0; k < 4; ++k) r[k] = (s0 * x[k] + s1 * y[k]) / sn;
    return r;
  }
  static int component_size(int component_type)
  {
    switch (component_type) {
      case 5120: case 5121: return 1;
      case 5122: case 5123: return 2;
      case 5125: case 5126: return 4;
      default: throw std::runtime_error("unknown accessor component type");
    }
  }
  static int type_count(const std::string& t)
  {
    if (t == "SCALAR") return 1;
    if (t == "VEC2") return 2;
    if (t == "VEC3") return 3;
    if (t == "VEC4" || t == "MAT2") return 4;
    if (t == "MAT3") return 9;
    if (t == "MAT4") return 16;
    throw std::runtime_error("unknown accessor type");
  }
  static std::vector<uint8_t> base64_decode(const std::string& in)
  {
    std::vector<uint8_t> out;
    uint32_t acc = 0;
    int bits = 0;
    for (char ch : in) {
      int v;
      if (ch >= 'A' && ch <= 'Z') v = ch - 'A';
      else if (ch >= 'a' && ch <= 'z') v = ch - 'a' + 26;
      else if (ch >= '0' && ch <= '9') v = ch - '0' + 52;
      else if (ch == '+' || ch == '-') v = 62;
      else if (ch == '/' || ch == '_') v = 63;
      else continue;  // padding, whitespace
      acc = (acc << 6) | uint32_t(v);
      bits += 6;
      if (bits >= 8) { bits -= 8; out.push_back(uint8_t((acc >> bits) & 0xffu)); }
    }
    return out;
  }

 public:

 private:
  static float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
  static float3 norm3(float3 a)
  {
    const float l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    return make_float3(a.x / l, a.y / l, a.z / l);
  }

  void load_mtl(const std::filesystem::path& path, std::map<std::string, int>& mat_index, std::map<std::string, int>& unique_textures)
  {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("failed to load " + path.generic_string());
    Material* cur = nullptr;
    float clearcoat_thickness = 0.0f;
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ss(line);
      std::string tag;
      if (!(ss >> tag) || tag[0] == '#') continue;
      if (tag == "newmtl") {
        std::string name;
        ss >> name;
        mat_index[name] = int(m_materials.size());
        Material m;
        m.base_color = make_float3(0, 0, 0);      // tinyobjloader initialises Kd / Ks to 0 (scene.cpp:196, :210)
        m.specular_color = make_float3(0, 0, 0);
        m_materials.push_back(m);
        cur = &m_materials.back();
        clearcoat_thickness = 0.0f;
        continue;
      }
      if (!cur) continue;
      auto f1 = [&]() { float v = 0; ss >> v; return v; };
      auto f3 = [&]() { float3 v{0, 0, 0}; ss >> v.x >> v.y >> v.z; return v; };
      if (tag == "Kd") cur->base_color = f3();
      else if (tag == "Ks") cur->specular_color = f3();
      else if (tag == "Pr") { const float v = f1(); if (v > 0) cur->specular_roughness = v; }
      else if (tag == "Pm") cur->metalness = f1();
      else if (tag == "Pc") { clearcoat_thickness = f1(); if (clearcoat_thickness > 0) cur->coat = clearcoat_thickness; }
      else if (tag == "Pcr") { const float v = f1(); if (v > 0) cur->coat_roughness = clearcoat_thickness; }
      else if (tag == "d") cur->transmission = std::fmax(1.0f - f1(), 0.0f);
      else if (tag == "Tr") cur->transmission = std::fmax(f1(), 0.0f);
      else if (tag == "Tf") { const float3 v = f3(); if (v.x > 0 || v.y > 0 || v.z > 0) cur->transmission_color = v; }
      else if (tag == "Ke") { const float3 v = f3(); if (v.x > 0 || v.y > 0 || v.z > 0) { cur->emission = 1.0f; cur->emission_color = v; } }
      else if (tag == "diffuse") cur->diffuse = f1();
      else if (tag == "diffuse_roughness") cur->diffuse_roughness = f1();
      else if (tag == "sheen") cur->sheen = f1();
      else if (tag == "sheen_color") cur->sheen_color = f3();
      else if (tag == "sheen_roughness") cur->sheen_roughness = f1();
      else if (tag == "subsurface") cur->subsurface = f1();
      else if (tag == "subsurface_color") cur->subsurface_color = f3();
      else if (tag == "thin_walled") cur->thin_walled = f1();
      else if (tag == "map_Kd" || tag == "map_Ks" || tag == "map_Pr" || tag == "map_Pm" || tag == "map_bump" || tag == "map_Bump" || tag == "bump" || tag == "norm" || tag == "map_d") {
        std::string name, tok;
        while (ss >> tok) name = tok;  // options ("-bm 1") precede the file name
        const bool color = tag == "map_Kd" || tag == "map_Ks";
        if (!unique_textures.count(name)) {  // scene.cpp:144-153
          unique_textures[name] = int(m_textures.size());
          m_textures.push_back(Texture(path.parent_path() / name, color ? TextureType::COLOR : TextureType::NONCOLOR));
        }
        const int id = unique_textures[name];
        if (tag == "map_Kd") cur->base_color_texture_id = id;
        else if (tag == "map_Ks") cur->specular_color_texture_id = id;
        else if (tag == "map_Pr") cur->specular_roughness_texture_id = id;
        else if (tag == "map_Pm") cur->metalness_texture_id = id;
        else if (tag == "norm") cur->normalmap_texture_id = id;
        else if (tag == "map_d") cur->alpha_texture_id = id;
        else cur->heightmap_texture_id = id;
      } else if (tag.rfind("map_", 0) == 0)
        throw std::runtime_error(tag + " is not a texture slot of the reference's .mtl mapping (" + path.generic_string() + ")");
    }
  }
};

}  // namespace fredholm
