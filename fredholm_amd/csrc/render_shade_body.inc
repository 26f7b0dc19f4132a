// render_shade_body.inc -- the body of k_shade, k_shade_env and k_shade_lt (render.hip includes it into all three).  In scope: sc, fr, pool, cls, depth; ENV and env; LT and ltab
// It is text, not a function: it reads the names sc, fr, pool, ENV, env, LT and ltab of the kernel it is included into.  The plain k_shade must keep its instruction stream, so after ANY
// edit here compare a device listing of render.hip with the one before the edit (tools/kernel_asm_diff.py): k_shade<...> may differ in nothing.
// (One change altered that stream on purpose, from outside this file: the divisions of concentric_disk and of the Hosek sky took their short form -- fh_vec.h: div_r.  The
// listing to compare with is the one from after it.)
  pass_priority();
  // (the grid is sized for every path of the pass; the blocks beyond this class's queue leave before they stage anything)
  if (blockIdx.x * blockDim.x >= pool.counters[depth * kCounterStride + CNT_CLS + cls]) return;
  __shared__ SobolRows<4> rows;
  // the shade kernels run one wave per SIMD (512 registers per lane), so nothing hides a dependent global load: the small tables every
  // hit reads -- the two albedo LUTs and, when there are few of them, the material records -- are staged in LDS once per workgroup
  __shared__ float s_lut[kLutReflFloats + kLutSheenFloats];
  __shared__ MaterialDev s_mat[kMatLds];
  for (uint32_t i = threadIdx.x; i < kLutReflFloats; i += blockDim.x) s_lut[i] = fr.lut.reflection[i];
  for (uint32_t i = threadIdx.x; i < kLutSheenFloats; i += blockDim.x) s_lut[kLutReflFloats + i] = fr.lut.sheen[i];
  fr.lut.reflection = s_lut;
  fr.lut.sheen = s_lut + kLutReflFloats;
  if (sc.n_materials <= kMatLds) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(sc.materials);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_mat);
    for (uint32_t i = threadIdx.x; i < sc.n_materials * (uint32_t)(sizeof(MaterialDev) / 4); i += blockDim.x) dst[i] = src[i];
    sc.materials = s_mat;
  }
  __shared__ float s_srgb[256];  // the sRGB decode table: twelve lookups per fetch of a colour texture
  if (sc.n_textures) {
    s_srgb[threadIdx.x] = sc.srgb_lut[threadIdx.x];
    sc.srgb_lut = s_srgb;
  }
  __shared__ HosekSky s_sky;
  stage_sky(fr, s_sky);
  BounceSlots bs;
  bs.set(fr, sc.n_lights, depth);
  bs.load_rows(rows, fr.sobol_bytes);  // (ends with the workgroup barrier that also publishes the tables above)

  uint32_t* cnt = pool.counters + depth * kCounterStride;
  uint32_t* cnt_next = cnt + kCounterStride;
  const uint32_t count = cnt[CNT_CLS + cls];
  const uint32_t* q = pool.q_cls + (size_t)cls * pool.capacity;
  const uint32_t qnext = (depth + 1u) & 1u;
  const uint32_t stride = gridDim.x * blockDim.x;
  __shared__ uint32_t s_reserve[2][10];  // (two areas, used alternately: block_queue_reserve)
  uint32_t iter = 0;
  for (uint32_t base = blockIdx.x * blockDim.x; base < count; base += stride) {
    const uint32_t i = base + threadIdx.x;
    const bool valid = i < count;
    bool shaded = false, cont = false;
    uint32_t p = 0, cell = 0;
    if (valid) {
      p = q[i];
      const float4 hit = pool.hit[p];
      PoolSink o(pool, p, hit.x);
      const bool first = depth != 0 || (pool.flags[p] & 4u) == 0u;
      const f3 L = depth == 0u ? mk3(pool.rad[p]) : mk3(0.0f);  // the radiance so far only enters at a directly visible emitter (first hit): later bounces skip the load
      shade_hit<LOBES, ENV, LT>(sc, fr, rows, bs, depth, hit, mk3(pool.ray_d[p]), mk3(pool.thr[p]), L, pool.pixel[p], pool.nspp[p], o, first, env, ltab);
      shaded = o.shaded;
      cont = o.cont;
      if (shaded || cont) cell = cell_of(fr, o.origin);
    }
    // queue positions of both appends: one returning atomic per workgroup and queue (fh_device.h: block_queue_reserve)
    uint32_t* const counters2[2] = {&cnt[CNT_SEC], &cnt_next[CNT_RAD]};
    const bool act[2] = {shaded, cont};
    uint32_t pos[2];
    block_queue_reserve<2>(counters2, act, pos, s_reserve[iter & 1u]);
    ++iter;
    if (shaded) { pool.q_sec[pos[0]] = p; pool.key_sec[pos[0]] = (uint16_t)cell; }
    if (cont) { pool.q_rad[qnext][pos[1]] = p; pool.key_rad[pos[1]] = (uint16_t)cell; }
  }
