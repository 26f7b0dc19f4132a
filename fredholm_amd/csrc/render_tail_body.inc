// render_tail_body.inc -- the body of k_tail, k_tail_env and k_tail_lt (render.hip includes it into all three).  In scope: sc, fr, pool, first_depth, coop_flush; ENV and env; LT and ltab
// It is text, not a function: it reads the names sc, fr, pool, ENV, env, LT and ltab of the kernel it is included into.  The plain k_tail must keep its instruction stream, so after ANY
// edit here compare a device listing of render.hip with the one before the edit (tools/kernel_asm_diff.py): k_tail<...> may differ in nothing.
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];  // traversal stack of every lane ([entry][thread], as in the streaming kernels): a private array lands in scratch
  __shared__ __attribute__((aligned(16))) unsigned char lds_coop[(kBlock / 64) * kCoopLdsBytesPerWave];
  __shared__ float4 s_in[kBlock / 64][2][64];  // one round of packed rays of a wave: (origin, tmax), (direction, stops at its first hit)
  __shared__ float4 s_out[kBlock / 64][64];    // and their hits: t, u, v, face id bits
  if (blockIdx.x * blockDim.x >= pool.counters[first_depth * kCounterStride + CNT_RAD]) return;  // (the grid is sized for the pass, the survivors are few: most blocks have nothing to do, and leave before the tables are staged)
  const CoopLds cl = coop_lds(lds_coop, threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const bool coop = sc.use_bvh8 && coop_flush != 0u;
  // all rays of the wave (called by its 64 lanes together)
  auto trace_all = [&](TailRay (&rays)[kTailRays]) {
    if (!coop) {  // one ray per lane, per-lane loops: tiny scenes (binary tree) and FH_COOP=0 (an out-of-line call per ray: five inlined copies of every traversal would be most of the kernel)
      HitRec t;  // (only this one has its address taken: the rays themselves stay in registers)
      if (rays[0].has) { rays[0].hit = tail_trace_lane(sc, lds_stack, rays[0].any, rays[0].o, rays[0].d, rays[0].tmax, t); rays[0].h = t; }
      if (rays[1].has) { rays[1].hit = tail_trace_lane(sc, lds_stack, rays[1].any, rays[1].o, rays[1].d, rays[1].tmax, t); rays[1].h = t; }
      if (rays[2].has) { rays[2].hit = tail_trace_lane(sc, lds_stack, rays[2].any, rays[2].o, rays[2].d, rays[2].tmax, t); rays[2].h = t; }
      if (rays[3].has) { rays[3].hit = tail_trace_lane(sc, lds_stack, rays[3].any, rays[3].o, rays[3].d, rays[3].tmax, t); rays[3].h = t; }
      if (rays[4].has) { rays[4].hit = tail_trace_lane(sc, lds_stack, rays[4].any, rays[4].o, rays[4].d, rays[4].tmax, t); rays[4].h = t; }
      return;
    }
    uint32_t idx[kTailRays], total = 0;  // position of this lane's ray of kind k among the wave's rays; total: wave-uniform
#pragma unroll
    for (uint32_t k = 0; k < kTailRays; ++k) {
      const unsigned long long m = __ballot(rays[k].has);
      idx[k] = total + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      total += (uint32_t)__popcll(m);
    }
    for (uint32_t lo = 0; lo < total; lo += 64u) {
#pragma unroll
      for (uint32_t k = 0; k < kTailRays; ++k)
        if (rays[k].has && idx[k] - lo < 64u) {
          s_in[wave][0][idx[k] - lo] = mk4(rays[k].o, rays[k].tmax);
          s_in[wave][1][idx[k] - lo] = mk4(rays[k].d, rays[k].any ? 1.0f : 0.0f);
        }
      const bool valid = lo + lane < total;
      const float4 a = valid ? s_in[wave][0][lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = valid ? s_in[wave][1][lane] : make_float4(0.0f, 0.0f, 1.0f, 0.0f);
      HitRec h;
      uint32_t na = 0, nb = 0;
      if (sc.has_alpha) traverse_bvh8_coop_mode<2, false, true, true>(sc.bvh8, valid, b.w != 0.0f, mk3(a), mk3(b), a.w, h, na, nb, nullptr, cl, coop_flush, lds_stack, (int)sc.bvh8.depth, &sc);
      else traverse_bvh8_coop_mode<2, false, true, false>(sc.bvh8, valid, b.w != 0.0f, mk3(a), mk3(b), a.w, h, na, nb, nullptr, cl, coop_flush, lds_stack, (int)sc.bvh8.depth, &sc);
      if (valid) s_out[wave][lane] = make_float4(h.t, h.u, h.v, __uint_as_float(h.prim));
#pragma unroll
      for (uint32_t k = 0; k < kTailRays; ++k)
        if (rays[k].has && idx[k] - lo < 64u) {
          const float4 r = s_out[wave][idx[k] - lo];
          rays[k].h.t = r.x; rays[k].h.u = r.y; rays[k].h.v = r.z; rays[k].h.prim = __float_as_uint(r.w);
          rays[k].hit = rays[k].h.prim != 0xffffffffu;
        }
    }
  };
  __shared__ SobolRows<4> rows;
  __shared__ float s_lut[kLutReflFloats + kLutSheenFloats];  // as in k_shade: small tables every hit reads live in LDS
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
  __shared__ HosekSky s_sky;
  stage_sky(fr, s_sky);
  __syncthreads();
  const uint32_t count = pool.counters[first_depth * kCounterStride + CNT_RAD];
  const uint32_t* q = pool.q_rad[first_depth & 1u];
  const bool has_lights = sc.n_lights > 0;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t base = blockIdx.x * blockDim.x; base < count; base += stride) {  // (block-uniform bound: the bounce loop holds workgroup barriers)
    const uint32_t i = base + threadIdx.x;
    bool alive = i < count;
    uint32_t p = 0, image_idx = 0, n_spp = 0;
    f3 ro = mk3(0.0f), rd = mk3(0.0f, 0.0f, 1.0f), T = mk3(0.0f), L = mk3(0.0f);
    if (alive) {
      p = q[i];
      const float4 o = pool.ray_o[p];
      ro = mk3(o); rd = mk3(pool.ray_d[p]); T = mk3(pool.thr[p]); L = mk3(pool.rad[p]);
      image_idx = pool.pixel[p]; n_spp = pool.nspp[p];
    }
    // the closest hit of the first bounce; every later one comes back with the rays of the bounce before it
    HitRec h;
    bool hit = false;
    {
      TailRay rays[kTailRays];
      rays[SEC_COUNT].has = alive; rays[SEC_COUNT].any = false; rays[SEC_COUNT].o = ro; rays[SEC_COUNT].d = rd; rays[SEC_COUNT].tmax = 1e9f;
      trace_all(rays);
      h = rays[SEC_COUNT].h; hit = rays[SEC_COUNT].hit;
    }
    for (uint32_t depth = first_depth; depth < fr.max_depth; ++depth) {
      BounceSlots bs;
      bs.set(fr, sc.n_lights, depth);
      __syncthreads();  // rows of the previous bounce are no longer read
      bs.load_rows(rows, fr.sobol_bytes);
      if (__ballot(alive) == 0ull) continue;  // (wave-uniform; the barriers above are still met)
      ShadeOut o;
      if (alive) {
        if (!hit) alive = false;  // pt.cu:504-523 with firsthit == false: nothing added
        else shade_hit<LOBES, ENV, LT>(sc, fr, rows, bs, depth, make_float4(h.t, h.u, h.v, __uint_as_float(h.prim)), rd, T, L, image_idx, n_spp, o, true, env, ltab);
      }
      TailRay rays[kTailRays];
#pragma unroll
      for (uint32_t slot = SEC_DIR; slot <= SEC_LIGHT; ++slot) {
        if (slot == SEC_DIR && !fr.has_dir) continue;
        if (slot == SEC_AREA && !has_lights) continue;
        rays[slot].has = alive && o.sec[slot].active;
        rays[slot].any = !(slot == SEC_LIGHT && has_lights);
        rays[slot].o = o.sec[slot].o; rays[slot].d = o.sec[slot].d; rays[slot].tmax = o.sec[slot].tmax;
      }
      rays[SEC_COUNT].has = alive && o.cont; rays[SEC_COUNT].any = false; rays[SEC_COUNT].o = o.next_o; rays[SEC_COUNT].d = o.next_d; rays[SEC_COUNT].tmax = 1e9f;
      trace_all(rays);
      // secondary rays in the reference's order
#pragma unroll
      for (uint32_t slot = SEC_DIR; slot <= SEC_LIGHT; ++slot) {
        if (!rays[slot].has) continue;
        if (slot == SEC_LIGHT && has_lights) L += resolve_light_ray<LT>(sc, fr, o.lp_T, o.lp_cos, o.lp_f, o.lp_pdf, o.sec[slot].o, o.sec[slot].d, rays[slot].hit, rays[slot].h, LT ? ltab->pick_p : nullptr);
        else if (!rays[slot].hit) L += o.sec[slot].c;
      }
      if (alive) {
        if (o.cont) { rd = o.next_d; T = o.T; h = rays[SEC_COUNT].h; hit = rays[SEC_COUNT].hit; }
        else alive = false;
      }
    }
    if (i < count) pool.rad[p] = mk4(L, 0.0f);
  }
