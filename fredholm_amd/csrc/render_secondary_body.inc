// render_secondary_body.inc -- the bodies of the four secondary-ray kernels and of their twins that take the light table (render.hip includes it into both; FH_BODY_STATIC,
// _COOP, _STREAM or _MERGED selects the section).  In scope: the kernel's parameters and template flags; LT and pick_p (fh_set_light_sampling: nullptr in the plain kernels)
// It is text, not a function, for the reason render_shade_body.inc gives: the plain kernels must keep their instruction streams, so after ANY edit here compare a device
// listing of render.hip with the one before the edit (tools/kernel_asm_diff.py).
#if defined(FH_BODY_STATIC)
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];  // [entry][thread], sized by the launcher for the depth of the BVH
  __shared__ HosekSky s_sky;  // (light rays that escape see the sky: resolve_light_ray)
  if (LIGHTS) { stage_sky(fr, s_sky); __syncthreads(); }
  const uint32_t count = pool.counters[depth * kCounterStride + CNT_SEC];
  constexpr bool has_lights = LIGHTS;
  uint32_t nn = 0, nt = 0, nr = 0;
  WaveSteps ws;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
    const uint32_t p = pool.q_sec[i];
    f3 L = mk3(pool.rad[p]);
#pragma unroll
    for (uint32_t slot = SEC_DIR; slot <= SEC_LIGHT; ++slot) {
      if (slot == SEC_DIR && !fr.has_dir) continue;
      if (slot == SEC_AREA && !has_lights) continue;
      const size_t k = pool.sec_at(slot, p);
      const float4 d = pool.sec[k + 1];
      if (!sec_present(d)) continue;
      const float4 o = pool.sec[k];
      HitRec h;
      if (COUNT) nr++;
      if (slot == SEC_LIGHT && has_lights) {
        const bool hit = WIDE ? traverse_bvh8<false, COUNT, true, ALPHA>(sc.bvh8, mk3(o), mk3(d), o.w, h, nn, nt, &ws, lds_stack, (int)sc.bvh8.depth, &sc)
                              : traverse_bvh2<false, COUNT, ALPHA>(sc.bvh2, mk3(o), mk3(d), o.w, h, nn, nt, &sc);
        const float4 la = pool.lp_a[p], lb = pool.lp_b[p];
        L += resolve_light_ray<LT>(sc, fr, mk3(la), la.w, mk3(lb), lb.w, mk3(o), mk3(d), hit, h, pick_p);
      } else {
        const uint32_t nn0 = nn;
        const bool occluded = WIDE ? traverse_bvh8<true, COUNT, true, ALPHA>(sc.bvh8, mk3(o), mk3(d), o.w, h, nn, nt, &ws, lds_stack, (int)sc.bvh8.depth, &sc)
                                   : traverse_bvh2<true, COUNT, ALPHA>(sc.bvh2, mk3(o), mk3(d), o.w, h, nn, nt, &sc);
        if (COUNT) { const uint32_t kk = nn - nn0; int b = 0; while (b < 7 && kk > (8u << b)) ++b; atomicAdd(tc.hist + b, 1ull); }
        if (!occluded) L += mk3(pool.sec[k + 2]);
      }
    }
    pool.rad[p] = mk4(L, 0.0f);
  }
  if (COUNT) {
    atomicAdd(tc.nodes, (unsigned long long)nn);
    atomicAdd(tc.tris, (unsigned long long)nt);
    atomicAdd(tc.rays, (unsigned long long)nr);
    if (ws.node) atomicAdd(tc.wave_nodes, (unsigned long long)ws.node);
    if (ws.tri) atomicAdd(tc.wave_tris, (unsigned long long)ws.tri);
  }
#elif defined(FH_BODY_COOP)
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];  // [entry][thread], sized by the launcher for the depth of the BVH
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kCoopLdsBytesPerWave];
  const CoopLds cl = coop_lds(lds, threadIdx.x >> 6);
  __shared__ HosekSky s_sky;  // (light rays that escape see the sky: resolve_light_ray)
  if (LIGHTS) { stage_sky(fr, s_sky); __syncthreads(); }
  const uint32_t count = pool.counters[depth * kCounterStride + CNT_SEC];
  constexpr bool has_lights = LIGHTS;
  uint32_t nn = 0, nt = 0, nr = 0;
  WaveSteps ws;
  for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < count; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + (threadIdx.x & 63u);
    const bool in_range = i < count;
    const uint32_t p = in_range ? pool.q_sec[i] : 0u;
    f3 L = in_range ? mk3(pool.rad[p]) : mk3(0.0f);
#pragma unroll
    for (uint32_t slot = SEC_DIR; slot <= SEC_LIGHT; ++slot) {
      if (slot == SEC_DIR && !fr.has_dir) continue;
      if (slot == SEC_AREA && !has_lights) continue;
      const size_t k = pool.sec_at(slot, p);
      const float4 d = in_range ? pool.sec[k + 1] : make_float4(0.0f, 0.0f, 1.0f, 0.0f);
      const bool valid = in_range && sec_present(d);
      if (__ballot(valid) == 0ull) continue;
      const float4 o = valid ? pool.sec[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      HitRec h;
      if (COUNT && valid) nr++;
      if (slot == SEC_LIGHT && has_lights) {
        const bool hit = traverse_bvh8_coop<false, COUNT, true, ALPHA>(sc.bvh8, valid, mk3(o), mk3(d), o.w, h, nn, nt, &ws, cl, flush, lds_stack, (int)sc.bvh8.depth, &sc);
        if (valid) {
          const float4 la = pool.lp_a[p], lb = pool.lp_b[p];
          L += resolve_light_ray<LT>(sc, fr, mk3(la), la.w, mk3(lb), lb.w, mk3(o), mk3(d), hit, h, pick_p);
        }
      } else {
        const uint32_t nn0 = nn;
        const bool occluded = traverse_bvh8_coop<true, COUNT, true, ALPHA>(sc.bvh8, valid, mk3(o), mk3(d), o.w, h, nn, nt, &ws, cl, flush, lds_stack, (int)sc.bvh8.depth, &sc);
        if (COUNT && valid) { const uint32_t kk = nn - nn0; int b = 0; while (b < 7 && kk > (8u << b)) ++b; atomicAdd(tc.hist + b, 1ull); }
        if (valid && !occluded) L += mk3(pool.sec[k + 2]);
      }
    }
    if (in_range) pool.rad[p] = mk4(L, 0.0f);
  }
  if (COUNT) {
    atomicAdd(tc.nodes, (unsigned long long)nn);
    atomicAdd(tc.tris, (unsigned long long)nt);
    atomicAdd(tc.rays, (unsigned long long)nr);
    if (ws.node) atomicAdd(tc.wave_nodes, (unsigned long long)ws.node);
    if (ws.tri) atomicAdd(tc.wave_tris, (unsigned long long)ws.tri);
  }
#elif defined(FH_BODY_STREAM)
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];  // [entry][thread], sized by the launcher for the depth of the BVH
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kCoopLdsBytesPerWave];
  const uint32_t count = pool.counters[depth * kCounterStride + CNT_SEC];
  if (stream_block_idle(count, min_rays)) return;
  __shared__ HosekSky s_sky;  // (light rays that escape see the sky: resolve_light_ray)
  if (LIGHTS) { stage_sky(fr, s_sky); __syncthreads(); }
  const ClockStamp stamp;
  CoopLds cl = coop_lds(lds, threadIdx.x >> 6);
  AlphaLds<AlphaDefer<true, ALPHA>::value>::attach(cl);  // candidates waiting for their any-hit test (fh_trace.h: alpha_ring): LDS of the kernels with the test compiled in only
  uint32_t nn = 0, nt = 0;
  WaveSteps ws;
  SecondaryStream<COUNT, LIGHTS, LT> pol(sc, fr, pool, ChunkFeed(pool.counters + depth * kCounterStride + CNT_CUR_SEC, count, stream_chunk_for(count, chunk)), tc.hist, pick_p);
  __shared__ uint4 lds_top[kTopNodes * 4];
  stage_top_nodes(sc.bvh8, lds_top);
  traverse_stream<true, COUNT, true, ALPHA>(sc.bvh8, pol, nn, nt, &ws, cl, flush, refill, lds_stack, (int)sc.bvh8.depth, &sc, spill, lds_top,
                                            spill.probe ? pool.counters + depth * kCounterStride + CNT_COST_NODE : nullptr);
  pol.finish();
  stamp.commit(tc.clk);
  if (COUNT) {
    atomicAdd(tc.nodes, (unsigned long long)nn);
    atomicAdd(tc.tris, (unsigned long long)nt);
    atomicAdd(tc.rays, (unsigned long long)pol.n_rays);
    pol.hp.flush(tc.hist);
    if (ws.node) atomicAdd(tc.wave_nodes, (unsigned long long)ws.node);
    if (ws.tri) atomicAdd(tc.wave_tris, (unsigned long long)ws.tri);
  }
#elif defined(FH_BODY_MERGED)
  pass_priority();
  extern __shared__ __attribute__((aligned(16))) uint2 lds_stack[];
  __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * kCoopLdsBytesPerWave];
  const uint32_t n_sec = ps.counters[depth * kCounterStride + CNT_SEC], n_closest = ps.counters[(depth + 1u) * kCounterStride + CNT_RAD];
  const uint32_t count = n_sec + n_closest;
  if (stream_block_idle(count, min_rays)) return;
  __shared__ HosekSky s_sky;
  if (LIGHTS) { stage_sky(fr, s_sky); __syncthreads(); }
  const ClockStamp stamp;
  CoopLds cl = coop_lds(lds, threadIdx.x >> 6);
  AlphaLds<AlphaDefer<true, ALPHA>::value>::attach(cl);  // candidates waiting for their any-hit test (fh_trace.h: alpha_ring): LDS of the kernels with the test compiled in only
  uint32_t nn = 0, nt = 0;
  MergedStream<LIGHTS, LT> pol(sc, fr, ps, pn, pn.q_rad[(depth + 1u) & 1u], n_sec, ChunkFeed(ps.counters + depth * kCounterStride + CNT_CUR_SEC, count, stream_chunk_for(count, chunk)), pick_p);
  __shared__ uint4 lds_top[kTopNodes * 4];
  stage_top_nodes(sc.bvh8, lds_top);
  traverse_stream<true, false, true, ALPHA>(sc.bvh8, pol, nn, nt, nullptr, cl, flush, refill, lds_stack, (int)sc.bvh8.depth, &sc, spill, lds_top,
                                            spill.probe ? ps.counters + depth * kCounterStride + CNT_COST_NODE : nullptr);
  pol.sec.finish();
  stamp.commit(tc.clk);
#endif
