// The body of k_temporal_response<KIND> and k_temporal_response_noise<KIND> (denoise.hip includes it into both; nothing else does).  In scope: KIND, A, M, gamma,
// kappa, and NOISE: whether step 4b of the header runs.
  __shared__ float4 s_cv[kGN];  // c.rgb, v of the preparation
  __shared__ float4 s_n[kGN];   // N; 0 outside the frame
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int tid = threadIdx.y * kTW + threadIdx.x;
  for (int k = tid; k < kGN; k += 256) {
    const int qx = x0 + k % kGW - 2, qy = y0 + k / kGW - 2;
    float4 cq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nq = cq;
    if (qx >= 0 && qx < A.w && qy >= 0 && qy < A.h) { cq = A.cv[qx + A.w * qy]; nq = A.normal[qx + A.w * qy]; }
    s_cv[k] = cq;
    s_n[k] = nq;
  }
  __syncthreads();
  const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
  if (x >= A.w || y >= A.h) return;
  const int p = x + A.w * y;
  const int kc = ((int)threadIdx.y + 2) * kGW + (int)threadIdx.x + 2;
  const float4 cv = s_cv[kc], np = s_n[kc], pp = A.position[p];
  float cx = cv.x, cy = cv.y, cz = cv.z, v = cv.w, hist = 0.0f;
  if (td_hit(np)) {
    hist = 1.0f;
    bool have = false;
    float hx = 0.0f, hy = 0.0f, hz = 0.0f, hv = 0.0f, hh = 0.0f;
    const float lim = A.plane_tol * fmaxf(A.depth[p], 1e-3f);
    bool own = KIND == 1;
    float4 nb = np, pb = pp;
    if constexpr (KIND == 3) {
      const uint32_t inst = M.ids[p];
      const bool carried = inst < M.n_instances && M.motion[inst < M.n_instances ? inst : 0u].moved != 0u;
      own = !carried && M.still;
      if (carried) {
        const float* a = M.motion[inst].point;
        const float* g = M.motion[inst].normal;
        pb.x = ((a[0] * pp.x + a[1] * pp.y) + a[2] * pp.z) + a[3];
        pb.y = ((a[4] * pp.x + a[5] * pp.y) + a[6] * pp.z) + a[7];
        pb.z = ((a[8] * pp.x + a[9] * pp.y) + a[10] * pp.z) + a[11];
        nb.x = (g[0] * np.x + g[1] * np.y) + g[2] * np.z;
        nb.y = (g[3] * np.x + g[4] * np.y) + g[5] * np.z;
        nb.z = (g[6] * np.x + g[7] * np.y) + g[8] * np.z;
      }
    }
    if (own) {
      const float4 qc = A.h_cv[p], qp = A.h_ph[p], qn = A.h_n[p];
      have = td_valid(A, np, pp, lim, qn, qp);
      hx = qc.x; hy = qc.y; hz = qc.z; hv = qc.w; hh = qp.w;
    } else {
      have = td_reproject(A, nb, pb, lim, hx, hy, hz, hv, hh);
    }
    if (have) {
      // 1: the window.  A tap that does not count adds + 0, which changes no bit of a sum that started at + 0.
      float n = 0.0f, s1x = 0.0f, s1y = 0.0f, s1z = 0.0f, s2x = 0.0f, s2y = 0.0f, s2z = 0.0f;
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
          const int k = kc + dy * kGW + dx;
          const float4 cq = s_cv[k], nq = s_n[k];
          const bool counts = (dx == 0 && dy == 0) || (td_hit(nq) && (np.x * nq.x + np.y * nq.y) + np.z * nq.z >= A.cos_min);
          n += counts ? 1.0f : 0.0f;
          s1x += counts ? cq.x : 0.0f; s1y += counts ? cq.y : 0.0f; s1z += counts ? cq.z : 0.0f;
          s2x += counts ? cq.x * cq.x : 0.0f; s2y += counts ? cq.y * cq.y : 0.0f; s2z += counts ? cq.z * cq.z : 0.0f;
        }
      if constexpr (!NOISE) {  // (the parent's statements as they were, so that k_temporal_response keeps its instruction stream; the other branch repeats the box for step 4b)
        if (n >= 2.0f) {  // (3: a window of the pixel alone clips nothing)
          // 2: the box; 4: the clip.  fmaxf and fminf drop a NaN operand.
          const float mx = s1x / n, my = s1y / n, mz = s1z / n;
          const float gx = gamma * fhe_sqrt(fmaxf(s2x / n - mx * mx, 0.0f)), gy = gamma * fhe_sqrt(fmaxf(s2y / n - my * my, 0.0f)), gz = gamma * fhe_sqrt(fmaxf(s2z / n - mz * mz, 0.0f));
          const float ccx = fminf(fmaxf(hx, mx - gx), mx + gx), ccy = fminf(fmaxf(hy, my - gy), my + gy), ccz = fminf(fmaxf(hz, mz - gz), mz + gz);
          const float ux = fabsf(ccx - hx) / (gx + 1e-6f), uy = fabsf(ccy - hy) / (gy + 1e-6f), uz = fabsf(ccz - hz) / (gz + 1e-6f);
          const float k1 = 1.0f + fmaxf(fmaxf(ux, uy), uz);
          // 5: the shortened history
          hx = ccx; hy = ccy; hz = ccz;
          hh = hh / k1; hv = hv * k1;
        }
      } else {
        float u = 0.0f;
        if (n >= 2.0f) {  // (the same box and clip; the history is shortened after step 4b)
          const float mx = s1x / n, my = s1y / n, mz = s1z / n;
          const float gx = gamma * fhe_sqrt(fmaxf(s2x / n - mx * mx, 0.0f)), gy = gamma * fhe_sqrt(fmaxf(s2y / n - my * my, 0.0f)), gz = gamma * fhe_sqrt(fmaxf(s2z / n - mz * mz, 0.0f));
          const float ccx = fminf(fmaxf(hx, mx - gx), mx + gx), ccy = fminf(fmaxf(hy, my - gy), my + gy), ccz = fminf(fmaxf(hz, mz - gz), mz + gz);
          const float ux = fabsf(ccx - hx) / (gx + 1e-6f), uy = fabsf(ccy - hy) / (gy + 1e-6f), uz = fabsf(ccz - hz) / (gz + 1e-6f);
          u = fmaxf(fmaxf(ux, uy), uz);
          hx = ccx; hy = ccy; hz = ccz;
        }
        // 4b: the noise box around the pixel's own colour, also where step 3 left the history alone; v_h as looked up.  A NaN s drops out of every fmaxf and fminf.
        const float s = kappa * fhe_sqrt(v + hv);
        const float dx = fminf(fmaxf(hx, cx - s), cx + s), dy = fminf(fmaxf(hy, cy - s), cy + s), dz = fminf(fmaxf(hz, cz - s), cz + s);
        const float wx = fabsf(dx - hx) / (s + 1e-6f), wy = fabsf(dy - hy) / (s + 1e-6f), wz = fabsf(dz - hz) / (s + 1e-6f);
        const float k1 = 1.0f + fmaxf(u, fmaxf(fmaxf(wx, wy), wz));
        // 5: the shortened history
        hx = dx; hy = dy; hz = dz;
        hh = hh / k1; hv = hv * k1;
      }
      hist = fminf(hh + 1.0f, A.max_history);
      const float a = fmaxf(1.0f / hist, A.alpha_min), b = 1.0f - a;
      cx = b * hx + a * cx; cy = b * hy + a * cy; cz = b * hz + a * cz;
      v = (b * b) * hv + (a * a) * v;
    }
  }
  A.o_cv[p] = make_float4(cx, cy, cz, v);
  A.o_ph[p] = make_float4(pp.x, pp.y, pp.z, hist);
  A.o_n[p] = np;
  A.vplane[p] = v;
