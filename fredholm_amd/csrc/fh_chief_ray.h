// fh_chief_ray.h -- the chief ray of a pixel (include/fredholm_hip.h: fh_primary_instances): render.hip's camera_ray at the pixel centre (u = 1/2, 1/2) through the
// lens centre (no lens offset), operation by operation.  One device function, so that the id kernel (motion.hip) and the known-answer hook (kat.hip:
// fh_kat_chief_rays) build the identical rays.
#pragma once
#include "fh_vec.h"

namespace fh {

struct ChiefCam {
  m34 xf;              // camera.transform
  float inv_tan, apb;  // 1 / tanf(0.5 * fov) and a + b of the thin lens (motion_host.h: chief_a_plus_b)
  uint32_t width, height;
};

FH_D void chief_ray(const ChiefCam& c, uint32_t px, uint32_t py, f3& org, f3& dir)
{
  float uvx = (2.0f * (px + 0.5f) - c.width) / c.height;
  const float uvy = (2.0f * (py + 0.5f) - c.height) / c.height;
  uvx = -uvx;
  const f3 p_sensor = mk3(uvx, uvy, 0.0f);
  const f3 p_lens = mk3(0.0f, 0.0f, c.inv_tan);
  const f3 s2c = normalize(p_lens - p_sensor);
  const f3 p_object = p_sensor + (c.apb / s2c.z) * s2c;
  org = xform_point(c.xf, p_lens);
  f3 d = normalize(p_object - p_lens);
  d.z *= -1.0f;
  dir = xform_dir(c.xf, d);
}

}  // namespace fh
