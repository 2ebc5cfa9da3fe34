// primary_ray.h -- the primary ray of a pixel and frame, lib.rs:174-189, as a function: the ray generation of the render kernels (device_code.inc,
// "ray generation") restated operation for operation -- the pixel's generator PCG32si::new((py * W + px) ^ seed), two pcg_f32 draws, the jittered
// film position divided by W - 1 / H - 1 through qdiv (quirk Q2), the camera origin read off camera_to_world, the film point through proj_inv
// and camera_to_world (camera.rs:77-90), normalize.  (px, py) is the launch id: py counts the image's rows from the BOTTOM, py = H - 1 - row.
// The render kernels keep their own text; the per-pixel frame-range passes (pixel_pass.h: kernels_gbuffer.hip, kernels_occlusion.hip,
// kernels_direct.hip) call this, and the two that go on sampling take the pixel's generator from it.
#pragma once
#include "device_math.h"

namespace rene {

struct PrimaryRay {
  f3 o, d;
};

// `rng` leaves as the pixel's generator behind the two jitter draws: what a pass that goes on sampling draws from next
RENE_DEV PrimaryRay primary_ray(const Uniforms* uni, uint32_t px, uint32_t py, uint32_t W, uint32_t H, uint32_t seed, Pcg& rng) {
  rng = pcg_new((py * W + px) ^ seed);
  float u = qdiv((float)px + pcg_f32(rng), (float)(W - 1));  // Q2
  float v = qdiv((float)py + pcg_f32(rng), (float)(H - 1));
  cfloat_ptr cam = (cfloat_ptr)(const void*)uni;  // c2w[16], proj_inv[16]
  f3 origin = camera_origin(cam);
  f3 target = m4_point(cam + 16, mk3(u * 2.0f - 1.0f, v * 2.0f - 1.0f, 1.0f));  // camera.rs:77-90
  target = m4_point(cam, target);
  return PrimaryRay{origin, normalize(target - origin)};
}
RENE_DEV PrimaryRay primary_ray(const Uniforms* uni, uint32_t px, uint32_t py, uint32_t W, uint32_t H, uint32_t seed) {
  Pcg rng;
  return primary_ray(uni, px, py, W, H, seed, rng);
}

}  // namespace rene
