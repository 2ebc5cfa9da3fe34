// kernels_occlusion.hip -- the occlusion pass (rene_occlusion, rene_occlusion_samples; specified in include/rene_hip.h): per pixel the ambient
// occlusion and the bent-normal sum of the first hits of the primary rays of a range of frames -- without shading, bounces or accumulation.
//
// A per-pixel frame-range pass: pixel_pass.h states what the family shares -- the slot -> pixel map, the clamped dead lane, the zeroed destination,
// the launch.  Here a lane's frame is the primary ray (primary_ray.h) and its closest hit in the instantiation and with the tmin / tmax of the
// geometry pass, shade_hit's position and normal, and then `rays` times, the pixel's generator going on behind the two jitter draws (primary_ray
// hands it out): the Matte bounce's direction (random_cosine_direction through onb_from_w and to_world) and ONE any-hit query of the main
// structure up to `radius`.
//
// The wave stays converged through BOTH queries: the small-scene item loop fetches its items by a wave-uniform index (traverse_small), so neither
// query stands inside a divergent branch.  A lane that has nothing to ask -- a slot outside the image (clamped to a pixel inside it), a primary miss,
// a normal that is not finite -- runs the second query along its primary ray with tmax = -1: no item, node or primitive accepts a parameter
// t >= tmin > tmax, the BVH form leaves at the root, and the verdict is discarded.  On a BVH scene the LDS stack column [depth][lane] serves the two
// queries one after the other (each starts at depth 0).  Counts and the bent sum stay in registers; the 32-byte record leaves in two 16-byte
// stores.  The bent sum is a plain fp32 sum in frame and ray order: tests/occlusion_reference.py restates it from the probe's samples bit for bit.
#include "primary_ray.h"
#include "device_code.inc"  // opens namespace rene
#include "pixel_pass.h"

// the first hit of the primary ray of (px, py) under `seed`: where the occlusion rays start, and the generator they draw from
struct OcclusionHit {
  f3 o, d;   // the primary ray
  f3 p, n;   // shade_hit's position; the unit normal facing the viewer (0 where nothing was hit)
  Pcg rng;   // the pixel's generator behind the two jitter draws
  bool hit;  // the primary ray hit something
  bool cast; // ... and its normal is finite: the sample casts rays
};
template <bool SMALL>
RENE_DEV OcclusionHit occlusion_first_hit(const SceneView& S, uint32_t px, uint32_t py, uint32_t W, uint32_t H, uint32_t seed, uint32_t* stack) {
  OcclusionHit fh;
  const PrimaryRay r = primary_ray(S.uni, px, py, W, H, seed, fh.rng);
  LaneCounters lc;
  const HitRec h = trace_accel<SMALL, false, true, false>(S.main, S.spheres, r.o, r.d, 0.001f, 100000.0f, stack, lc);  // lib.rs:182-183
  fh.o = r.o, fh.d = r.d;
  fh.p = splat(0.0f), fh.n = splat(0.0f);
  fh.hit = h.slot != 0xffffffffu;
  fh.cast = false;
  if (fh.hit) {
    const Surface sf = shade_hit<true>(S, h, r.o, r.d);
    const f3 n = normalize(sf.normal);
    fh.p = sf.position;
    fh.n = dot(sf.normal, r.d) > 0.0f ? -n : n;
    const float inf = __builtin_inff();
    fh.cast = fabsf(fh.n.x) < inf && fabsf(fh.n.y) < inf && fabsf(fh.n.z) < inf;  // (a NaN compares false)
  }
  return fh;
}

// one occlusion ray of a first hit: the next two draws of its generator, the Matte bounce's direction, the any-hit query.  Every lane of the wave
// calls this, whatever its first hit: see the head of the file
struct OcclusionRay {
  float r1, r2;
  f3 w;
  bool occluded;
};
template <bool SMALL>
RENE_DEV OcclusionRay occlusion_ray(const SceneView& S, OcclusionHit& fh, float radius, uint32_t* stack) {
  OcclusionRay q;
  Pcg peek = fh.rng;  // what random_cosine_direction is about to draw, for the probe
  q.r1 = pcg_f32(peek);
  q.r2 = pcg_f32(peek);
  const f3 local = random_cosine_direction(fh.rng);
  q.w = to_world(onb_from_w(fh.n), local);
  const f3 o = fh.cast ? fh.p : fh.o, d = fh.cast ? q.w : fh.d;
  const float tmax = fh.cast ? radius : -1.0f;
  LaneCounters lc;
  const HitRec h = trace_accel<SMALL, true, true, false>(S.main, S.spheres, o, d, 0.001f, tmax, stack, lc);
  q.occluded = fh.cast && h.slot != 0xffffffffu;
  return q;
}

template <bool SMALL>
__global__ void __launch_bounds__(BLOCK) occlusion_kernel(SceneView S, OcclusionLaunch L) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  uint32_t hits = 0u, rays = 0u, occluded = 0u;
  f3 bent = splat(0.0f);
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    OcclusionHit fh = occlusion_first_hit<SMALL>(S, x, py, W, H, L.seeds[f], stack);
    hits += fh.hit ? 1u : 0u;
    for (uint32_t k = 0; k < L.rays; ++k) {
      const OcclusionRay q = occlusion_ray<SMALL>(S, fh, L.radius, stack);
      const bool open = fh.cast && !q.occluded;
      rays += fh.cast ? 1u : 0u;
      occluded += q.occluded ? 1u : 0u;
      bent.x = __fadd_rn(bent.x, open ? q.w.x : 0.0f);  // (a sum that holds +0 or a finite value: adding +0 changes no bit of it)
      bent.y = __fadd_rn(bent.y, open ? q.w.y : 0.0f);
      bent.z = __fadd_rn(bent.z, open ? q.w.z : 0.0f);
    }
  }
  if (!live) return;
  uint4* dst = reinterpret_cast<uint4*>(L.dst) + ((size_t)yi * W + x) * 2u;
  dst[0] = make_uint4(hits, rays, occluded, L.n_frames);
  dst[1] = make_uint4(__float_as_uint(bent.x), __float_as_uint(bent.y), __float_as_uint(bent.z), 0u);
}

// the per-sample probe: the same two device functions, every ray's rene_occlusion_sample into [n_frames][rays][H][W]
template <bool SMALL>
__global__ void __launch_bounds__(BLOCK) occlusion_samples_kernel(SceneView S, OcclusionLaunch L) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    OcclusionHit fh = occlusion_first_hit<SMALL>(S, x, py, W, H, L.seeds[f], stack);
    for (uint32_t k = 0; k < L.rays; ++k) {
      const OcclusionRay q = occlusion_ray<SMALL>(S, fh, L.radius, stack);
      if (!live || !fh.hit) continue;  // (a miss: the all-zero record the host left)
      const uint32_t state = !fh.cast ? RENE_OCCLUSION_NO_RAY : (q.occluded ? RENE_OCCLUSION_OCCLUDED : RENE_OCCLUSION_OPEN);
      const float r1 = fh.cast ? q.r1 : 0.0f, r2 = fh.cast ? q.r2 : 0.0f;
      const f3 w = fh.cast ? q.w : splat(0.0f);
      uint4* dst = reinterpret_cast<uint4*>(L.dst) + ((((size_t)f * L.rays + k) * H + yi) * W + x) * 3u;
      dst[0] = make_uint4(__float_as_uint(fh.p.x), __float_as_uint(fh.p.y), __float_as_uint(fh.p.z), state);
      dst[1] = make_uint4(__float_as_uint(fh.n.x), __float_as_uint(fh.n.y), __float_as_uint(fh.n.z), __float_as_uint(r1));
      dst[2] = make_uint4(__float_as_uint(w.x), __float_as_uint(w.y), __float_as_uint(w.z), __float_as_uint(r2));
    }
  }
}

static_assert(sizeof(rene_occlusion_pixel) == 32 && sizeof(rene_occlusion_sample) == 48, "the records the kernels store in 16-byte pieces");

hipError_t launch_occlusion(const LaunchConfig& cfg, const SceneView& S, const OcclusionLaunch& L, bool samples, hipStream_t st) {
  if (L.rays == 0) return hipSuccess;
  if (samples) return launch_pixel_pass(cfg, S, L, occlusion_samples_kernel<true>, occlusion_samples_kernel<false>, st);
  return launch_pixel_pass(cfg, S, L, occlusion_kernel<true>, occlusion_kernel<false>, st);
}

}  // namespace rene
