// kernels_gbuffer.hip -- the geometry pass (rene_gbuffer, rene_primary_hits; specified in include/rene_hip.h): per pixel the first hit of the
// primary rays of a range of frames -- depth, world position, coverage and four id slots -- without shading, bounces or accumulation.
//
// A per-pixel frame-range pass: pixel_pass.h states what the family shares -- one lane per pixel slot of an owned tile (chain_pass.h's slot_pixel
// and owned_tile_origin in item_slot.h's spelling: chain_pass.h and device_code.inc each define a wave_sum and cannot share a unit), the clamped
// dead lane, the zeroed destination, the launch.  Here a lane's frame is the primary ray (primary_ray.h, the render kernels' ray generation
// restated) and the closest-hit query of lib.rs:195-207 in the instantiation and with the tmin / tmax of rene_trace and the render kernels.  The
// aggregates stay in registers; the finished 64-byte record leaves in four 16-byte stores.  The sample's position is o + t d as a rounded
// multiply and a rounded add (never fused), the sums are plain fp32 sums in frame order: tests/gbuffer_reference.py restates them bit for bit.
#include "primary_ray.h"
#include "device_code.inc"  // opens namespace rene
#include "pixel_pass.h"

// one sample: the primary ray of (px, py) under `seed` and its closest hit in the main structure (t = -1: a miss)
struct PrimarySample {
  f3 o, d;
  float t, u, v;
  uint32_t instance, primitive;
};
template <bool SMALL>
RENE_DEV PrimarySample primary_sample(const SceneView& S, uint32_t px, uint32_t py, uint32_t W, uint32_t H, uint32_t seed, uint32_t* stack) {
  const PrimaryRay r = primary_ray(S.uni, px, py, W, H, seed);
  LaneCounters lc;
  const HitRec h = trace_accel<SMALL, false, true, false>(S.main, S.spheres, r.o, r.d, 0.001f, 100000.0f, stack, lc);  // lib.rs:182-183
  PrimarySample s{r.o, r.d, -1.0f, 0.0f, 0.0f, 0u, 0u};
  if (h.slot != 0xffffffffu) {
    const float* q = S.main.isect[h.slot].q;
    s.t = h.t, s.u = h.u, s.v = h.v;
    s.instance = __float_as_uint(q[9]);
    s.primitive = __float_as_uint(q[10]);
  }
  return s;
}

template <bool SMALL>
__global__ void __launch_bounds__(BLOCK) gbuffer_kernel(SceneView S, GbufferLaunch L) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  float depth_sum = 0.0f, depth_min = __builtin_inff();
  f3 pos = splat(0.0f);
  uint32_t hits = 0u, other = 0u, id[4], cnt[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) id[k] = 0xffffffffu, cnt[k] = 0u;
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    const PrimarySample s = primary_sample<SMALL>(S, x, py, W, H, L.seeds[f], stack);
    if (s.t < 0.0f) continue;
    hits++;
    depth_sum += s.t;
    depth_min = fminf(depth_min, s.t);
    pos.x += __fadd_rn(s.o.x, __fmul_rn(s.t, s.d.x));
    pos.y += __fadd_rn(s.o.y, __fmul_rn(s.t, s.d.y));
    pos.z += __fadd_rn(s.o.z, __fmul_rn(s.t, s.d.z));
    uint32_t sid = s.instance;
    if (L.id_source == RENE_GBUFFER_ID_MATERIAL) sid = S.insts[s.instance].material;
    else if (L.id_source == RENE_GBUFFER_ID_PRIMITIVE) sid = s.primitive;
    // the streaming rule: the id's slot, else the lowest free slot, else `other` (the slots fill from 0 up: a free one has count 0)
    bool placed = false;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (!placed && cnt[k] != 0u && id[k] == sid) cnt[k]++, placed = true;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (!placed && cnt[k] == 0u) id[k] = sid, cnt[k] = 1u, placed = true;
    if (!placed) other++;
  }
  if (!live) return;
  // count descending, ties by id ascending: a five-comparator network (an unused slot, count 0 and id ~0, sorts last)
  auto order = [&](int a, int b) {
    if (cnt[b] > cnt[a] || (cnt[b] == cnt[a] && id[b] < id[a])) {
      const uint32_t ti = id[a], tc = cnt[a];
      id[a] = id[b], cnt[a] = cnt[b], id[b] = ti, cnt[b] = tc;
    }
  };
  order(0, 1), order(2, 3), order(0, 2), order(1, 3), order(1, 2);
  uint4* dst = reinterpret_cast<uint4*>(L.dst) + ((size_t)yi * W + x) * 4u;
  dst[0] = make_uint4(__float_as_uint(depth_sum), __float_as_uint(depth_min), hits, L.n_frames);
  dst[1] = make_uint4(__float_as_uint(pos.x), __float_as_uint(pos.y), __float_as_uint(pos.z), other);
  dst[2] = make_uint4(id[0], id[1], id[2], id[3]);
  dst[3] = make_uint4(cnt[0], cnt[1], cnt[2], cnt[3]);
}

// the per-sample probe: the same sample function, every frame's rene_primary_hit of the pixel into [n_frames][H][W]
template <bool SMALL>
__global__ void __launch_bounds__(BLOCK) primary_hits_kernel(SceneView S, GbufferLaunch L) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    const PrimarySample s = primary_sample<SMALL>(S, x, py, W, H, L.seeds[f], stack);
    if (!live) continue;
    uint4* dst = reinterpret_cast<uint4*>(L.dst) + (((size_t)f * H + yi) * W + x) * 2u;
    dst[0] = make_uint4(__float_as_uint(s.d.x), __float_as_uint(s.d.y), __float_as_uint(s.d.z), __float_as_uint(s.t));
    dst[1] = make_uint4(__float_as_uint(s.u), __float_as_uint(s.v), s.instance, s.primitive);
  }
}

static_assert(sizeof(rene_gbuffer_pixel) == 64 && sizeof(rene_primary_hit) == 32, "the records the kernels store in 16-byte pieces");

hipError_t launch_gbuffer(const LaunchConfig& cfg, const SceneView& S, const GbufferLaunch& L, bool samples, hipStream_t st) {
  if (samples) return launch_pixel_pass(cfg, S, L, primary_hits_kernel<true>, primary_hits_kernel<false>, st);
  return launch_pixel_pass(cfg, S, L, gbuffer_kernel<true>, gbuffer_kernel<false>, st);
}

}  // namespace rene
