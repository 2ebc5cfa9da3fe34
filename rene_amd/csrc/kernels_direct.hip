// kernels_direct.hip -- the direct-light pass (rene_direct, rene_direct_samples; specified in include/rene_hip.h): per pixel the path estimator's
// first two steps over a range of frames -- all of iteration 0 (what the primary ray sees, the distant lights, the light / BSDF mixture ray) and
// iteration 1's closest-hit query with its one emission-or-background add -- replayed from the job's own seeds, without accumulation.
//
// A per-pixel frame-range pass: pixel_pass.h states what the family shares -- the slot -> pixel map, the clamped dead lane, the zeroed destination,
// the launch.  Here a lane's frame is the primary ray (primary_ray.h, which hands out the pixel's generator behind the two jitter draws) and its
// closest hit in the instantiation and with the tmin / tmax of the geometry pass, shade_hit, the BSDF (compute_bsdf in one of the two forms
// below), and the statements of render_kernel's bounce (device_code.inc, lib.rs:225-342) with a throughput of one.
//
// The wave stays converged through EVERY query: the small-scene item loop fetches its items by a wave-uniform index (traverse_small), so no
// trace_accel call stands inside a lane-divergent branch -- the primary query, the lights_len shadow queries, the emitter-structure query and the
// second main query.  The loop over the lights and the branch on emit_object_len are wave-uniform.  A lane that has nothing to ask -- a slot
// outside the image (clamped to a pixel inside it), a primary miss, an ended sample, a sample without the mixture -- runs the query along its
// primary ray with tmax = -1: no item, node or primitive accepts a parameter t >= tmin > tmax, the BVH form leaves at the root, and the verdict
// is discarded.  On a BVH scene the LDS stack column [depth][lane] serves the queries one after the other (each starts at depth 0).  The sums
// stay in registers; the 48-byte record leaves in three 16-byte stores.
// Every sum is a plain fp32 add per component in frame order: tests/direct_reference.py restates them from the probe's samples bit for bit.
#include "primary_ray.h"
#include "device_code.inc"  // opens namespace rene
#include "pixel_pass.h"

// The BSDF comes in two forms, chosen where kernel_select.h chooses MAXL: the general one -- every lobe kind, five lobes, textures, a background:
// compute_bsdf<FEAT_ALL, 5> as bsdf_eval_kernel instantiates it, which needs 64 bytes of scratch per lane -- and, for a scene whose pack reports
// Matte only (ShadeClass::Matte: Cornell, dragon-class), the Matte kernels' FEAT_LIGHTS with one lobe, which needs none.
template <bool MATTE>
struct DirectForm {
  static constexpr uint32_t FEAT = MATTE ? shade_feat(ShadeClass::Matte) : FEAT_ALL;
  static constexpr uint32_t KINDS = lobe_kinds(FEAT);  // 0: Matte only
  static constexpr int MAXL = shade_maxl(MATTE ? ShadeClass::Matte : ShadeClass::Multi);
};

// main_miss, lib.rs:120-139, of a ray that left the scene along rd (a Matte-only scene has no background)
template <bool MATTE>
RENE_DEV f3 direct_miss_colour(const SceneView& S, bool background, f3 rd) {
  if (MATTE || !background) return splat(0.0f);
  const uv2 uv = sphere_uv(normalize(m4_vector(S.uni->bg_matrix, rd)));
  return mk3(S.uni->bg_color[0], S.uni->bg_color[1], S.uni->bg_color[2]) * background_tex<DirectForm<MATTE>::FEAT>(S, uv);
}

// one sample of the pass: what rene_direct_sample holds, and whether the primary ray hit
struct DirectSample {
  f3 seen, distant, sampled, wi;
  float pdf;
  uint32_t state, second;
  bool hit;
};

// Every lane of the wave calls this, whatever its pixel: see the head of the file
template <bool SMALL, bool MATTE>
RENE_DEV DirectSample direct_sample(const SceneView& S, bool background, uint32_t px, uint32_t py, uint32_t W, uint32_t H, uint32_t seed, uint32_t* stack) {
  constexpr uint32_t DIRECT_ALL = DirectForm<MATTE>::FEAT, DIRECT_KINDS = DirectForm<MATTE>::KINDS;
  constexpr int DIRECT_MAXL = DirectForm<MATTE>::MAXL;
  const float tmin = 0.001f, tmax = 100000.0f;  // lib.rs:182-183
  DirectSample q;
  q.seen = splat(0.0f), q.distant = splat(0.0f), q.sampled = splat(0.0f), q.wi = splat(0.0f);
  q.pdf = 0.0f;
  q.state = RENE_DIRECT_MISS, q.second = RENE_DIRECT_SECOND_NONE;
  Pcg rng;  // the pixel's generator, behind the two jitter draws
  const PrimaryRay r = primary_ray(S.uni, px, py, W, H, seed, rng);
  Pcg fw = pcg_new(seed);  // Q3: the frame-wide stream
  LaneCounters lc;
  const HitRec h = trace_accel<SMALL, false, true, false>(S.main, S.spheres, r.o, r.d, tmin, tmax, stack, lc);
  q.hit = h.slot != 0xffffffffu;

  // ---- iteration 0, lib.rs:209-232: the miss colour, or the surface, its BSDF and its emission -------------------------------------------------
  f3 position = r.o, normal = splat(0.0f), wo = splat(0.0f);
  Bsdf<DIRECT_MAXL> bsdf;
  bsdf.len = 0;
  bsdf.codes = 0xffffffffu;
  bsdf.ng = splat(0.0f);
  if (!q.hit) {
    q.seen = direct_miss_colour<MATTE>(S, background, r.d);
  } else {
    const Surface sf = shade_hit<true>(S, h, r.o, r.d);
    const Inst& inst = S.insts[sf.instance];
    wo = -normalize(r.d);
    normal = normalize(sf.normal);
    position = sf.position;
    bsdf.ng = normal;
    bsdf.onb = onb_from_w(normal);
    compute_bsdf<DIRECT_ALL, DIRECT_MAXL>(S, inst, sf.uv, bsdf);
    if (inst.emit[3] != 0.0f)  // lib.rs:225-227, area_light.rs:66-74
      q.seen = dot(wo, normal) > 0.0f ? mk3(inst.emit[0], inst.emit[1], inst.emit[2]) : splat(0.0f);
  }

  // ---- the distant lights, lib.rs:234-272 (a wave-uniform loop; a lane without a hit asks nothing) -------------------------------------------
  for (uint32_t li = 0; li < S.lights_len; ++li) {
    const float4 ld = ldg4(S.lights[li].dir), lL = ldg4(S.lights[li].L);
    const f3 target = position + mk3(ld.x, ld.y, ld.z);  // light.rs:52-55
    const f3 wi = normalize(target - position);
    const HitRec sh = trace_accel<SMALL, true, true, false>(S.main, S.spheres, position, q.hit ? wi : r.d, tmin, q.hit ? 1e5f : -1.0f, stack, lc);
    if (q.hit && sh.slot == 0xffffffffu) {
      const f3 f = bsdf_f<DIRECT_MAXL, DIRECT_KINDS>(bsdf, wo, wi);
      q.distant = q.distant + f * fabsf(dot(wi, normal)) * mk3(lL.x, lL.y, lL.z);
    }
  }

  // ---- the mixture, lib.rs:274-337 --------------------------------------------------------------------------------------------------------------
  const bool emitters = S.emit_object_len > 0;  // wave-uniform
  const bool mix = q.hit && emitters && bsdf_contains<DIRECT_MAXL, DIRECT_KINDS>(bsdf, K_DIFFUSE);
  bool alive = q.hit;
  f3 T = splat(0.0f), f = splat(0.0f), wi = r.d;
  float pdf = 0.0f;
  if (mix) {
    if (pcg_f32(fw) > 0.5f) {
      const uint32_t obj = umod(pcg_u32(fw), S.emit_object_len);
      wi = normalize(emit_sample<true>(S, obj, fw) - position);
      pdf = bsdf_pdf<DIRECT_MAXL, DIRECT_KINDS>(bsdf, wi, normal);  // Q1: (wi, normal), lib.rs:287
      f = bsdf_f<DIRECT_MAXL, DIRECT_KINDS>(bsdf, wo, wi);
      q.state = RENE_DIRECT_LIGHT;
    } else {
      const Sampled s = bsdf_sample<DIRECT_MAXL, DIRECT_KINDS>(bsdf, wo, rng);
      wi = s.wi;
      pdf = s.pdf;
      f = s.f;
      q.state = RENE_DIRECT_BSDF;
    }
  } else if (q.hit) {  // lib.rs:325-337
    const Sampled s = bsdf_sample<DIRECT_MAXL, DIRECT_KINDS>(bsdf, wo, rng);
    wi = s.wi;
    pdf = s.pdf;
    q.state = RENE_DIRECT_PLAIN;
    if (s.pdf < 1e-5f) alive = false, q.state = RENE_DIRECT_ENDED_PDF;
    else T = s.f * qdiv(fabsf(dot(normal, s.wi)), s.pdf);
  }
  if (emitters) {  // Q5: the closest-hit query of the emitter structure; a lane without the mixture asks nothing
    const HitRec eh = trace_accel<SMALL, false, true, false>(S.emit, S.spheres, mix ? position : r.o, mix ? wi : r.d, tmin, mix ? tmax : -1.0f, stack, lc);
    if (mix) {
      const float pdf_l = emitter_pdf<true>(S, eh, position, wi);
      T = f * fabsf(dot(normal, wi));
      pdf = 0.5f * pdf + qdiv(0.5f * pdf_l, (float)S.emit_object_len);
      if (pdf < 1e-5f) alive = false, q.state = RENE_DIRECT_ENDED_PDF;
      else T = T / pdf;
    }
  }
  if (alive && is_zero(T)) alive = false, q.state = RENE_DIRECT_ENDED_ZERO;  // lib.rs:340-342
  if (q.hit) q.wi = wi, q.pdf = pdf;

  // ---- iteration 1, lib.rs:209-227: the closest hit of the mixture ray and its one add ----------------------------------------------------------
  const HitRec h2 = trace_accel<SMALL, false, true, false>(S.main, S.spheres, alive ? position : r.o, alive ? wi : r.d, tmin, alive ? tmax : -1.0f, stack, lc);
  if (alive) {
    if (h2.slot == 0xffffffffu) {
      q.second = RENE_DIRECT_SECOND_MISS;
      q.sampled = T * direct_miss_colour<MATTE>(S, background, wi);
    } else {
      const Surface sf = shade_hit<true>(S, h2, position, wi);
      const Inst& inst = S.insts[sf.instance];
      q.second = RENE_DIRECT_SECOND_SURFACE;
      if (inst.emit[3] != 0.0f) {
        const f3 e = dot(-normalize(wi), normalize(sf.normal)) > 0.0f ? mk3(inst.emit[0], inst.emit[1], inst.emit[2]) : splat(0.0f);
        q.second = RENE_DIRECT_SECOND_EMITTER;
        q.sampled = T * e;
      }
    }
  }
  return q;
}

RENE_DEV f3 direct_add(f3 a, f3 b) { return mk3(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z)); }

template <bool SMALL, bool MATTE>
__global__ void __launch_bounds__(BLOCK) direct_kernel(SceneView S, DirectLaunch L) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  uint32_t hits = 0u;
  f3 seen = splat(0.0f), distant = splat(0.0f), sampled = splat(0.0f);
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    const DirectSample q = direct_sample<SMALL, MATTE>(S, L.background != 0u, x, py, W, H, L.seeds[f], stack);
    hits += q.hit ? 1u : 0u;
    seen = direct_add(seen, q.seen);
    distant = direct_add(distant, q.distant);
    sampled = direct_add(sampled, q.sampled);
  }
  if (!live) return;
  uint4* dst = reinterpret_cast<uint4*>(L.dst) + ((size_t)yi * W + x) * 3u;
  dst[0] = make_uint4(__float_as_uint(seen.x), __float_as_uint(seen.y), __float_as_uint(seen.z), hits);
  dst[1] = make_uint4(__float_as_uint(distant.x), __float_as_uint(distant.y), __float_as_uint(distant.z), L.n_frames);
  dst[2] = make_uint4(__float_as_uint(sampled.x), __float_as_uint(sampled.y), __float_as_uint(sampled.z), 0u);
}

// the per-sample probe: the same device function, every sample's rene_direct_sample into [n_frames][H][W]
template <bool SMALL, bool MATTE>
__global__ void __launch_bounds__(BLOCK) direct_samples_kernel(SceneView S, DirectLaunch L) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    const DirectSample q = direct_sample<SMALL, MATTE>(S, L.background != 0u, x, py, W, H, L.seeds[f], stack);
    if (!live) continue;
    uint4* dst = reinterpret_cast<uint4*>(L.dst) + (((size_t)f * H + yi) * W + x) * 4u;
    dst[0] = make_uint4(__float_as_uint(q.seen.x), __float_as_uint(q.seen.y), __float_as_uint(q.seen.z), q.state);
    dst[1] = make_uint4(__float_as_uint(q.distant.x), __float_as_uint(q.distant.y), __float_as_uint(q.distant.z), __float_as_uint(q.pdf));
    dst[2] = make_uint4(__float_as_uint(q.wi.x), __float_as_uint(q.wi.y), __float_as_uint(q.wi.z), q.second);
    dst[3] = make_uint4(__float_as_uint(q.sampled.x), __float_as_uint(q.sampled.y), __float_as_uint(q.sampled.z), 0u);
  }
}

static_assert(sizeof(rene_direct_pixel) == 48 && sizeof(rene_direct_sample) == 64, "the records the kernels store in 16-byte pieces");

hipError_t launch_direct(const LaunchConfig& cfg, const SceneView& S, const DirectLaunch& L, bool samples, hipStream_t st) {
  const bool matte = shade_class(cfg.features) == ShadeClass::Matte;  // (kernel_select.h: where the render launchers choose one lobe over five)
  if (samples)
    return launch_pixel_pass(cfg, S, L, matte ? direct_samples_kernel<true, true> : direct_samples_kernel<true, false>,
                             matte ? direct_samples_kernel<false, true> : direct_samples_kernel<false, false>, st);
  return launch_pixel_pass(cfg, S, L, matte ? direct_kernel<true, true> : direct_kernel<true, false>,
                           matte ? direct_kernel<false, true> : direct_kernel<false, false>, st);
}

}  // namespace rene
