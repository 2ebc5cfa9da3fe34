// kernels_bounces.hip -- the bounce pass (rene_bounces, rene_bounces_samples; specified in include/rene_hip.h): per pixel the WHOLE path estimator over a
// range of frames, replayed from the job's own seeds without accumulation, its radiance split by the iteration that added it -- ten buckets, the
// last one for every iteration from 9 on -- with the paths' lengths beside it, and an optional cap on the iterations.
//
// A per-pixel frame-range pass: pixel_pass.h states what the family shares.  Here a lane's frame is the path integrator's complete loop
// (lib.rs:141-357) in the form of render_kernel's bounce without the emitter fusion and without the frame-stream table (device_code.inc), written
// with the device functions the direct-light pass uses.  It has no work items, no trims and no tables in LDS: a plain second statement of the
// estimator, whose total can be held against what the render kernels make of the same seeds.
//
// The wave stays converged through EVERY query, as in the direct-light pass: the loop over the iterations runs while ANY lane of the wave has a
// live path (a ballot), so the iteration i, the bucket min(i, 9), the loop over the lights and the branch on emit_object_len are wave-uniform and
// no trace_accel call stands inside a lane-divergent branch.  A lane that has nothing to ask -- a slot outside the image, an ended path, a miss,
// a bounce without the mixture -- runs the query along the last ray it did trace with tmax = -1: nothing accepts a parameter t >= tmin > tmax,
// and the verdict is discarded.  The loop leaves when the ballot is empty: a wave whose 64 paths have ended does not walk to the cap.
//
// Where the sums live.  A sample adds to one bucket at a time, and the bucket only moves forward, so the sample's own ten values need three
// registers: `cur`, handed to the sink when the iteration is over (iterations 0 .. 8) or when the sample is (bucket 9).  The probe's sink stores
// the piece; the pass's sink adds it to the pixel's 40 bucket words, which live in an LDS column [word][lane] -- static, 40 x BLOCK x 4 bytes,
// indexed by the wave-uniform bucket at no cost, conflict-free, private to the lane (no barrier) -- and not in registers, where they would sit
// on top of the five-lobe BSDF's.  The tail's four words stay in registers.  A bucket the wave never reaches is not added to: x + (+0) is x
// for every x a sum can hold (a sum starts at +0 and +0 + -0 is +0, so no sum is ever -0), which is what tests/bounces_reference.py adds.
#include "primary_ray.h"
#include "device_code.inc"  // opens namespace rene
#include "pixel_pass.h"

// The BSDF's two forms, chosen where kernel_select.h chooses MAXL: the general one (every lobe kind, five lobes, textures, a background: 64 bytes of
// scratch per lane, as in bsdf_eval_kernel) and the Matte kernels' one lobe, which needs none
template <bool MATTE>
struct BouncesForm {
  static constexpr uint32_t FEAT = MATTE ? shade_feat(ShadeClass::Matte) : FEAT_ALL;
  static constexpr uint32_t KINDS = lobe_kinds(FEAT);  // 0: Matte only
  static constexpr int MAXL = shade_maxl(MATTE ? ShadeClass::Matte : ShadeClass::Multi);
};

constexpr uint32_t BOUNCES_BUCKETS = 10u, BOUNCES_LAST = BOUNCES_BUCKETS - 1u;
constexpr uint32_t BOUNCES_PIECES = BOUNCES_BUCKETS + 1u;  // 16-byte pieces of either record

// main_miss, lib.rs:120-139, of a ray that left the scene along rd (a Matte-only scene has no background)
template <bool MATTE>
RENE_DEV f3 bounces_miss_colour(const SceneView& S, bool background, f3 rd) {
  if (MATTE || !background) return splat(0.0f);
  const uv2 uv = sphere_uv(normalize(m4_vector(S.uni->bg_matrix, rd)));
  return mk3(S.uni->bg_color[0], S.uni->bg_color[1], S.uni->bg_color[2]) * background_tex<BouncesForm<MATTE>::FEAT>(S, uv);
}

// what a sample leaves beside its buckets
struct BouncesEnd {
  uint32_t length, end;
};

// One sample.  Every lane of the wave calls this, whatever its pixel (`live`: the slot is inside the image; else the lane asks nothing).
// sink(b, v, reached) receives bucket b's value and count once per bucket the wave got to, b wave-uniform and ascending.
template <bool SMALL, bool MATTE, class Sink>
RENE_DEV BouncesEnd bounces_sample(const SceneView& S, bool background, uint32_t max_depth, bool live, uint32_t px, uint32_t py, uint32_t W, uint32_t H,
                                   uint32_t seed, uint32_t* stack, Sink&& sink) {
  constexpr uint32_t ALL = BouncesForm<MATTE>::FEAT, KINDS = BouncesForm<MATTE>::KINDS;
  constexpr int MAXL = BouncesForm<MATTE>::MAXL;
  const float tmin = 0.001f, tmax = 100000.0f;  // lib.rs:182-183
  Pcg rng;  // the pixel's generator, behind the two jitter draws
  const PrimaryRay r = primary_ray(S.uni, px, py, W, H, seed, rng);
  Pcg fw = pcg_new(seed);  // Q3: the frame-wide stream
  LaneCounters lc;
  f3 color = splat(1.0f), ro = r.o, rd = r.d;  // (ro, rd): the last ray the lane traced or is about to
  f3 cur = splat(0.0f);                        // the sample's value for the bucket the wave is at
  uint32_t cur_reached = 0u, i = 0u;
  bool alive = live;
  BouncesEnd q{0u, RENE_BOUNCES_END_MISS};
  const bool emitters = S.emit_object_len > 0;  // wave-uniform

  while (__ballot(alive) != 0ull) {  // lib.rs:192-357; i is wave-uniform
    if (alive) cur_reached++, q.length++;
    const HitRec h = trace_accel<SMALL, false, true, false>(S.main, S.spheres, ro, rd, tmin, alive ? tmax : -1.0f, stack, lc);
    const bool hit = alive && h.slot != 0xffffffffu;
    if (alive && !hit) {  // main_miss, lib.rs:209-211
      cur = cur + color * bounces_miss_colour<MATTE>(S, background, rd);
      alive = false, q.end = RENE_BOUNCES_END_MISS;
    }

    // ---- the surface, its BSDF and its emission, lib.rs:212-227 ----------------------------------------------------------------------------------
    f3 position = ro, normal = splat(0.0f), wo = splat(0.0f);
    Bsdf<MAXL> bsdf;
    bsdf.len = 0;
    bsdf.codes = 0xffffffffu;
    bsdf.ng = splat(0.0f);
    if (hit) {
      const Surface sf = shade_hit<true>(S, h, ro, rd);
      const Inst& inst = S.insts[sf.instance];
      wo = -normalize(rd);
      normal = normalize(sf.normal);
      position = sf.position;
      bsdf.ng = normal;
      bsdf.onb = onb_from_w(normal);
      compute_bsdf<ALL, MAXL>(S, inst, sf.uv, bsdf);
      if (inst.emit[3] != 0.0f) {  // lib.rs:225-227, area_light.rs:66-74
        const f3 e = dot(wo, normal) > 0.0f ? mk3(inst.emit[0], inst.emit[1], inst.emit[2]) : splat(0.0f);
        cur = cur + color * e;
      }
    }

    // ---- the distant lights, lib.rs:234-272 (a wave-uniform loop; a lane without a hit asks nothing) -------------------------------------------
    for (uint32_t li = 0; li < S.lights_len; ++li) {
      const float4 ld = ldg4(S.lights[li].dir), lL = ldg4(S.lights[li].L);
      const f3 target = position + mk3(ld.x, ld.y, ld.z);  // light.rs:52-55
      const f3 wi = normalize(target - position);
      const HitRec sh = trace_accel<SMALL, true, true, false>(S.main, S.spheres, position, hit ? wi : rd, tmin, hit ? 1e5f : -1.0f, stack, lc);
      if (hit && sh.slot == 0xffffffffu) {
        const f3 f = bsdf_f<MAXL, KINDS>(bsdf, wo, wi);
        cur = cur + color * f * fabsf(dot(wi, normal)) * mk3(lL.x, lL.y, lL.z);
      }
    }

    // ---- the mixture or the plain sample, lib.rs:274-337 ------------------------------------------------------------------------------------------
    const bool mix = hit && emitters && bsdf_contains<MAXL, KINDS>(bsdf, K_DIFFUSE);
    f3 f = splat(0.0f), wi = rd;
    float pdf = 0.0f;
    if (mix) {
      if (pcg_f32(fw) > 0.5f) {
        const uint32_t obj = umod(pcg_u32(fw), S.emit_object_len);
        wi = normalize(emit_sample<true>(S, obj, fw) - position);
        pdf = bsdf_pdf<MAXL, KINDS>(bsdf, wi, normal);  // Q1: (wi, normal), lib.rs:287
        f = bsdf_f<MAXL, KINDS>(bsdf, wo, wi);
      } else {
        const Sampled s = bsdf_sample<MAXL, KINDS>(bsdf, wo, rng);
        wi = s.wi;
        pdf = s.pdf;
        f = s.f;
      }
    } else if (hit) {  // lib.rs:325-337
      const Sampled s = bsdf_sample<MAXL, KINDS>(bsdf, wo, rng);
      if (s.pdf < 1e-5f) {
        alive = false, q.end = RENE_BOUNCES_END_PDF;
      } else {
        color = color * (s.f * qdiv(fabsf(dot(normal, s.wi)), s.pdf));
        wi = s.wi;
      }
    }
    if (emitters) {  // Q5: the closest-hit query of the emitter structure; a lane without the mixture asks nothing
      const HitRec eh = trace_accel<SMALL, false, true, false>(S.emit, S.spheres, position, mix ? wi : rd, tmin, mix ? tmax : -1.0f, stack, lc);
      if (mix) {
        const float pdf_l = emitter_pdf<true>(S, eh, position, wi);
        color = color * (f * fabsf(dot(normal, wi)));
        pdf = 0.5f * pdf + qdiv(0.5f * pdf_l, (float)S.emit_object_len);
        if (pdf < 1e-5f) alive = false, q.end = RENE_BOUNCES_END_PDF;
        else color = color / pdf;
      }
    }
    if (alive && is_zero(color)) alive = false, q.end = RENE_BOUNCES_END_ZERO;  // lib.rs:340-342
    if (alive && i > 12u) {                                                     // lib.rs:345-354
      const float coin = pcg_f32(fw), continue_p = max_element(color);
      if (coin > continue_p) alive = false, q.end = RENE_BOUNCES_END_ROULETTE;
      else color = color / continue_p;
    }
    if (alive) ro = position, rd = wi;  // (an ended lane keeps a ray that was traced: finite, whatever the failed sample left in wi)

    if (i < BOUNCES_LAST) {  // the wave leaves bucket i
      sink(i, cur, cur_reached);
      cur = splat(0.0f), cur_reached = 0u;
    }
    i++;
    if (alive && i >= max_depth) alive = false, q.end = RENE_BOUNCES_END_CAP;  // lib.rs:192 (Q7) with max_depth = 50
  }
  sink(BOUNCES_LAST, cur, cur_reached);  // (+0 and 0 where no iteration >= 9 was made)
  return q;
}

static_assert(sizeof(rene_bounces_pixel) == 16 * BOUNCES_PIECES && sizeof(rene_bounces_sample) == 16 * BOUNCES_PIECES, "the records the kernels store in 16-byte pieces");

template <bool SMALL, bool MATTE>
__global__ void __launch_bounds__(BLOCK) bounces_kernel(SceneView S, BouncesLaunch L) {
  __shared__ uint32_t s_sums[4u * BOUNCES_BUCKETS][BLOCK];  // the pixel's bucket words, a column per lane: [4 b + c] the sum's component c, [4 b + 3] reached
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  uint32_t* col = &s_sums[0][threadIdx.x];
#pragma unroll
  for (uint32_t w = 0; w < 4u * BOUNCES_BUCKETS; ++w) col[w * BLOCK] = 0u;
  uint32_t length_sum = 0u, length_max = 0u, capped = 0u;
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    const BouncesEnd q = bounces_sample<SMALL, MATTE>(S, L.background != 0u, L.max_depth, live, x, py, W, H, L.seeds[f], stack, [&](uint32_t b, f3 v, uint32_t reached) {
      uint32_t* p = col + 4u * b * BLOCK;
      p[0] = __float_as_uint(__fadd_rn(__uint_as_float(p[0]), v.x));
      p[BLOCK] = __float_as_uint(__fadd_rn(__uint_as_float(p[BLOCK]), v.y));
      p[2 * BLOCK] = __float_as_uint(__fadd_rn(__uint_as_float(p[2 * BLOCK]), v.z));
      p[3 * BLOCK] += reached;
    });
    length_sum += q.length;
    length_max = max(length_max, q.length);
    capped += q.end == RENE_BOUNCES_END_CAP ? 1u : 0u;
  }
  if (!live) return;
  uint4* dst = reinterpret_cast<uint4*>(L.dst) + ((size_t)yi * W + x) * BOUNCES_PIECES;
#pragma unroll
  for (uint32_t b = 0; b < BOUNCES_BUCKETS; ++b) {
    const uint32_t* p = col + 4u * b * BLOCK;
    dst[b] = make_uint4(p[0], p[BLOCK], p[2 * BLOCK], p[3 * BLOCK]);
  }
  dst[BOUNCES_BUCKETS] = make_uint4(L.n_frames, length_sum, length_max, capped);
}

// the per-sample probe: the same device function, every sample's rene_bounces_sample into [n_frames][H][W]
template <bool SMALL, bool MATTE>
__global__ void __launch_bounds__(BLOCK) bounces_samples_kernel(SceneView S, BouncesLaunch L) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    uint4* dst = reinterpret_cast<uint4*>(L.dst) + (((size_t)f * H + yi) * W + x) * BOUNCES_PIECES;
    const BouncesEnd q = bounces_sample<SMALL, MATTE>(S, L.background != 0u, L.max_depth, live, x, py, W, H, L.seeds[f], stack, [&](uint32_t b, f3 v, uint32_t reached) {
      if (live) dst[b] = make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), reached);
    });
    if (live) dst[BOUNCES_BUCKETS] = make_uint4(1u, q.length, q.end, 0u);
  }
}

hipError_t launch_bounces(const LaunchConfig& cfg, const SceneView& S, const BouncesLaunch& L, bool samples, hipStream_t st) {
  const bool matte = shade_class(cfg.features) == ShadeClass::Matte;  // (kernel_select.h: where the render launchers choose one lobe over five)
  if (samples)
    return launch_pixel_pass(cfg, S, L, matte ? bounces_samples_kernel<true, true> : bounces_samples_kernel<true, false>,
                             matte ? bounces_samples_kernel<false, true> : bounces_samples_kernel<false, false>, st);
  return launch_pixel_pass(cfg, S, L, matte ? bounces_kernel<true, true> : bounces_kernel<true, false>,
                           matte ? bounces_kernel<false, true> : bounces_kernel<false, false>, st);
}

}  // namespace rene
