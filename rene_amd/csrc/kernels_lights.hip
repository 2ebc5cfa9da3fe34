// kernels_lights.hip -- the light-group pass (rene_lights, rene_lights_samples; specified in include/rene_hip.h): per pixel the WHOLE path estimator over
// a range of frames, replayed from the job's own seeds without accumulation, its radiance split by the SOURCE of every add -- the background, an
// emitting instance, a distant light -- into up to eight groups that the caller's tables name.
//
// A per-pixel frame-range pass: pixel_pass.h states what the family shares.  A lane's frame is the bounce pass's: the path integrator's complete
// loop (lib.rs:141-357) in render_kernel's unfused form, written with the device functions kernels_bounces.hip uses.  The loop is restated here,
// not shared: the bounce pass contracts an add's product into its add (one rounding, into three registers that a wave-uniform sink takes per
// bucket), this pass needs every term on its own -- is it black? -- and adds it where the lane's source says; a body serving both would change
// the bounce pass's bits or its pinned registers.  The same ballot loop, the same idle queries with tmax = -1, the same order of draws: the
// wave stays converged through every query, and a lane that has nothing to ask discards the verdict.
//
// Where the sums live.  The group of an add differs from lane to lane (two lanes of a wave hit two lamps), so a sample's eight values cannot be
// indexed statically.  They live in an LDS column of the lane's own, [4 g + c][lane] -- static, 32 x BLOCK x 4 bytes: the bank is the lane's
// whatever the row, so a lane-divergent g costs no conflict, and the column is private (no barrier).  [4 g + 3] counts the adds with a non-zero
// component.  A sample's value for a group is the fp32 fold of its adds in the estimator's order from +0; the product of an add is rounded on its
// own (a statement of its own: no contraction into the add).  The PIXEL's 32 words stay in registers: when a sample ends, a statically unrolled
// loop over g adds the column to them (__fadd_rn; x + (+0) is x, and no sum is ever -0, so a group the sample left alone needs no branch).  A second
// column would make 65 536 bytes in front of the traversal stack, two workgroups per CU at the most; the registers leave the Matte forms their
// waves (has the figures).
#include "primary_ray.h"
#include "device_code.inc"  // opens namespace rene
#include "pixel_pass.h"

// The BSDF's two forms, chosen where kernel_select.h chooses MAXL: the general one (every lobe kind, five lobes, textures, a background) and the
// Matte kernels' one lobe
template <bool MATTE>
struct LightsForm {
  static constexpr uint32_t FEAT = MATTE ? shade_feat(ShadeClass::Matte) : FEAT_ALL;
  static constexpr uint32_t KINDS = lobe_kinds(FEAT);  // 0: Matte only
  static constexpr int MAXL = shade_maxl(MATTE ? ShadeClass::Matte : ShadeClass::Multi);
};

constexpr uint32_t LIGHTS_GROUPS = RENE_LIGHTS_GROUPS, LIGHTS_WORDS = 4u * LIGHTS_GROUPS;
constexpr uint32_t LIGHTS_PIECES = LIGHTS_GROUPS + 1u;  // 16-byte pieces of either record
static_assert(sizeof(rene_lights_pixel) == 16 * LIGHTS_PIECES && sizeof(rene_lights_sample) == 16 * LIGHTS_PIECES, "the records the kernels store in 16-byte pieces");

// main_miss, lib.rs:120-139, of a ray that left the scene along rd (a Matte-only scene has no background)
template <bool MATTE>
RENE_DEV f3 lights_miss_colour(const SceneView& S, bool background, f3 rd) {
  if (MATTE || !background) return splat(0.0f);
  const uv2 uv = sphere_uv(normalize(m4_vector(S.uni->bg_matrix, rd)));
  return mk3(S.uni->bg_color[0], S.uni->bg_color[1], S.uni->bg_color[2]) * background_tex<LightsForm<MATTE>::FEAT>(S, uv);
}

// what a sample leaves beside its column
struct LightsEnd {
  uint32_t length, end, lit;
};

// one add of the estimator: the term t to group g of the lane's column (g < LIGHTS_GROUPS: the host has checked the tables).  true: t has a
// non-zero component
RENE_DEV bool lights_add(uint32_t* col, uint32_t g, f3 t) {
  uint32_t* p = col + 4u * g * BLOCK;
  const bool some = t.x != 0.0f || t.y != 0.0f || t.z != 0.0f;
  p[0] = __float_as_uint(__fadd_rn(__uint_as_float(p[0]), t.x));
  p[BLOCK] = __float_as_uint(__fadd_rn(__uint_as_float(p[BLOCK]), t.y));
  p[2 * BLOCK] = __float_as_uint(__fadd_rn(__uint_as_float(p[2 * BLOCK]), t.z));
  p[3 * BLOCK] += some ? 1u : 0u;
  return some;
}

// One sample into the lane's column `col`, which it zeroes first.  Every lane of the wave calls this, whatever its pixel (`live`: the slot is
// inside the image; else the lane asks nothing and adds nothing).
template <bool SMALL, bool MATTE>
RENE_DEV LightsEnd lights_sample(const SceneView& S, const LightsLaunch& L, bool live, uint32_t px, uint32_t py, uint32_t W, uint32_t H, uint32_t seed,
                                 uint32_t* stack, uint32_t* col) {
  constexpr uint32_t ALL = LightsForm<MATTE>::FEAT, KINDS = LightsForm<MATTE>::KINDS;
  constexpr int MAXL = LightsForm<MATTE>::MAXL;
  const float tmin = 0.001f, tmax = 100000.0f;  // lib.rs:182-183
#pragma unroll
  for (uint32_t w = 0; w < LIGHTS_WORDS; ++w) col[w * BLOCK] = 0u;
  Pcg rng;  // the pixel's generator, behind the two jitter draws
  const PrimaryRay r = primary_ray(S.uni, px, py, W, H, seed, rng);
  Pcg fw = pcg_new(seed);  // Q3: the frame-wide stream
  LaneCounters lc;
  f3 color = splat(1.0f), ro = r.o, rd = r.d;  // (ro, rd): the last ray the lane traced or is about to
  uint32_t i = 0u;
  bool alive = live, lit = false;
  LightsEnd q{0u, RENE_BOUNCES_END_MISS, 0u};
  const bool emitters = S.emit_object_len > 0, background = L.background != 0u;  // wave-uniform

  while (__ballot(alive) != 0ull) {  // lib.rs:192-357; i is wave-uniform
    if (alive) q.length++;
    const HitRec h = trace_accel<SMALL, false, true, false>(S.main, S.spheres, ro, rd, tmin, alive ? tmax : -1.0f, stack, lc);
    const bool hit = alive && h.slot != 0xffffffffu;
    if (alive && !hit) {  // main_miss, lib.rs:209-211
      const f3 t = color * lights_miss_colour<MATTE>(S, background, rd);
      lit |= lights_add(col, L.background_group, t);
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
        const f3 t = color * e;
        lit |= lights_add(col, L.instance_group[sf.instance], t);
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
        const f3 t = color * f * fabsf(dot(wi, normal)) * mk3(lL.x, lL.y, lL.z);
        lit |= lights_add(col, L.distant_group[li], t);
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
    i++;
    if (alive && i >= RENE_BOUNCES_MAX_DEPTH) alive = false, q.end = RENE_BOUNCES_END_CAP;  // lib.rs:192 (Q7)
  }
  q.lit = lit ? 1u : 0u;
  return q;
}

template <bool SMALL, bool MATTE>
__global__ void __launch_bounds__(BLOCK) lights_kernel(SceneView S, LightsLaunch L) {
  __shared__ uint32_t s_col[LIGHTS_WORDS][BLOCK];  // the SAMPLE's group words, a column per lane: [4 g + c] the value's component c, [4 g + 3] adds
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  uint32_t* col = &s_col[0][threadIdx.x];
  float sum[LIGHTS_GROUPS][3];  // the PIXEL's words: registers (every index below is static)
  uint32_t adds[LIGHTS_GROUPS], lit = 0u;
#pragma unroll
  for (uint32_t g = 0; g < LIGHTS_GROUPS; ++g) sum[g][0] = sum[g][1] = sum[g][2] = 0.0f, adds[g] = 0u;
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    const LightsEnd q = lights_sample<SMALL, MATTE>(S, L, live, x, py, W, H, L.seeds[f], stack, col);
#pragma unroll
    for (uint32_t g = 0; g < LIGHTS_GROUPS; ++g) {
      const uint32_t* p = col + 4u * g * BLOCK;
      sum[g][0] = __fadd_rn(sum[g][0], __uint_as_float(p[0]));
      sum[g][1] = __fadd_rn(sum[g][1], __uint_as_float(p[BLOCK]));
      sum[g][2] = __fadd_rn(sum[g][2], __uint_as_float(p[2 * BLOCK]));
      adds[g] += p[3 * BLOCK];
    }
    lit += q.lit;
  }
  if (!live) return;
  uint4* dst = reinterpret_cast<uint4*>(L.dst) + ((size_t)yi * W + x) * LIGHTS_PIECES;
#pragma unroll
  for (uint32_t g = 0; g < LIGHTS_GROUPS; ++g) dst[g] = make_uint4(__float_as_uint(sum[g][0]), __float_as_uint(sum[g][1]), __float_as_uint(sum[g][2]), adds[g]);
  dst[LIGHTS_GROUPS] = make_uint4(L.n_frames, lit, 0u, 0u);
}

// the per-sample probe: the same device function, every sample's rene_lights_sample into [n_frames][H][W]
template <bool SMALL, bool MATTE>
__global__ void __launch_bounds__(BLOCK) lights_samples_kernel(SceneView S, LightsLaunch L) {
  __shared__ uint32_t s_col[LIGHTS_WORDS][BLOCK];
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t x, yi;
  bool live;
  if (!pass_pixel(L.grid, x, yi, live)) return;
  const uint32_t W = L.grid.width, H = L.grid.height, py = H - 1u - yi;
  uint32_t* col = &s_col[0][threadIdx.x];
  for (uint32_t f = 0; f < L.n_frames; ++f) {
    const LightsEnd q = lights_sample<SMALL, MATTE>(S, L, live, x, py, W, H, L.seeds[f], stack, col);
    if (!live) continue;  // (behind the sample: the wave's queries are over)
    uint4* dst = reinterpret_cast<uint4*>(L.dst) + (((size_t)f * H + yi) * W + x) * LIGHTS_PIECES;
#pragma unroll
    for (uint32_t g = 0; g < LIGHTS_GROUPS; ++g) {
      const uint32_t* p = col + 4u * g * BLOCK;
      dst[g] = make_uint4(p[0], p[BLOCK], p[2 * BLOCK], p[3 * BLOCK]);
    }
    dst[LIGHTS_GROUPS] = make_uint4(1u, q.lit, q.length, q.end);
  }
}

hipError_t launch_lights(const LaunchConfig& cfg, const SceneView& S, const LightsLaunch& L, bool samples, hipStream_t st) {
  const bool matte = shade_class(cfg.features) == ShadeClass::Matte;  // (kernel_select.h: where the render launchers choose one lobe over five)
  if (samples)
    return launch_pixel_pass(cfg, S, L, matte ? lights_samples_kernel<true, true> : lights_samples_kernel<true, false>,
                             matte ? lights_samples_kernel<false, true> : lights_samples_kernel<false, false>, st);
  return launch_pixel_pass(cfg, S, L, matte ? lights_kernel<true, true> : lights_kernel<true, false>,
                           matte ? lights_kernel<false, true> : lights_kernel<false, false>, st);
}

}  // namespace rene
