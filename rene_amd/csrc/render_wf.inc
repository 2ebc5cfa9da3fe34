// render_wf.inc -- included by kernels.hip.
//
// render_kernel_wf: the integrator for scenes that need the BVH (everything too large for the
// wave-coherent item loop).  Same arithmetic, same RNG order, same summation order as
// render_kernel, but scheduled as a per-lane state machine:
//
//   * every lane carries a *ray query* (closest / shadow / emitter-pdf) with its own traversal
//     cursor and LDS stack; one loop iteration advances every in-flight query by ONE step (an inner
//     node, or a leaf);
//   * the lanes whose query has completed wait until `READY_MIN` of them have accumulated (or no
//     query is in flight) and are then served together by the *logic step*: hit shading, light
//     loop, BSDF / emitter sampling, Russian roulette, path regeneration, work-item bookkeeping --
//     each ending with the lane's next query;
//   * so a lane that finishes its traversal early does not idle until the slowest of its 63
//     neighbours is done (the while-while kernel measured ~7 active lanes per vector-memory
//     instruction on the 870 k-triangle scene): it is refilled with its path's next ray -- the
//     "wavefront-ballot traversal restart" of BASELINE.json's north star, with the path state kept
//     in registers instead of HBM queues.
//
// The surface / BSDF state is NOT kept across a shadow query: it is recomputed from the stored hit
// record (slot, u, v, t) and the incoming ray, which costs a few cached loads and keeps the kernel
// at an occupancy that hides the BVH's memory latency.

// PH_LAST_SHADOW + n: the shadow query of the bounce's LAST distant light is in flight and the rest of the bounce has been
// done already; when it completes the lane adds the light's share itself and goes straight on to phase n (PH_NEWPATH,
// PH_CLOSEST or PH_EMIT) -- no second visit of the logic step per bounce (see the logic step)
enum : uint32_t { PH_NEWPATH = 0, PH_CLOSEST = 1, PH_SHADOW = 2, PH_EMIT = 3, PH_LAST_SHADOW = 4 };
// FEAT_VOLPATH (main_ray_generation_volpath, lib.rs:477-803): the bounce's inner loops -- the transmittance walks tr / tr_emit
// (lib.rs:359-468), one closest-hit query per surface crossed -- become phases of their own, so that a walk's queries are
// scheduled like any other query:
//   PV_WALK_L_SC / _SF  a walk towards distant light `li` from a scattering vertex / from a surface
//   PV_EMITQ_SC         the emitter-pdf query of the emitter sample drawn at a scattering vertex (lib.rs:599-654)
//   PV_WALK_E_SC        the walk towards that emitter (tr_emit)
//   PV_EMITQ_SF         the emitter-pdf query of the surface's one-sample mixture (lib.rs:703-754)
enum : uint32_t { PV_WALK_L_SC = 8, PV_WALK_L_SF = 9, PV_EMITQ_SC = 10, PV_WALK_E_SC = 11, PV_EMITQ_SF = 12 };
// thresholds (RenderParams.ready_min / leaf_min): lanes that must be waiting before the logic step
// runs, and lanes that must be at a leaf before the leaf step runs

template <uint32_t FEAT, int MAXL, bool COUNT, bool AOV, bool TABLES = false>
#ifndef RENE_WF_NODE_STEPS
#define RENE_WF_NODE_STEPS 3  // inner-node steps per loop iteration: the ballots, the logic-step test and the leaf step are paid once per
                               // iteration (measured, dragon- / teapot-class Grays/s: 1: 4.94 / 5.66, 2: 5.26 / 5.76, 3: 5.32 / 5.96, 4: 5.25 / 5.69)
#endif
#ifndef RENE_WF_POSTPONE
#define RENE_WF_POSTPONE 0  // speculative traversal (the traversal step below): 0 off, 1 closest-hit and emitter queries, 2 occlusion queries too
#endif
#ifndef RENE_WF_GEN1_WAVES
#define RENE_WF_GEN1_WAVES 3  // waves per SIMD requested for the general single-lobe variants (171 VGPRs otherwise: 2 waves)
#endif
#ifndef RENE_WF_GEN1_BLEND_WAVES
#define RENE_WF_GEN1_BLEND_WAVES 4  // ... and for the instantiation with Substrate as the only general material (teapot-class): 128 VGPRs without scratch
                                     // since the device code is built without SLP packing (136 and three waves unasked): 9.2 -> 10.6 Grays/s
#endif
#ifndef RENE_WF_MATTE_WAVES
#define RENE_WF_MATTE_WAVES 1
#endif
// (only the production variant -- first-hit layers on, counters off -- fits 168 VGPRs without scratch; the others
// stay at 2 waves rather than combine SGPR spills with VGPR spills, DESIGN.md section 5)
__global__ void __launch_bounds__(BLOCK, (FEAT & FEAT_VOLPATH) ? 1 : (FEAT & FEAT_GENERAL_BSDF) ? ((MAXL == 1 && AOV && !COUNT) ? (((FEAT & FEAT_NO_SPECULAR) && (FEAT & FEAT_NO_MICROFACET)) ? RENE_WF_GEN1_BLEND_WAVES : RENE_WF_GEN1_WAVES) : 1) : RENE_WF_MATTE_WAVES) render_kernel_wf(SceneView S, RenderParams P) {
  constexpr bool SPHERES = (FEAT & FEAT_SPHERES) != 0;
  constexpr uint32_t GENERAL = lobe_kinds(FEAT);  // 0: Matte only
  // FEAT_NO_EMITTERS: a scene without emit objects never runs the one-sample emitter mixture (lib.rs:274-324); without its
  // branches the path state is four registers smaller (the pending f and pdf) and the Substrate kernel stops spilling SGPRs
  constexpr bool EMITTERS = !(FEAT & FEAT_NO_EMITTERS);
  constexpr bool VOL = (FEAT & FEAT_VOLPATH) != 0;
  static_assert(!VOL || (EMITTERS && !TABLES), "the volpath instantiations keep the emitter state and read their tables from global memory");
  extern __shared__ uint32_t s_stack[];  // [stack depth][BLOCK]; then, TABLES: every Inst and every distant Light
  uint32_t* stack = s_stack + threadIdx.x;
  const karg_ptr KB0 = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  // TABLES: the tables every shaded hit reads are in LDS (the launcher picks this instantiation when they fit,
  // kernels_bvh.hip): one round trip to the memory system less for the instance record, one less for the light
  // (where the tables are is re-read from the kernel arguments by the logic step, like the other cold arguments: two more SGPRs
  // held across the traversal steps are two more spilled)
  if constexpr (TABLES) {
    const uint32_t n_li = S.lds_insts;
    __attribute__((address_space(3))) lds_v4* dst = (__attribute__((address_space(3))) lds_v4*)(s_stack + P.stack_entries * BLOCK);
    const lds_v4* a = reinterpret_cast<const lds_v4*>(S.insts);
    const lds_v4* b = reinterpret_cast<const lds_v4*>(S.lights);
    const uint32_t na = (uint32_t)(sizeof(Inst) / 16) * n_li, nb = (uint32_t)(sizeof(Light) / 16) * S.lights_len;
    for (uint32_t i = threadIdx.x; i < na + nb; i += BLOCK) dst[i] = i < na ? a[i] : b[i - na];
  }
  seed_tables_fill(P, s_stack);  // behind the stack (and the tables)
  __syncthreads();

  LaneCounters lc;
  uint32_t st_node = 0, st_leaf = 0, st_logic = 0, st_iter = 0, ln_leaf = 0, ln_logic = 0, ln_dead = 0, ln_popped = 0, ln_popped_dead = 0, ln_top = 0, sp_max = 0;
  bool popped = false;  // COUNT: executions of each step kind and the lanes they served
  uint32_t ln_rep[RENE_WF_NODE_STEPS] = {};  // COUNT: lanes at an inner node at the iteration's first, second, ... node step (how fast a wave's density decays without a re-grouping)
  const uint32_t W = S.width, H = S.height;
  const float tmin = 0.001f, tmax = 100000.0f;  // lib.rs:182-183

  // ---- work item (see render_kernel) ----
  uint32_t ver = 0, px = 0, py = 0, frame = 0, frame_end = 0;  // ver: the lane's work item = the version it will leave (device_code.inc); 0 = none
  bool waiting = false, done = false;
  f3 acc0 = splat(0.0f), acc1 = splat(0.0f), acc2 = splat(0.0f);
  const size_t layer_stride = (size_t)(P.n_work >> CHAINS_LOG2) * 4;  // n_slots records
  // frame chains (device_scene.h, CHAINS): `py` carries the item's chain in its upper half (rows are below 65536); chain g's sums
  // are in the g-th [3][n_slots][4] block behind `framebuffer`, its versions in the g-th [n_slots] block of `item_done`, at the pixel's slot
  const karg_ptr KB = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr();  // cold arguments are re-read where they are used (karg_u32)
  auto pyy = [&]() { return py & 0xffffu; };
  auto rec_pixel = [&]() {
    uint32_t n_slots;
    const uint32_t slot = pixel_slot(KB, px, H - 1 - pyy(), n_slots);
    return (py >> 16) * n_slots + slot;  // < 2^31: n_slots <= 2^28
  };
  auto rec_offset = [&]() { return pixel_record(KB, px, H - 1 - pyy(), py >> 16) * 4; };
  uint32_t batch_next = 0, batch_ll = 0;  // the wave's batch of work ids: the next level-local id, level << 16 | ids left (device_code.inc)
  bool exhausted = false;
  first_batch(P, KB, batch_next, batch_ll);
  wave_stamp(KB, 0);
  clock_probe(P, false);

  // ---- path ----
  f3 ro = splat(0.0f), rd = splat(0.0f), color = splat(0.0f);
  Pcg rng{0}, fw{0};
  int depth = 0;
  uint32_t phase = PH_NEWPATH;
  HitRec hit;  // the closest hit being shaded (kept across its shadow queries)
  hit.t = hit.u = hit.v = 0.0f;
  hit.slot = 0xffffffffu;
  uint32_t li = 0;            // next distant light
  f3 pend_f = splat(0.0f);    // f * |n . wi| of the sampled direction, applied after the emitter query
  float pend_pdf = 0.0f;

  // ---- ray query ----
  bool q_active = false, q_any = false, q_emit = false;
  f3 qo = splat(0.0f), qd = splat(0.0f), qinv = splat(0.0f);
  float q_tmax = 0.0f;
  uint32_t cur = 0, pleaf = 0;  // pleaf: the leaf put aside (RENE_WF_POSTPONE), 0 = none
  constexpr uint32_t CUR_NONE = 0xffffffffu;  // cur: nothing left to visit (no leaf word looks like this: sixteen spheres from slot 2^26 - 1)
  int sp = 0;
  HitRec best;
  best.t = best.u = best.v = 0.0f;
  best.slot = 0xffffffffu;

  auto issue = [&](f3 o, f3 d, float t_max, bool any, bool emit) {
    if constexpr (COUNT) {  // rene_ray_dump (probe): the query as a wavefront's shading pass would have queued it
      if (P.ray_dump) {
        const uint32_t at = atomicAdd(reinterpret_cast<uint32_t*>(P.ray_dump), 1u);
        if (at < P.ray_dump_cap) {
          float4* rec = reinterpret_cast<float4*>(P.ray_dump) + 2 + 2 * (size_t)at;
          rec[0] = make_float4(o.x, o.y, o.z, t_max);
          rec[1] = make_float4(d.x, d.y, d.z, __uint_as_float(((H - 1 - pyy()) * W + px) | ((uint32_t)depth << 21) | ((any ? 1u : 0u) << 27) | ((emit ? 1u : 0u) << 28) |
                                                               (((frame - CHAINS) & 7u) << 29)));  // (frame: the launch's frame the path belongs to, its low three bits)
        }
      }
    }
    qo = o;
    qd = d;
    qinv = safe_inv(d);
    q_tmax = t_max;
    q_any = any;
    q_emit = emit;
    cur = 0;  // the root of either structure is inner node 0
    pleaf = 0;
    sp = 0;
    best.slot = 0xffffffffu;
    q_active = true;
  };
  // lib.rs:340-355 + loop control: what follows the bounce -- the path's next closest query (PH_CLOSEST) or its end (PH_NEWPATH)
  auto post_bounce = [&](bool alive) -> uint32_t {
    if (alive && is_zero(color)) alive = false;
    if (alive && depth > 12) {
      float rr_coin = pcg_f32(fw);
      float continue_p = max_element(color);
      if (rr_coin > continue_p) alive = false;
      else color = color / continue_p;
    }
    depth++;
    if (depth >= 50) alive = false;  // lib.rs:192 (Q7)
    return alive ? (uint32_t)PH_CLOSEST : (uint32_t)PH_NEWPATH;
  };
  // enter phase `next` with the query it stands for, along the path's (ro, rd)
  auto start = [&](uint32_t next) {
    phase = next;
    if (next == PH_CLOSEST) {
      lc.closest++;
      issue(ro, rd, tmax, false, false);
    } else if (EMITTERS && next == PH_EMIT) {
      lc.emitter++;
      issue(ro, rd, tmax, false, true);  // Q5: emitter-only structure
    }
  };
  f3 pend_light = splat(0.0f);  // PH_LAST_SHADOW: color * f * |n . wi| * L of the last distant light, added if its shadow query finds nothing
  // volpath: the medium the path travels in (0 = vacuum, lib.rs:529) and the walk in flight -- what it has accumulated, the
  // medium of its current segment, the segments so far (a walk crosses at most 4096 surfaces: every wave leaves)
  uint32_t medium_index = 0, walk_medium = 0, walk_guard = 0;
  f3 walk_tr = splat(1.0f);

  for (uint32_t iter = 0;; ++iter) {
    // ================================================================================================
    // logic step: serve the lanes whose query has completed (or that have none yet)
    // ================================================================================================
    // (a lane that waits for a hand-off -- it polled once, in the step that gave it its item -- takes part, and is counted by
    // the ballot, only on every RENE_POLL_EVERY-th iteration: a poll is a cache-bypassing round trip the whole wave stands behind, and a waiting lane that counted as
    // ready on every iteration made the logic step run for a handful of lanes)
    const bool ready = !q_active && !done && (!waiting || (iter & (RENE_POLL_EVERY - 1u)) == 0u);
    const uint32_t n_ready = (uint32_t)__popcll(__ballot(ready));
    const uint32_t n_trav = (uint32_t)__popcll(__ballot(q_active));
    if (n_ready != 0 && (n_ready >= P.ready_min || n_trav == 0)) {
      // the scene tables only this step reads: loaded from the kernarg segment here, not parked in SGPRs (and spilled
      // into VGPR lanes) across the traversal steps -- logic_view, device_code.inc
      const SceneView L = logic_view(KB, S, iter);
      // where the LDS tables are: both kernel arguments behind ONE wait (a scalar load and its wait per use was a scalar-cache round
      // trip per use -- a dozen and more per logic step with the eleven of logic_view, most of them for pointers this
      // instantiation never reads)
      uint32_t k_stack_entries = 0, k_lds_insts = 0;
      if constexpr (TABLES)
        asm volatile("s_load_dword %0, %2, %3\n\ts_load_dword %1, %2, %4\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(k_stack_entries), "=&s"(k_lds_insts)
                     : "s"(KB0), "n"(RENE_KARG(stack_entries)), "n"(RENE_SKARG(lds_insts)));
      auto lds_insts = [&]() { return (lds_ptr)s_stack + k_stack_entries * BLOCK; };
      auto lds_lights = [&]() { return lds_insts() + (uint32_t)(sizeof(Inst) / 4) * k_lds_insts; };
      auto light_dir = [&](const SceneView& V, uint32_t i) { return TABLES ? lds4(lds_lights() + 8u * i) : ldg4(V.lights[i].dir); };
      auto light_L = [&](const SceneView& V, uint32_t i) { return TABLES ? lds4(lds_lights() + 8u * i + 4u) : ldg4(V.lights[i].L); };
      if (COUNT) {
        st_logic++;
        if (ready) ln_logic++;
      }
      if constexpr (VOL) {
       if (ready && phase != PH_NEWPATH) {
        // What the completed query leads to, as a chain of blocks the lane runs through in ONE visit of this step -- each block
        // the statement-for-statement body of render_kernel's volpath branch (device_code.inc), cut where that one traces a ray.
        enum : uint32_t { ACT_NONE = 0, ACT_LIGHTS_SC, ACT_LIGHTS_SF, ACT_AFTER_SC, ACT_AFTER_SF, ACT_SAMPLE_P, ACT_END_SURFACE, ACT_END_BOUNCE };
        uint32_t act = ACT_NONE;
        bool alive = true;
        const f3 wo = -normalize(rd);  // rd is the INCOMING direction until the bounce ends (a scattering vertex moves ro only)
        // the surface of the closest hit, evaluated again from the stored hit record where a later block needs it
        const bool at_surface = (phase == PH_CLOSEST && best.slot != 0xffffffffu) || phase == PV_WALK_L_SF || phase == PV_EMITQ_SF;
        if (phase == PH_CLOSEST && best.slot != 0xffffffffu) {
          hit = best;
          lc.hits++;
        }
        Surface sf{};
        f3 normal = splat(0.0f), position = splat(0.0f);
        Bsdf<MAXL> bsdf;
        bsdf.len = 0;
        bsdf.codes = 0xffffffffu;
        uint32_t sf_instance = 0;
        if (at_surface) {
          sf = shade_hit<SPHERES>(L, hit, ro, rd);
          sf_instance = sf.instance;
          normal = normalize(sf.normal);
          position = sf.position;
          bsdf.ng = normal;
          bsdf.onb = onb_from_w(normal);
          compute_bsdf<FEAT, MAXL>(L, L.insts[sf_instance], sf.uv, bsdf);
        }
        // one segment of a walk, transmittance() of device_code.inc: issue it, or end the walk with `result`
        auto walk_begin = [&](f3 o, f3 d, uint32_t kind) {
          walk_tr = splat(1.0f);
          walk_medium = medium_index;
          walk_guard = 0;
          lc.shadow++;
          issue(o, d, 1e5f, false, false);
          phase = kind;
        };

        // ---- block A: the query that has completed ----
        if (phase == PH_CLOSEST) {
          if (best.slot == 0xffffffffu) {  // main_miss, lib.rs:120-139, 209-211
            f3 bg = splat(0.0f);
            if (FEAT & FEAT_BACKGROUND) {
              uv2 uv = sphere_uv(normalize(m4_vector(L.uni->bg_matrix, rd)));
              bg = mk3(L.uni->bg_color[0], L.uni->bg_color[1], L.uni->bg_color[2]) * background_tex<FEAT>(L, uv);
            }
            acc0 = acc0 + color * bg;
            lc.adds++;
            phase = PH_NEWPATH;
          } else {  // lib.rs:552-565
            const Inst& inst = L.insts[sf_instance];
            MediumRec medium = load_medium(L, medium_index);
            bool scattered = false;
            if (medium.type != RENE_MEDIUM_VACUUM) {
              SampledMedium sm = medium_sample(medium, ro, rd, hit.t, rng);
              color = color * sm.tr;
              scattered = sm.sampled;
              if (scattered) ro = sm.position;
            }
            li = 0;
            if (scattered) {
              act = ACT_LIGHTS_SC;
            } else {  // the surface, lib.rs:657-670
              if (inst.emit[3] != 0.0f) {
                f3 e = dot(wo, normal) > 0.0f ? mk3(inst.emit[0], inst.emit[1], inst.emit[2]) : splat(0.0f);
                acc0 = acc0 + color * e;
                lc.adds++;
              }
              if (depth == 0) {
                if (AOV) {
                  acc1 = acc1 + normal;
                  acc2 = acc2 + material_albedo<FEAT>(L, inst, sf.uv);
                }
                lc.adds += 2;
              }
              if (inst.material_type != RENE_MATERIAL_NONE) {
                act = ACT_LIGHTS_SF;
              } else {  // a medium boundary: straight through, lib.rs:768-773
                ro = position;
                act = ACT_END_SURFACE;
              }
            }
          }
        } else if (phase == PV_WALK_L_SC || phase == PV_WALK_L_SF || phase == PV_WALK_E_SC) {
          // tr / tr_emit, lib.rs:359-468: the segment (qo, qd) has met a surface, or nothing
          const bool to_emitter = phase == PV_WALK_E_SC;
          bool ended = true;
          f3 result = splat(0.0f);
          if (best.slot == 0xffffffffu) {
            result = to_emitter ? splat(0.0f) : walk_tr;
          } else {
            Surface ws = shade_hit<SPHERES>(L, best, qo, qd);
            const Inst& wi_inst = L.insts[ws.instance];
            if (to_emitter && wi_inst.emit[3] != 0.0f) {  // area_light.emit(-normalize(rd), payload.normal), lib.rs:447-451
              f3 wo_w = -normalize(qd);
              result = dot(wo_w, ws.normal) > 0.0f ? walk_tr * mk3(wi_inst.emit[0], wi_inst.emit[1], wi_inst.emit[2]) : splat(0.0f);
            } else if (wi_inst.material_type != RENE_MATERIAL_NONE) {
              result = splat(0.0f);
            } else {
              MediumRec m = load_medium(L, walk_medium);
              if (m.type != RENE_MEDIUM_VACUUM) walk_tr = walk_tr * medium_tr(m, qd, best.t);
              InstMedium im = L.inst_medium[ws.instance];
              walk_medium = dot(qd, ws.normal) > 0.0f ? im.exterior : im.interior;
              walk_guard++;
              if (walk_guard >= 4096u) {
                result = walk_tr;
              } else {
                ended = false;
                lc.shadow++;
                issue(ws.position, qd, 1e5f, false, false);  // the phase stays: the walk's next segment
              }
            }
          }
          if (ended) {
            const f3 wi = qd;
            if (phase == PV_WALK_L_SC) {  // lib.rs:567-597
              MediumRec medium = load_medium(L, medium_index);
              float4 lL = light_L(L, li);
              acc0 = acc0 + color * result * medium_phase(medium, wo, wi) * mk3(lL.x, lL.y, lL.z);
              lc.adds++;
              li++;
              act = ACT_LIGHTS_SC;
            } else if (phase == PV_WALK_L_SF) {  // lib.rs:671-701
              float4 lL = light_L(L, li);
              f3 f = bsdf_f<MAXL, GENERAL>(bsdf, wo, wi);
              acc0 = acc0 + color * result * f * fabsf(dot(wi, normal)) * mk3(lL.x, lL.y, lL.z);
              lc.adds++;
              li++;
              act = ACT_LIGHTS_SF;
            } else {  // the emitter sample of a scattering vertex, lib.rs:599-654
              MediumRec medium = load_medium(L, medium_index);
              float pdf = qdiv(pend_pdf, (float)L.emit_object_len);
              if (pdf > 1e-5f) {
                acc0 = acc0 + color * result * medium_phase(medium, wo, wi) / pdf;
                lc.adds++;
              }
              act = ACT_SAMPLE_P;
            }
          }
        } else if (phase == PV_EMITQ_SC) {
          pend_pdf = emitter_pdf<SPHERES>(L, best, qo, qd);
          walk_begin(qo, qd, PV_WALK_E_SC);
        } else if (phase == PV_EMITQ_SF) {  // lib.rs:736-754; (qo, qd) = (position, wi): the path's next ray
          float pdf_l = emitter_pdf<SPHERES>(L, best, qo, qd);
          ro = qo;
          rd = qd;  // (wo above was taken from the incoming direction)
          color = color * pend_f;
          float pdf = 0.5f * pend_pdf + qdiv(0.5f * pdf_l, (float)L.emit_object_len);
          if (pdf < 1e-5f) alive = false;
          else color = color / pdf;
          act = ACT_END_SURFACE;
        }

        // ---- block B: the next distant light, or what follows the lights ----
        if (act == ACT_LIGHTS_SC || act == ACT_LIGHTS_SF) {
          if ((FEAT & FEAT_LIGHTS) && li < L.lights_len) {
            float4 ld = light_dir(L, li);
            const f3 from = act == ACT_LIGHTS_SC ? ro : position;
            f3 wi = normalize((from + mk3(ld.x, ld.y, ld.z)) - from);
            walk_begin(from, wi, act == ACT_LIGHTS_SC ? (uint32_t)PV_WALK_L_SC : (uint32_t)PV_WALK_L_SF);
            act = ACT_NONE;
          } else {
            act = act == ACT_LIGHTS_SC ? (uint32_t)ACT_AFTER_SC : (uint32_t)ACT_AFTER_SF;
          }
        }
        // ---- block C: after the lights ----
        if (act == ACT_AFTER_SC) {  // emitter sample drawn from the PIXEL stream here, lib.rs:599-654
          if (L.emit_object_len > 0) {
            uint32_t obj = umod(pcg_u32(rng), L.emit_object_len);
            f3 wi = normalize(emit_sample<SPHERES>(L, obj, rng) - ro);
            lc.emitter++;
            issue(ro, wi, tmax, false, true);
            phase = PV_EMITQ_SC;
            act = ACT_NONE;
          } else {
            act = ACT_SAMPLE_P;
          }
        }
        if (act == ACT_AFTER_SF) {
          if (L.emit_object_len > 0 && bsdf_contains<MAXL, GENERAL>(bsdf, K_DIFFUSE)) {  // lib.rs:703-754
            f3 wi, f;
            float pdf;
            if (pcg_f32(fw) > 0.5f) {
              uint32_t obj = umod(pcg_u32(fw), L.emit_object_len);
              wi = normalize(emit_sample<SPHERES>(L, obj, fw) - position);
              pdf = bsdf_pdf<MAXL, GENERAL>(bsdf, wi, normal);
              f = bsdf_f<MAXL, GENERAL>(bsdf, wo, wi);
            } else {
              Sampled sm = bsdf_sample<MAXL, GENERAL>(bsdf, wo, rng);
              wi = sm.wi;
              pdf = sm.pdf;
              f = sm.f;
            }
            // (the incoming ray is needed once more -- for the surface of the stored hit, when the query comes back -- so the
            // path's next ray lives in the query until then)
            pend_f = f * fabsf(dot(normal, wi));
            pend_pdf = pdf;
            lc.emitter++;
            issue(position, wi, tmax, false, true);
            phase = PV_EMITQ_SF;
            act = ACT_NONE;
          } else {  // lib.rs:755-767
            Sampled sm = bsdf_sample<MAXL, GENERAL>(bsdf, wo, rng);
            if (sm.pdf < 1e-5f) {
              alive = false;
            } else {
              color = color * (sm.f * qdiv(fabsf(dot(normal, sm.wi)), sm.pdf));
              ro = position;
              rd = sm.wi;
            }
            act = ACT_END_SURFACE;
          }
        }
        if (act == ACT_SAMPLE_P) {  // lib.rs:656
          MediumRec medium = load_medium(L, medium_index);
          rd = medium_sample_p(medium, wo, rng);
          act = ACT_END_BOUNCE;
        }
        if (act == ACT_END_SURFACE) {  // lib.rs:775-779: the side of the surface the path arrived on decides the medium it goes on in
          InstMedium im = L.inst_medium[sf_instance];
          medium_index = dot(wo, normal) < 0.0f ? im.exterior : im.interior;
          act = ACT_END_BOUNCE;
        }
        if (act == ACT_END_BOUNCE) {  // lib.rs:783-801; the roulette is commented out upstream
          if (alive && is_zero(color)) alive = false;
          depth++;
          if (depth >= 80) alive = false;  // MAX_DEPTH, lib.rs:499
          start(alive ? (uint32_t)PH_CLOSEST : (uint32_t)PH_NEWPATH);
        }
       }
      } else
      if (ready) {
        // ---- after the emitter-pdf query, lib.rs:301-324 ----
        if (EMITTERS && phase == PH_EMIT) {
          float pdf_l = emitter_pdf<SPHERES>(L, best, ro, rd);
          color = color * pend_f;
          float pdf = 0.5f * pend_pdf + qdiv(0.5f * pdf_l, (float)L.emit_object_len);
          bool alive = true;
          if (pdf < 1e-5f) alive = false;
          else color = color / pdf;
          start(post_bounce(alive));
        }
        // ---- after the closest-hit query (lib.rs:209-232) or a shadow query (lib.rs:260-271) ----
        else if (phase == PH_CLOSEST || phase == PH_SHADOW) {
          bool shade = true;
          if (phase == PH_CLOSEST) {
            if (best.slot == 0xffffffffu) {  // main_miss, lib.rs:120-139, 209-211
              f3 bg = splat(0.0f);
              if (FEAT & FEAT_BACKGROUND) {
                uv2 uv = sphere_uv(normalize(m4_vector(L.uni->bg_matrix, rd)));
                bg = mk3(L.uni->bg_color[0], L.uni->bg_color[1], L.uni->bg_color[2]) * background_tex<FEAT>(L, uv);
              }
              acc0 = acc0 + color * bg;
              lc.adds++;
              phase = PH_NEWPATH;
              shade = false;
            } else {
              hit = best;
              lc.hits++;
            }
          }
          if (shade) {
            Surface sf = shade_hit<SPHERES>(L, hit, ro, rd);
            // (a reference either way: the fields are read where they are used, from LDS or from global memory)
            const Inst& inst = TABLES ? reinterpret_cast<const Inst*>(s_stack + k_stack_entries * BLOCK)[sf.instance]
                                      : L.insts[sf.instance];
            f3 wo = -normalize(rd);
            f3 normal = normalize(sf.normal);
            f3 position = sf.position;
            Bsdf<MAXL> bsdf;
            bsdf.len = 0;
            bsdf.codes = 0xffffffffu;
            bsdf.ng = normal;
            bsdf.onb = onb_from_w(normal);
            compute_bsdf<FEAT, MAXL>(L, inst, sf.uv, bsdf);
            if (phase == PH_CLOSEST) {
              if (inst.emit[3] != 0.0f) {  // lib.rs:225-227, area_light.rs:66-74
                f3 e = dot(wo, normal) > 0.0f ? mk3(inst.emit[0], inst.emit[1], inst.emit[2]) : splat(0.0f);
                acc0 = acc0 + color * e;
                lc.adds++;
              }
              if (depth == 0) {  // lib.rs:229-232
                if (AOV) {
                  acc1 = acc1 + normal;
                  acc2 = acc2 + material_albedo<FEAT>(L, inst, sf.uv);
                }
                lc.adds += 2;
              }
              li = 0;
            } else {  // result of the shadow query for light li, lib.rs:260-271
              if (best.slot == 0xffffffffu) {
                float4 ld = light_dir(L, li), lL = light_L(L, li);
                f3 wi = normalize((position + mk3(ld.x, ld.y, ld.z)) - position);
                f3 f = bsdf_f<MAXL, GENERAL>(bsdf, wo, wi);
                acc0 = acc0 + color * f * fabsf(dot(wi, normal)) * mk3(lL.x, lL.y, lL.z);
                lc.adds++;
              }
              li++;
            }
            // the rest of the bounce (lib.rs:274-337): the one-sample emitter mixture or a BSDF sample; leaves the path's next
            // ray in (ro, rd) and returns the phase that follows -- the emitter-pdf query, the next closest query, the path's end
            auto rest_of_bounce = [&]() -> uint32_t {
              if (EMITTERS && L.emit_object_len > 0 && bsdf_contains<MAXL, GENERAL>(bsdf, K_DIFFUSE)) {  // lib.rs:274-314
                f3 wi, f;
                float pdf;
                if (pcg_f32(fw) > 0.5f) {  // Q3: frame-wide stream
                  uint32_t obj = umod(pcg_u32(fw), L.emit_object_len);
                  wi = normalize(emit_sample<SPHERES>(L, obj, fw) - position);
                  pdf = bsdf_pdf<MAXL, GENERAL>(bsdf, wi, normal);  // Q1: (wi, normal), lib.rs:287
                  f = bsdf_f<MAXL, GENERAL>(bsdf, wo, wi);
                } else {
                  Sampled s = bsdf_sample<MAXL, GENERAL>(bsdf, wo, rng);
                  wi = s.wi;
                  pdf = s.pdf;
                  f = s.f;
                }
                ro = position;
                rd = wi;
                pend_f = f * fabsf(dot(normal, wi));
                pend_pdf = pdf;
                return PH_EMIT;
              }
              Sampled s = bsdf_sample<MAXL, GENERAL>(bsdf, wo, rng);  // lib.rs:325-337
              bool alive = true;
              if (s.pdf < 1e-5f) {
                alive = false;
              } else {
                color = color * (s.f * qdiv(fabsf(dot(normal, s.wi)), s.pdf));
                ro = position;
                rd = s.wi;
              }
              return post_bounce(alive);
            };
            if ((FEAT & FEAT_LIGHTS) && li < L.lights_len) {  // lib.rs:234-258
              float4 ld = light_dir(L, li);
              f3 wi = normalize((position + mk3(ld.x, ld.y, ld.z)) - position);  // light.rs:52-55
              lc.shadow++;
              if (li + 1u == L.lights_len) {
                // The bounce's last light.  Nothing of what follows in the bounce depends on its shadow query but ONE add
                // (lib.rs:260-271): the light's share is put aside (pend_light; the throughput changes below), the rest of the
                // bounce runs now, and the lane that finishes the shadow query adds the share -- or not -- and starts the
                // query that follows without coming back here: one visit of the logic step per bounce instead of two, and no
                // second evaluation of the hit's surface and BSDF.  Same draws from both generators in the same order (a
                // shadow query draws nothing), same adds in the same order (the next add of this pixel is the next bounce's).
                f3 f = bsdf_f<MAXL, GENERAL>(bsdf, wo, wi);
                const float4 lL = light_L(L, li);  // (the same product in the same order as lib.rs:260-271, formed here: the lane that ends the query only adds)
                pend_light = color * f * fabsf(dot(wi, normal)) * mk3(lL.x, lL.y, lL.z);
                const uint32_t next = rest_of_bounce();
                issue(position, wi, 1e5f, true, false);
                phase = PH_LAST_SHADOW + next;
              } else {
                issue(position, wi, 1e5f, true, false);
                phase = PH_SHADOW;
              }
            } else {
              start(rest_of_bounce());
            }
          }
        }
      }
      // ---- work-item bookkeeping + ray generation (same protocol as render_kernel) ----
      if (ready) {
        if (phase == PH_NEWPATH) {
          if (!waiting && ver != 0u && frame == frame_end) {  // item finished: commit its sums
            float* p = reinterpret_cast<float*>(karg_u64<RENE_KARG(framebuffer)>(KB)) + rec_offset();
            if (AOV) {
              fb_store_rgb(p + layer_stride, acc1);
              fb_store_rgb(p + 2 * layer_stride, acc2);
            }
            fb_store_rgb(p, acc0);
            item_flag_publish(KB, ver, rec_pixel());
            ver = 0u;
          }
        }
      }
      // item fetch: wave-uniform control flow (ballots inside), so outside the per-lane `if (ready)`
      {
        bool need = ready && phase == PH_NEWPATH && ver == 0u;
        if (__any(need)) {
          if ((batch_ll & 0xffffu) == 0u && !exhausted) exhausted = !batch_refill(KB, batch_next, batch_ll);
          unsigned long long mask = __ballot(need);
          uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane_id()) - 1ull));
          const uint32_t batch_level = batch_ll >> 16, left = batch_ll & 0xffffu;
          uint32_t id = batch_next + rank;  // level-local
          bool got = need && !exhausted && rank < left;
          uint32_t taken = (uint32_t)__popcll(mask);
          taken = taken < left ? taken : left;
          batch_next += taken;
          batch_ll -= taken;
          if (need && exhausted) done = true;
          if (got) {
            const ItemArgs IA = item_args(KB);
            uint32_t w = id;
            const uint32_t level = batch_level;
            const uint32_t grp = w & (CHAINS - 1u);  // frame chains: a level's ids are pixel slot * CHAINS + chain
            w >>= CHAINS_LOG2;
            uint32_t k = w >> 10, r = w & 1023u;
            uint32_t tile = IA.shard_rank + k * IA.shard_count;
            uint32_t tx;
            const uint32_t ty = udiv_small(tile, IA.tiles_x, IA.inv_tiles_x, tx);
            uint32_t sub = r >> 6, l = r & 63u;
            uint32_t x = tx * RENE_TILE_SIZE + (sub & 3u) * 8u + (l & 7u);
            uint32_t yi = ty * RENE_TILE_SIZE + (sub >> 2) * 8u + (l >> 3);
            if (x < W && yi < H) {
              ver = (IA.epoch << VERSION_LEVEL_BITS) | (level + 1u);
              px = x;
              py = (H - 1 - yi) | (grp << 16);  // (the chain rides in the row's upper half: pyy() is the row)
              item_frames(KB, IA, level, frame, frame_end);
              chain_frames(KB, grp, frame, frame_end);  // the launch's frames of chain grp: every CHAINS-th one
              if (tile_inactive(IA, k)) frame = frame_end;  // a tile switched off: the empty item (device_code.inc, tile_inactive)
              waiting = true;
              depth = wait_start();  // a lane that waits has no path: its depth register holds when the wait began
            }
          }
        }
      }
      if (ready && phase == PH_NEWPATH && !done) {
        if (waiting) {
          const uint32_t st = item_flag_state(KB, ver, rec_pixel());
          const bool drop = (P.flags & RENE_FLAG_INTERNAL_TEST_DROP) && item_test_drop(px | (py << 16)) && st != ITEM_DONE;  // fault injection (tests)
          if (st == ITEM_READY && !drop) {
            const float* p = reinterpret_cast<const float*>(karg_u64<RENE_KARG(framebuffer)>(KB)) + rec_offset();
            acc0 = fb_load_rgb(p);
            if (AOV) {
              acc1 = fb_load_rgb(p + layer_stride);
              acc2 = fb_load_rgb(p + 2 * layer_stride);
            }
            waiting = false;
          } else if (st == ITEM_DONE) {  // a replayed launch: committed the first time round
            ver = 0u;
            waiting = false;
          } else {  // slow poll + safety net, see render_kernel: a dropped item is rendered by the host's replay of the launch
            if (!__any(phase != PH_NEWPATH)) __builtin_amdgcn_s_sleep(16);
            if (drop || wait_timed_out(depth) || ((iter & 63u) == 0u && wait_abandoned(P))) {
              wait_report(P, KB, px | (pyy() << 14) | ((py >> 16) << 28), ver, flag_load(reinterpret_cast<const uint32_t*>(karg_u64<RENE_KARG(item_done)>(KB)) + rec_pixel()));
              ver = 0u;
              waiting = false;
            }
          }
        }
        if (!waiting && ver != 0u && frame < frame_end) {  // ray generation, lib.rs:174-189
          const uint32_t seed = launch_seed(P, s_stack, frame);
          frame += CHAINS;  // the chain's next frame
          rng = pcg_new((pyy() * W + px) ^ seed);
          fw = pcg_new(seed);
          float u = qdiv((float)px + pcg_f32(rng), (float)(W - 1));  // Q2
          float v = qdiv((float)pyy() + pcg_f32(rng), (float)(H - 1));
          cfloat_ptr cam = (cfloat_ptr)(const void*)L.uni;  // c2w[16], proj_inv[16]
      f3 origin = camera_origin(cam);
          f3 target = m4_point(cam + 16, mk3(u * 2.0f - 1.0f, v * 2.0f - 1.0f, 1.0f));  // camera.rs:77-90
          target = m4_point(cam, target);
          ro = origin;
          rd = normalize(target - origin);
          color = splat(1.0f);
          depth = 0;
          medium_index = 0;  // lib.rs:529
          lc.closest++;
          issue(ro, rd, tmax, false, false);
          phase = PH_CLOSEST;
        }
      }
    }
    if (__all(done) && !__any(q_active)) break;

    // ================================================================================================
    // traversal step: every in-flight query advances by one inner node or one leaf
    // ================================================================================================
    if (COUNT) st_iter++;
    // RENE_WF_POSTPONE (speculative traversal, Aila & Laine 2009): a lane that arrives at a leaf puts it aside (`pleaf`, tested by the
    // next leaf step) and goes on with the stack's top instead of sitting out the iteration's remaining inner-node steps; when it
    // arrives at a second leaf it waits.  Leaves are still tested in the order the traversal finds them and every test sees the
    // distance the tests before it have left, so hits -- ties included -- are those of the plain order; what is speculative are
    // the inner-node visits made before the pending leaf has shortened the ray (counted: node_visits grows by a few per cent).
    // take_leaf: `cur` is a leaf and `pleaf` is free
    auto take_leaf = [&]() {
      pleaf = cur;
      if ((RENE_WF_POSTPONE == 2 || (RENE_WF_POSTPONE == 1 && !q_any)) && sp > 0) {
        if (COUNT) popped = true;
        sp--;
        cur = stack[sp * BLOCK];
      } else {
        cur = CUR_NONE;  // (without speculation: the stack's top is taken after the leaf's test)
      }
    };
    // one inner-node step of every lane that is at one
    auto node_step = [&]() {
      if (COUNT) {
        lc.nodes++;
        if (cur < (q_emit ? S.emit.n_top : S.main.n_top)) ln_top++;
      }
      float t4[4];
      uint32_t w4[4];
      node4_test((q_emit ? S.emit.nodes : S.main.nodes)[cur].q, qo, qinv, tmin, q_tmax, t4, w4);
      if (COUNT) {  // how many visits find nothing, and how many of those were popped (what a distance on the stack would cull)
        const bool dead = !(t4[0] < __builtin_inff());
        ln_dead += dead ? 1u : 0u;
        ln_popped += popped ? 1u : 0u;
        ln_popped_dead += (popped && dead) ? 1u : 0u;
        popped = false;
      }
      if (!node4_descend(t4, w4, stack, sp, cur)) {
        if (sp == 0) {
          if (RENE_WF_POSTPONE) cur = CUR_NONE;
          else q_active = false;
        } else {
          if (COUNT) popped = true;
          sp--;
          cur = stack[sp * BLOCK];
        }
      }
      if (RENE_WF_POSTPONE) {
        if ((cur & LEAF_BIT) && cur != CUR_NONE && pleaf == 0u) take_leaf();
        if (cur == CUR_NONE && pleaf == 0u) q_active = false;
      }
      if (COUNT) sp_max = (uint32_t)sp > sp_max ? (uint32_t)sp : sp_max;
    };
#pragma unroll
    for (int rep = 0; rep < RENE_WF_NODE_STEPS; ++rep) {
      if (COUNT && __any(q_active && !(cur & LEAF_BIT))) st_node++;
      if (COUNT && q_active && !(cur & LEAF_BIT)) ln_rep[rep]++;
      if (q_active && !(cur & LEAF_BIT)) node_step();
    }
    {
      const bool at_leaf = q_active && (RENE_WF_POSTPONE ? pleaf != 0u : (cur & LEAF_BIT) != 0);
      const uint32_t n_leaf = (uint32_t)__popcll(__ballot(at_leaf));
      const uint32_t n_inner = (uint32_t)__popcll(__ballot(q_active && !(cur & LEAF_BIT)));
      if (n_leaf != 0 && (n_leaf >= P.leaf_min || n_inner == 0)) {  // postpone leaves until enough lanes have one
        if (COUNT) {
          st_leaf++;
          if (at_leaf) ln_leaf++;
        }
        if (at_leaf) {
          const PrimIsect* isect = q_emit ? S.emit.isect : S.main.isect;
          const uint32_t leaf = RENE_WF_POSTPONE ? pleaf : cur;
          uint32_t first = leaf & LEAF_FIRST_MASK;
          uint32_t count = ((leaf >> LEAF_COUNT_SHIFT) & 15u) + 1u;
          if (SPHERES && (leaf & SPHERE_BIT)) {
            if (COUNT) lc.prims++;
            intersect_sphere(isect, S.spheres, first, qo, qd, tmin, best, q_tmax);
          } else {
            uint32_t n_tests = 0;
            intersect_leaf(isect, first, count, qo, qd, tmin, best, q_tmax, n_tests);
            if (COUNT) lc.prims += n_tests;
          }
          if (RENE_WF_POSTPONE) {
            pleaf = 0u;
            if (q_any && best.slot != 0xffffffffu) {
              q_active = false;
            } else {
              if (cur == CUR_NONE && sp > 0) {
                if (COUNT) popped = true;
                sp--;
                cur = stack[sp * BLOCK];
              }
              if ((cur & LEAF_BIT) && cur != CUR_NONE) take_leaf();  // the second leaf the lane has been waiting with
              if (cur == CUR_NONE && pleaf == 0u) q_active = false;
            }
          } else if ((q_any && best.slot != 0xffffffffu) || sp == 0) {
            q_active = false;
          } else {
            if (COUNT) popped = true;
            sp--;
            cur = stack[sp * BLOCK];
          }
        }
      }
    }
    // ================================================================================================
    // a lane whose last-light shadow query has completed (PH_LAST_SHADOW, see the logic step): the light's share, then
    // straight on to the query that follows -- or, at the path's end, to the logic step for a new path
    // ================================================================================================
    if ((FEAT & FEAT_LIGHTS) && !VOL && !q_active && phase >= PH_LAST_SHADOW) {
      if (best.slot == 0xffffffffu) {  // lib.rs:260-271
        acc0 = acc0 + pend_light;
        lc.adds++;
      }
      start(phase - PH_LAST_SHADOW);
    }
  }

  wave_stamp(KB, 1);
  clock_probe(P, true);
  // ---- counters: one atomic per wave per counter ---------------------------------------------------
  unsigned long long sums[8] = {wave_sum(lc.closest), wave_sum(lc.shadow), wave_sum(lc.emitter),
                                wave_sum(lc.paths),   wave_sum(lc.hits),   wave_sum(lc.adds),
                                wave_sum(lc.nodes),   wave_sum(lc.prims)};
  if (lane_id() == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (sums[i]) atomicAdd(&P.counters[i], sums[i]);
  }
  if (COUNT) {  // wave-uniform step counts from lane 0, lane counts summed (rene_get_stats prints them under RENE_DEBUG)
    unsigned long long a = wave_sum(ln_leaf), b = wave_sum(ln_logic);
    if (lane_id() == 0) {
      atomicAdd(&P.counters[12], (unsigned long long)st_node);
      atomicAdd(&P.counters[13], (unsigned long long)st_leaf);
      atomicAdd(&P.counters[14], (unsigned long long)st_logic);
      atomicAdd(&P.counters[15], b);
      atomicAdd(&P.counters[16], a);
      atomicAdd(&P.counters[17], (unsigned long long)st_iter);
    }
    unsigned long long c = wave_sum(ln_dead), d = wave_sum(ln_popped), e = wave_sum(ln_popped_dead);
    if (lane_id() == 0) {
      atomicAdd(&P.counters[18], c);
      atomicAdd(&P.counters[19], d);
      atomicAdd(&P.counters[20], e);
    }
    atomicMax(&P.counters[21], (unsigned long long)sp_max);
    unsigned long long g = wave_sum(ln_top);
    if (lane_id() == 0) atomicAdd(&P.counters[22], g);
#pragma unroll
    for (int rep = 0; rep < RENE_WF_NODE_STEPS && rep < 3; ++rep) {
      unsigned long long r = wave_sum(ln_rep[rep]);
      if (lane_id() == 0) atomicAdd(&P.counters[28 + rep], r);
    }
  }
}
