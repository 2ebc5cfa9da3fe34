// wavefront.inc -- the path integrator for BVH scenes as a stage-separated wavefront: path state in HBM,
// one slot per pixel, five kernels per bounce round:
//
//   wave_regen            dead paths start the next frame of their pixel: RNG streams, camera ray
//   wave_trace<false>     closest hit of every live path -> hit record      (persistent waves, lanes refilled
//   wave_shade            miss: background; hit: surface, BSDF, emission +   with the next ray as soon as their
//                         first-hit layers added to the image, the distant   own is done: no lane waits for the
//                         lights' contributions prepared as shadow rays,     slowest of its 63 neighbours)
//                         the next direction sampled
//   wave_trace<true>      shadow rays (any-hit) and emitter-pdf rays of all slots
//   wave_bounce           add the unoccluded light contributions, finish the light/BSDF mixture weight,
//                         zero test, Russian roulette, depth cap
//
// Same device functions, same RNG order and the same fp32 operation order as render_kernel /
// render_kernel_wf (device_code.inc, render_wf.inc): the image is bit-identical to theirs.  A slot is
// bound to one pixel for the whole launch and renders that pixel's frames one after the other, so a
// pixel's sums are still added in the reference's order (frame by frame, bounce by bounce; within a
// bounce: emission, first-hit layers, lights in order -- lib.rs:225-272).  Dead paths are regenerated at
// the top of the next round, so every round works on all unfinished pixels.
//
// Why: the traversal-restart megakernel holds traversal, shading and bookkeeping state at once
// (114-171 VGPRs: 2-4 waves per SIMD) and serves its logic step with as few as 20 of 64 lanes.  Here the
// traversal passes hold a ray and a stack, the shading stages start with all lanes live, and the price is
// the path state's round trip through HBM (~300 bytes per slot and round), which 8 TB/s affords.

enum : uint32_t { WS_ALIVE = 1, WS_NEED_EMIT = 2, WS_HAS_SHADOW = 4, WS_DONE = 8, WS_TAIL = 16 };

// ---- a slot's ray direction and throughput: two float4 (fp32), or -- RENE_FLAG_FP16_PAYLOAD, BASELINE config 5's "fp16 ray
// payload" -- six halves and the pending pdf in ONE float4 (Q.rd; Q.color is then never touched): 16 bytes less per slot
// on every one of the five passes that read or write it.  Halves are rounded toward zero (v_cvt_pkrtz_f16_f32); the
// throughput is clamped to the largest half so that a bright path stays finite.
typedef __fp16 half2v __attribute__((ext_vector_type(2)));
RENE_DEV float pack_h2(float a, float b) {
  const half2v h = __builtin_amdgcn_cvt_pkrtz(a, b);
  return __builtin_bit_cast(float, h);
}
RENE_DEV void unpack_h2(float w, float& a, float& b) {
  const half2v h = __builtin_bit_cast(half2v, w);
  a = (float)h.x;
  b = (float)h.y;
}
RENE_DEV void slot_put(const WaveState& Q, uint32_t i, f3 rd, f3 color, float pdf) {
  if (Q.fp16_payload) {
    const float m = 65504.0f;
    Q.rd[i] = make_float4(pack_h2(rd.x, rd.y), pack_h2(rd.z, fminf(color.x, m)), pack_h2(fminf(color.y, m), fminf(color.z, m)), pdf);
  } else {
    Q.rd[i] = make_float4(rd.x, rd.y, rd.z, 0.0f);
    Q.color[i] = make_float4(color.x, color.y, color.z, pdf);
  }
}
RENE_DEV void slot_get(const WaveState& Q, uint32_t i, f3& rd, f3& color, float& pdf) {
  const float4 b = Q.rd[i];
  if (Q.fp16_payload) {
    unpack_h2(b.x, rd.x, rd.y);
    unpack_h2(b.y, rd.z, color.x);
    unpack_h2(b.z, color.y, color.z);
    pdf = b.w;
  } else {
    const float4 c = Q.color[i];
    rd = mk3(b.x, b.y, b.z);
    color = mk3(c.x, c.y, c.z);
    pdf = c.w;
  }
}
RENE_DEV f3 slot_dir(const WaveState& Q, uint32_t i) {
  const float4 b = Q.rd[i];
  if (!Q.fp16_payload) return mk3(b.x, b.y, b.z);
  f3 rd;
  float unused;
  unpack_h2(b.x, rd.x, rd.y);
  unpack_h2(b.y, rd.z, unused);
  return rd;
}

// slot -> pixel: the item -> pixel map of render_kernel (owned 32x32 tiles, 8x8 micro-tiles inside)
RENE_DEV bool wave_pixel(const SceneView& S, const RenderParams& P, uint32_t w, uint32_t& px, uint32_t& py) {
  uint32_t k = w >> 10, r = w & 1023u;
  uint32_t tile = P.shard_rank + k * P.shard_count;
  uint32_t tx = tile % P.tiles_x, ty = tile / P.tiles_x;
  uint32_t sub = r >> 6, l = r & 63u;
  uint32_t x = tx * RENE_TILE_SIZE + (sub & 3u) * 8u + (l & 7u);
  uint32_t yi = ty * RENE_TILE_SIZE + (sub >> 2) * 8u + (l >> 3);  // image row, top first
  px = x;
  py = S.height - 1u - yi;  // launch_id.y
  return x < S.width && yi < S.height;
}
// (frame chains, device_scene.h: `frames_started` = ctl.w of the slot, the path being rendered is the launch's frame ctl.w - 1 and adds to its chain's
// records -- at the slot itself: a queue slot is the pixel slot of device_scene.h, and the layers are n_slots records apart)
RENE_DEV float* wave_fb(const RenderParams& P, const WaveState& Q, uint32_t slot, uint32_t frames_started) {
  const uint32_t chain = (P.chain_phase + frames_started - 1u) & (CHAINS - 1u);
  return P.framebuffer + ((size_t)chain * 3u * Q.n_slots + slot) * 4;  // add_image target, lib.rs:166
}
RENE_DEV void wave_add(float* p, f3 c) {  // image.write(pos, prev + v), lib.rs:167-171 (alpha untouched)
  f3 v = mk3(p[0], p[1], p[2]);
  v = v + c;
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
}
// Counters without atomics in the round kernels: every wave owns one row of Q.wave_sums and adds its
// totals there (plain read-modify-write: the kernels of a stream run one after the other); wave_finish
// folds the table into the context's counters once per launch.  MASK selects what a kernel can count.
template <uint32_t MASK>
RENE_DEV void wave_counters(const WaveState& Q, const LaneCounters& lc) {
  const uint32_t v[8] = {lc.closest, lc.shadow, lc.emitter, lc.paths, lc.hits, lc.adds, lc.nodes, lc.prims};
  unsigned long long* row = Q.wave_sums + (size_t)(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)) * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (!(MASK & (1u << i))) continue;
    unsigned long long s = wave_sum(v[i]);
    if (lane_id() == 0 && s) row[i] += s;
  }
}
__global__ void __launch_bounds__(BLOCK) wave_finish(RenderParams P, WaveState Q, uint32_t n_rows) {
  uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    unsigned long long s = i < n_rows ? Q.wave_sums[(size_t)i * 8 + k] : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane_id() == 0 && s) atomicAdd(&P.counters[k], s);
  }
}

__global__ void __launch_bounds__(BLOCK) wave_init(WaveState Q) {
  uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= Q.n_slots) return;
  Q.status[i] = 0u;
  Q.ctl[i] = make_uint4(0u, 0u, 0u, 0u);
  if (i == 0) *Q.n_done = 0u;
  if ((i & 63u) == 0u)
    for (int k = 0; k < 8; ++k) Q.wave_sums[(size_t)(i >> 6) * 8 + k] = 0ull;
}

// ---- stage 0: regenerate dead paths (ray generation, lib.rs:174-189) ---------------------------------
template <bool COUNT>
__global__ void __launch_bounds__(BLOCK) wave_regen(SceneView S, RenderParams P, WaveState Q) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  LaneCounters lc;
  if (i == 0) Q.trace_counter[0] = 0u;  // the closest-hit pass that follows starts from id 0
  uint32_t st = i < Q.n_slots ? Q.status[i] : WS_DONE;
  bool newly_done = false;
  if (!(st & (WS_DONE | WS_ALIVE))) {
    uint4 c = Q.ctl[i];
    uint32_t px, py;
    bool inside = wave_pixel(S, P, i, px, py);
    if (!inside || c.w >= P.n_frames) {
      st = WS_DONE;
      newly_done = true;
    } else {
      const uint32_t W = S.width, H = S.height;
      uint32_t seed = frame_seed(P.seed_state0, P.first_frame + c.w * P.frame_stride);
      lc.paths++;
      Pcg rng = pcg_new((py * W + px) ^ seed);
      Pcg fw = pcg_new(seed);
      float u = qdiv((float)px + pcg_f32(rng), (float)(W - 1));  // Q2
      float v = qdiv((float)py + pcg_f32(rng), (float)(H - 1));
      cfloat_ptr cam = (cfloat_ptr)(const void*)S.uni;  // c2w[16], proj_inv[16]
      f3 origin = camera_origin(cam);
      f3 target = m4_point(cam + 16, mk3(u * 2.0f - 1.0f, v * 2.0f - 1.0f, 1.0f));  // camera.rs:77-90
      target = m4_point(cam, target);
      f3 rd = normalize(target - origin);
      Q.ro[i] = make_float4(origin.x, origin.y, origin.z, 0.0f);
      slot_put(Q, i, rd, splat(1.0f), 0.0f);
      Q.ctl[i] = make_uint4(rng.state, fw.state, 0u, c.w + 1u);
      st = WS_ALIVE;
    }
    Q.status[i] = st;
  }
  unsigned long long m = __ballot(newly_done);
  if (m != 0ull && lane_id() == 0) atomicAdd(Q.n_done, (uint32_t)__popcll(m));
  wave_counters<0x08u>(Q, lc);  // paths
}

// ---- traversal passes: persistent waves, every lane refilled with the next ray as soon as its own is done
// (the rays of a pass are independent, so no lane waits for the slowest of its 63 neighbours).
//   SECONDARY = false: ray id = slot; the closest hit of every live path -> Q.hit
//   SECONDARY = true : ray id = light * n_slots + slot: shadow ray of that light (any-hit) -> occluded flag in
//                      Q.sh_wi[..].w; ids from max_lights * n_slots on: the emitter-pdf ray of the slot
//                      (closest hit in the emitter-only structure, Q5) -> pdf_l in Q.hit[slot].x
constexpr uint32_t WAVE_ID_BATCH = 256;  // ray ids a wave takes per global atomic
template <bool SECONDARY, bool SPHERES, bool COUNT>
__global__ void __launch_bounds__(BLOCK) wave_trace(SceneView S, RenderParams P, WaveState Q, uint32_t n_ids, uint32_t static_waves) {
  extern __shared__ uint32_t s_stack[];  // [stack depth][BLOCK]
  uint32_t* stack = s_stack + threadIdx.x;
  LaneCounters lc;
  const float tmin = 0.001f;
  // ray query (render_wf.inc)
  bool q_active = false, q_any = false, q_emit = false;
  f3 qo = splat(0.0f), qd = splat(0.0f), qinv = splat(0.0f);
  float q_tmax = 0.0f;
  uint32_t cur = 0, q_id = 0;
  int sp = 0;
  HitRec best;
  best.t = best.u = best.v = 0.0f;
  best.slot = 0xffffffffu;
  // wave-uniform batch of ray ids; the first batch of every co-resident wave is static (first_batch)
  uint32_t batch_next = 0, batch_end = 0;
  bool exhausted = false;
  uint32_t* counter = Q.trace_counter + (SECONDARY ? 1 : 0);
  {
    uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)));
    if (wave < static_waves && wave * WAVE_ID_BATCH < n_ids) {
      batch_next = wave * WAVE_ID_BATCH;
      batch_end = batch_next + WAVE_ID_BATCH < n_ids ? batch_next + WAVE_ID_BATCH : n_ids;
    }
  }
  const uint32_t n = Q.n_slots;
  for (;;) {
    // ---- refill idle lanes ----
    const unsigned long long idle_mask = __ballot(!q_active);
    const uint32_t n_idle = (uint32_t)__popcll(idle_mask);
    bool more = batch_next < batch_end || !exhausted;
    if (more && (n_idle >= P.ready_min || n_idle == 64u)) {
      if (batch_next >= batch_end) {
        uint32_t base = 0;
        if (lane_id() == 0) base = atomicAdd(counter, WAVE_ID_BATCH);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base) + static_waves * WAVE_ID_BATCH;
        if (base >= n_ids) {
          exhausted = true;
        } else {
          batch_next = base;
          batch_end = base + WAVE_ID_BATCH < n_ids ? base + WAVE_ID_BATCH : n_ids;
        }
      }
      uint32_t rank = (uint32_t)__popcll(idle_mask & ((1ull << lane_id()) - 1ull));
      uint32_t id = batch_next + rank;
      bool got = !q_active && id < batch_end;
      batch_next = batch_next + n_idle < batch_end ? batch_next + n_idle : batch_end;
      if (got) {
        uint32_t slot = id, l = 0;
        if (SECONDARY) {
          while (slot >= n) {
            slot -= n;
            l++;
          }
        }
        const uint32_t st = Q.status[slot];
        bool valid;
        if (!SECONDARY) valid = (st & WS_ALIVE) && !(st & WS_DONE);
        else valid = l < Q.max_lights ? (st & WS_HAS_SHADOW) != 0 : (st & WS_NEED_EMIT) != 0;
        if (valid) {
          float4 a = Q.ro[slot];
          qo = mk3(a.x, a.y, a.z);
          if (SECONDARY && l < Q.max_lights) {
            const float4 b = Q.sh_wi[(size_t)l * n + slot];
            qd = mk3(b.x, b.y, b.z);
          } else {
            qd = slot_dir(Q, slot);
          }
          qinv = safe_inv(qd);
          q_any = SECONDARY && l < Q.max_lights;
          q_emit = SECONDARY && l >= Q.max_lights;
          q_tmax = q_any ? 1e5f : 100000.0f;
          q_id = id;
          cur = 0;
          sp = 0;
          best.slot = 0xffffffffu;
          q_active = true;
          if (!SECONDARY) lc.closest++;
          else if (q_any) lc.shadow++;
          else lc.emitter++;
        }
      }
      more = batch_next < batch_end || !exhausted;
    }
    if (!more && !__any(q_active)) break;

    // ---- one traversal step per in-flight ray: an inner node ... ----
    bool finished = false;
    if (q_active) {
      const Node* nodes = q_emit ? S.emit.nodes : S.main.nodes;
      if (!(cur & LEAF_BIT)) {
        if (COUNT) lc.nodes++;
        float t4[4];
        uint32_t w4[4];
        node4_test(nodes[cur].q, qo, qinv, tmin, q_tmax, t4, w4);
        if (!node4_descend(t4, w4, stack, sp, cur)) {
          if (sp == 0) {
            finished = true;
          } else {
            sp--;
            cur = stack[sp * BLOCK];
          }
        }
      }
    }
    // ---- ... or a leaf, postponed until enough lanes have one ----
    {
      const bool at_leaf = q_active && !finished && (cur & LEAF_BIT) != 0;
      const uint32_t n_leaf = (uint32_t)__popcll(__ballot(at_leaf));
      const uint32_t n_inner = (uint32_t)__popcll(__ballot(q_active && !finished && !(cur & LEAF_BIT)));
      if (n_leaf != 0 && (n_leaf >= P.leaf_min || n_inner == 0)) {
        if (at_leaf) {
          const PrimIsect* isect = q_emit ? S.emit.isect : S.main.isect;
          uint32_t first = cur & LEAF_FIRST_MASK;
          uint32_t count = ((cur >> LEAF_COUNT_SHIFT) & 15u) + 1u;
          if (SPHERES && (cur & SPHERE_BIT)) {
            if (COUNT) lc.prims++;
            intersect_sphere(isect, S.spheres, first, qo, qd, tmin, best, q_tmax);
          } else {
            uint32_t n_tests = 0;
            intersect_leaf(isect, first, count, qo, qd, tmin, best, q_tmax, n_tests);
            if (COUNT) lc.prims += n_tests;
          }
          if ((q_any && best.slot != 0xffffffffu) || sp == 0) {
            finished = true;
          } else {
            sp--;
            cur = stack[sp * BLOCK];
          }
        }
      }
    }
    // ---- a finished ray hands its result to the slot and frees the lane ----
    if (finished) {
      q_active = false;
      if (!SECONDARY) {
        Q.hit[q_id] = make_float4(best.t, best.u, best.v, __uint_as_float(best.slot));
      } else if (q_any) {
        uint32_t slot = q_id, l = 0;
        while (slot >= n) {
          slot -= n;
          l++;
        }
        Q.sh_wi[(size_t)l * n + slot].w = best.slot != 0xffffffffu ? 1.0f : 0.0f;  // occluded
      } else {
        uint32_t slot = q_id - Q.max_lights * n;
        Q.hit[slot].x = emitter_pdf<SPHERES>(S, best, qo, qd);
      }
    }
  }
  wave_counters<SECONDARY ? (COUNT ? 0xc6u : 0x06u) : (COUNT ? 0xc1u : 0x01u)>(Q, lc);
}

template <uint32_t FEAT, int MAXL, bool COUNT, bool AOV>
__global__ void __launch_bounds__(BLOCK) wave_shade(SceneView S, RenderParams P, WaveState Q) {
  constexpr bool SPHERES = (FEAT & FEAT_SPHERES) != 0;
  constexpr uint32_t GENERAL = lobe_kinds(FEAT);  // 0: Matte only
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  LaneCounters lc;
  if (i == 0) Q.trace_counter[1] = 0u;  // the secondary-ray pass that follows starts from id 0
  uint32_t st = i < Q.n_slots ? Q.status[i] : WS_DONE;
  if ((st & WS_ALIVE) && !(st & WS_DONE)) {
    const size_t layer_stride = (size_t)Q.n_slots * 4;
    float4 a = Q.ro[i], hh = Q.hit[i];
    uint4 ctl = Q.ctl[i];
    float* fb = wave_fb(P, Q, i, ctl.w);
    f3 ro = mk3(a.x, a.y, a.z), rd, color;
    float pdf_in_slot;
    slot_get(Q, i, rd, color, pdf_in_slot);
    Pcg rng{ctl.x}, fw{ctl.y};
    const uint32_t depth = ctl.z;
    HitRec hit{hh.x, hh.y, hh.z, __float_as_uint(hh.w)};
    if (hit.slot == 0xffffffffu) {  // main_miss, lib.rs:120-139, 209-211
      f3 bg = splat(0.0f);
      if (FEAT & FEAT_BACKGROUND) {
        uv2 uv = sphere_uv(normalize(m4_vector(S.uni->bg_matrix, rd)));
        bg = mk3(S.uni->bg_color[0], S.uni->bg_color[1], S.uni->bg_color[2]) * tex_color<FEAT | FEAT_TEXTURES>(S, S.bg_texture, uv);
      }
      wave_add(fb, color * bg);
      lc.adds++;
      st = 0u;
    } else {
      lc.hits++;
      Surface sf = shade_hit<SPHERES>(S, hit, ro, rd);
      const Inst& inst = S.insts[sf.instance];
      f3 wo = -normalize(rd);
      f3 normal = normalize(sf.normal);
      f3 position = sf.position;
      Bsdf<MAXL> bsdf;
      bsdf.len = 0;
      bsdf.codes = 0xffffffffu;
      bsdf.ng = normal;
      bsdf.onb = onb_from_w(normal);
      compute_bsdf<FEAT, MAXL>(S, inst, sf.uv, bsdf);
      if (inst.emit[3] != 0.0f) {  // lib.rs:225-227, area_light.rs:66-74
        f3 e = dot(wo, normal) > 0.0f ? mk3(inst.emit[0], inst.emit[1], inst.emit[2]) : splat(0.0f);
        wave_add(fb, color * e);
        lc.adds++;
      }
      if (depth == 0u) {  // lib.rs:229-232
        if (AOV) {
          wave_add(fb + layer_stride, normal);
          wave_add(fb + 2 * layer_stride, material_albedo<FEAT>(S, inst, sf.uv));
        }
        lc.adds += 2;
      }
      st = WS_ALIVE | WS_TAIL;
      if (FEAT & FEAT_LIGHTS) {  // lib.rs:234-272: the add happens in wave_bounce if the shadow ray escapes
        for (uint32_t li = 0; li < S.lights_len; ++li) {
          float4 ld = ldg4(S.lights[li].dir), lL = ldg4(S.lights[li].L);
          f3 wi = normalize((position + mk3(ld.x, ld.y, ld.z)) - position);  // light.rs:52-55
          f3 f = bsdf_f<MAXL, GENERAL>(bsdf, wo, wi);
          f3 c = color * f * fabsf(dot(wi, normal)) * mk3(lL.x, lL.y, lL.z);
          Q.sh_wi[(size_t)li * Q.n_slots + i] = make_float4(wi.x, wi.y, wi.z, 0.0f);
          Q.sh_c[(size_t)li * Q.n_slots + i] = make_float4(c.x, c.y, c.z, 0.0f);
        }
        if (S.lights_len) st |= WS_HAS_SHADOW;
      }
      float pend_pdf = 0.0f;
      if (S.emit_object_len > 0 && bsdf_contains<MAXL, GENERAL>(bsdf, K_DIFFUSE)) {  // lib.rs:274-314
        f3 wi, f;
        float pdf;
        if (pcg_f32(fw) > 0.5f) {  // Q3: frame-wide stream
          uint32_t obj = umod(pcg_u32(fw), S.emit_object_len);
          wi = normalize(emit_sample<SPHERES>(S, obj, fw) - position);
          pdf = bsdf_pdf<MAXL, GENERAL>(bsdf, wi, normal);  // Q1: (wi, normal), lib.rs:287
          f = bsdf_f<MAXL, GENERAL>(bsdf, wo, wi);
        } else {
          Sampled s = bsdf_sample<MAXL, GENERAL>(bsdf, wo, rng);
          wi = s.wi;
          pdf = s.pdf;
          f = s.f;
        }
        rd = wi;
        f3 pend_f = f * fabsf(dot(normal, wi));
        color = color * pend_f;  // lib.rs:316; the division by the mixture pdf follows the emitter-pdf ray
        pend_pdf = pdf;
        st |= WS_NEED_EMIT;
      } else {  // lib.rs:325-337
        Sampled s = bsdf_sample<MAXL, GENERAL>(bsdf, wo, rng);
        if (s.pdf < 1e-5f) {
          st &= ~WS_ALIVE;
        } else {
          color = color * (s.f * qdiv(fabsf(dot(normal, s.wi)), s.pdf));
          rd = s.wi;
        }
      }
      Q.ro[i] = make_float4(position.x, position.y, position.z, 0.0f);  // also the shadow rays' origin
      slot_put(Q, i, rd, color, pend_pdf);
      Q.ctl[i] = make_uint4(rng.state, fw.state, depth, ctl.w);
    }
    Q.status[i] = st;
  }
  wave_counters<0x30u>(Q, lc);  // hits, adds
}

// ---- last stage of a round: consume the secondary rays' results, finish the bounce (lib.rs:260-355) ----
__global__ void __launch_bounds__(BLOCK) wave_bounce(SceneView S, RenderParams P, WaveState Q) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  LaneCounters lc;
  uint32_t st = i < Q.n_slots ? Q.status[i] : 0u;
  if (st & WS_TAIL) {
    if (st & WS_HAS_SHADOW) {  // lib.rs:260-271, lights in order
      float* fb = wave_fb(P, Q, i, Q.ctl[i].w);
      for (uint32_t li = 0; li < S.lights_len; ++li) {
        if (Q.sh_wi[(size_t)li * Q.n_slots + i].w == 0.0f) {
          float4 c = Q.sh_c[(size_t)li * Q.n_slots + i];
          wave_add(fb, mk3(c.x, c.y, c.z));
          lc.adds++;
        }
      }
    }
    bool alive = (st & WS_ALIVE) != 0;
    f3 slot_rd, color;
    float slot_pdf;
    slot_get(Q, i, slot_rd, color, slot_pdf);
    if (st & WS_NEED_EMIT) {  // lib.rs:301-324
      float pdf_l = Q.hit[i].x;
      float pdf = 0.5f * slot_pdf + qdiv(0.5f * pdf_l, (float)S.emit_object_len);
      if (pdf < 1e-5f) alive = false;
      else color = color / pdf;
    }
    uint4 ctl = Q.ctl[i];
    Pcg fw{ctl.y};
    uint32_t depth = ctl.z;
    if (alive && is_zero(color)) alive = false;  // lib.rs:340-342
    if (alive && depth > 12u) {                  // lib.rs:345-354
      float rr_coin = pcg_f32(fw);
      float continue_p = max_element(color);
      if (rr_coin > continue_p) alive = false;
      else color = color / continue_p;
    }
    depth++;
    if (depth >= 50u) alive = false;  // lib.rs:192 (Q7)
    if (alive) {
      if (Q.fp16_payload) slot_put(Q, i, slot_rd, color, 0.0f);
      else Q.color[i] = make_float4(color.x, color.y, color.z, 0.0f);
      Q.ctl[i] = make_uint4(ctl.x, fw.state, depth, ctl.w);
    }
    Q.status[i] = alive ? WS_ALIVE : 0u;
  }
  wave_counters<0x20u>(Q, lc);  // adds
}
