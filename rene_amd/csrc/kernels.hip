// kernels.hip -- launch wrappers + the small kernels (trace, BSDF probe) + the render kernels of the
// small-scene family, and the one launcher of every render kernel (kernel_select.h decides which).  The BVH family is instantiated in
// kernels_bvh.hip, the volumetric integrator's kernels in kernels_vol.hip.  All device code lives in device_code.inc / render_wf.inc.
#include "device_code.inc"

// -------------------------------------------------------------------------------------------------
// batch closest-hit queries (rene_trace): one lane per ray
// -------------------------------------------------------------------------------------------------
template <bool SMALL>
__global__ void __launch_bounds__(BLOCK) trace_kernel(SceneView S, int which, uint32_t n, const float* o3,
                                                      const float* d3, float tmin, float tmax, rene_hit* out) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = i < n;
  if (!live) i = n - 1;  // keep the wave converged for the coherent item loop
  LaneCounters lc;
  f3 o = mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
  const Accel& A = which ? S.emit : S.main;
  HitRec h = trace_accel<SMALL, false, true, false>(A, S.spheres, o, d, tmin, tmax, stack, lc);
  if (!live) return;
  rene_hit r;
  if (h.slot == 0xffffffffu) {
    r.t = -1.0f; r.u = 0.0f; r.v = 0.0f; r.instance = 0; r.primitive = 0;
  } else {
    const float* q = A.isect[h.slot].q;
    r.t = h.t; r.u = h.u; r.v = h.v;
    r.instance = __float_as_uint(q[9]);
    r.primitive = __float_as_uint(q[10]);
  }
  out[i] = r;
}

// -------------------------------------------------------------------------------------------------
// emitter-pdf probe (rene_emitter_pdf): the query of lib.rs:301-318 for a batch of rays, one lane per ray
// -------------------------------------------------------------------------------------------------
template <bool SMALL>
__global__ void __launch_bounds__(BLOCK) emitter_pdf_kernel(SceneView S, uint32_t n, const float* o3, const float* d3, float* out) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = i < n;
  if (!live) i = n - 1;  // keep the wave converged for the coherent item loop
  LaneCounters lc;
  f3 o = mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
  HitRec h = trace_accel<SMALL, false, true, false>(S.emit, S.spheres, o, d, 0.001f, 100000.0f, stack, lc);
  const float pdf = emitter_pdf<true>(S, h, o, d);
  if (live) out[i] = pdf;
}
hipError_t launch_emitter_pdf(const LaunchConfig& cfg, const SceneView& S, uint32_t n, const float* o, const float* d, float* out, hipStream_t st) {
  size_t lds = (size_t)cfg.stack_depth * BLOCK * sizeof(uint32_t);
  dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
  if (cfg.features & FEAT_SMALL) hipLaunchKernelGGL(emitter_pdf_kernel<true>, grid, block, 0, st, S, n, o, d, out);
  else hipLaunchKernelGGL(emitter_pdf_kernel<false>, grid, block, lds, st, S, n, o, d, out);
  return hipGetLastError();
}

// the same query over the LDS image (rene_emitter_pdf_form, forms 1 and 2): what the small-scene render kernels run -- the item loop with the
// winning item's look-up in LDS, then emitter_pdf_lds.  NORMALISED: the direction is normalised first and handed on as it is (SHARED_RD)
template <bool NORMALISED>
__global__ void __launch_bounds__(BLOCK) emitter_pdf_lds_kernel(SceneView S, uint32_t n, const float* o3, const float* d3, float* out) {
  extern __shared__ uint32_t s_stack[];
  small_lds_fill(S, s_stack);
  const SmallLds T = small_lds(S, s_stack);
  __syncthreads();
  uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = i < n;
  if (!live) i = n - 1;  // keep the wave converged for the coherent item loop
  LaneCounters lc;
  f3 o = mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
  if (NORMALISED) d = normalize(d);
  HitRec h = traverse_small<false, true, false, true>(S.emit, S.spheres, o, d, 0.001f, 100000.0f, lc, T.items_emit);
  const float pdf = emitter_pdf_lds<true, NORMALISED>(S, T, h, o, d);
  if (live) out[i] = pdf;
}
hipError_t launch_emitter_pdf_lds(const SceneView& S, bool normalised, uint32_t n, const float* o, const float* d, float* out, hipStream_t st) {
  dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
  if (normalised) hipLaunchKernelGGL(emitter_pdf_lds_kernel<true>, grid, block, S.small_bytes, st, S, n, o, d, out);
  else hipLaunchKernelGGL(emitter_pdf_lds_kernel<false>, grid, block, S.small_bytes, st, S, n, o, d, out);
  return hipGetLastError();
}

// emitter-point probe (rene_emit_sample): fw = PCG32si::new(seed), the object, the point, the stream's next word; out[8] per item.
// LDS: emit_sample_lds over the LDS image instead of emit_sample over the global tables
template <bool LDS>
__global__ void __launch_bounds__(BLOCK) emit_sample_kernel(SceneView S, uint32_t n, const uint32_t* seeds, float* out) {
  extern __shared__ uint32_t s_stack[];
  SmallLds T{};
  if constexpr (LDS) {
    small_lds_fill(S, s_stack);
    T = small_lds(S, s_stack);
    __syncthreads();
  }
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  Pcg fw = pcg_new(seeds[i]);
  const uint32_t obj = umod(pcg_u32(fw), S.emit_object_len);
  f3 p;
  if constexpr (LDS) p = emit_sample_lds<true>(T, obj, fw);
  else p = emit_sample<true>(S, obj, fw);
  float* q = out + 8 * (size_t)i;
  q[0] = p.x; q[1] = p.y; q[2] = p.z; q[3] = __uint_as_float(obj);
  q[4] = __uint_as_float(pcg_u32(fw)); q[5] = 0.0f; q[6] = 0.0f; q[7] = 0.0f;
}
hipError_t launch_emit_sample(const SceneView& S, bool lds, uint32_t n, const uint32_t* seeds, float* out8, hipStream_t st) {
  dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
  if (lds) hipLaunchKernelGGL(emit_sample_kernel<true>, grid, block, S.small_bytes, st, S, n, seeds, out8);
  else hipLaunchKernelGGL(emit_sample_kernel<false>, grid, block, 0, st, S, n, seeds, out8);
  return hipGetLastError();
}

// PCG32si on the device (rene_pcg_probe): one lane, n outputs
__global__ void pcg_probe_kernel(uint32_t seed, uint32_t n, uint32_t* out) {
  Pcg r = pcg_new(seed);
  for (uint32_t k = 0; k < n; ++k) out[k] = pcg_u32(r);
}
hipError_t launch_pcg_probe(uint32_t seed, uint32_t n, uint32_t* out, hipStream_t st) {
  hipLaunchKernelGGL(pcg_probe_kernel, dim3(1), dim3(1), 0, st, seed, n, out);
  return hipGetLastError();
}

// The frame-wide sample stream of a launch's frames as a table (device_scene.h, FRAME_STREAM_*): one thread per launch frame, seeded as
// launch_seed + pcg_new seed a path of that frame, walks depths 0 .. 49 (device_code.inc, frame_stream_row).  Runs on the context's stream
// directly before every persistent launch that reads the table -- 50 short steps of a few hundred threads against a launch of milliseconds --
// and again before a replay of that launch: the context has ONE table and a later launch of the same drain interval has refilled it.
__global__ void __launch_bounds__(64) frame_stream_fill_kernel(SceneView S, uint32_t seed_state0, uint32_t first_frame, uint32_t frame_stride,
                                                               uint32_t n_frames, float4* table) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_frames) return;
  frame_stream_row<false>(S, frame_seed(seed_state0, first_frame + i * frame_stride), table + ((size_t)i << FRAME_STREAM_STRIDE_LOG2));
}
hipError_t launch_frame_stream_fill(const SceneView& S, uint32_t seed_state0, uint32_t first_frame, uint32_t frame_stride, uint32_t n_frames,
                                    float* table, hipStream_t st) {
  if (n_frames == 0) return hipSuccess;
  hipLaunchKernelGGL(frame_stream_fill_kernel, dim3((n_frames + 63u) / 64u), dim3(64), 0, st, S, seed_state0, first_frame, frame_stride, n_frames,
                     reinterpret_cast<float4*>(table));
  return hipGetLastError();
}

// (resolve_chains_kernel, the frame chains added into the image a call hands out, lives in kernels_mean.hip: its sums keep denormals)

// owned tiles <-> packed buffer (rene_gather_tiles): one thread per (owned tile, layer, texel), 16 bytes each
__global__ void __launch_bounds__(BLOCK) pack_tiles_kernel(float* fb, float* packed, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_owned,
                                                            uint32_t shard_rank, uint32_t shard_count, bool unpack) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;  // ((k * 3 + layer) * 32 + ty) * 32 + tx
  if (i >= (size_t)n_owned * 3u * RENE_TILE_SIZE * RENE_TILE_SIZE) return;
  const uint32_t tx = (uint32_t)(i & 31u), ty = (uint32_t)((i >> 5) & 31u);
  const uint32_t kl = (uint32_t)(i >> 10), layer = kl % 3u, k = kl / 3u;
  const uint32_t tile = shard_rank + k * shard_count;
  const uint32_t x = (tile % tiles_x) * RENE_TILE_SIZE + tx, y = (tile / tiles_x) * RENE_TILE_SIZE + ty;
  float4* p = reinterpret_cast<float4*>(packed) + i;
  if (x < W && y < H) {
    float4* f = reinterpret_cast<float4*>(fb) + ((size_t)layer * H + y) * W + x;
    if (unpack) *f = *p;
    else *p = *f;
  } else if (!unpack) {
    *p = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
hipError_t launch_pack_tiles(const float* fb, float* packed, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t n_tiles,
                             uint32_t shard_rank, uint32_t shard_count, bool unpack, hipStream_t st) {
  const uint32_t n_owned = n_tiles > shard_rank ? (n_tiles - shard_rank + shard_count - 1) / shard_count : 0;
  if (n_owned == 0) return hipSuccess;
  const size_t n = (size_t)n_owned * 3u * RENE_TILE_SIZE * RENE_TILE_SIZE;
  hipLaunchKernelGGL(pack_tiles_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, const_cast<float*>(fb), packed, width, height, tiles_x,
                     n_owned, shard_rank, shard_count, unpack);
  return hipGetLastError();
}

// -------------------------------------------------------------------------------------------------
// per-function BSDF probe (rene_bsdf_eval): builds the material's lobes at (normal, uv) exactly like
// the integrator does and returns f(wo,wi), pdf(wo,wi) and one sample_f(wo) drawn from
// PCG32si::new(seed).  out[12] = f.xyz, pdf, s.wi.xyz, s.f.xyz, s.pdf, len
// -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) bsdf_eval_kernel(SceneView S, uint32_t material, int inst_index, uint32_t n, const float* nrm3,
                                                       const float* uv2_, const float* wo3, const float* wi3,
                                                       const uint32_t* seeds, float* out) {
  constexpr uint32_t ALL = FEAT_SPHERES | FEAT_GENERAL_BSDF | FEAT_TEXTURES | FEAT_LIGHTS | FEAT_BACKGROUND | FEAT_MULTI_LOBE;
  uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Inst inst;
  if (inst_index >= 0) {
    inst = S.insts[inst_index];
  } else {
    inst.material = material;
    inst.area_light = 0;
    inst.primitive_count = 1.0f;
    inst.material_type = S.materials[material].type;
    inst.kd[0] = inst.kd[1] = inst.kd[2] = inst.kd[3] = 0.0f;
    inst.emit[0] = inst.emit[1] = inst.emit[2] = inst.emit[3] = 0.0f;
    inst.res_type = 0u;
  }
  f3 normal = normalize(mk3(nrm3[3 * i], nrm3[3 * i + 1], nrm3[3 * i + 2]));
  Bsdf<5> b;
  b.len = 0;
  b.codes = 0xffffffffu;
  b.ng = normal;
  b.onb = onb_from_w(normal);
  compute_bsdf<ALL, 5>(S, inst, uv2{uv2_[2 * i], uv2_[2 * i + 1]}, b);
  f3 wo = mk3(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]), wi = mk3(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]);
  constexpr uint32_t KINDS = lobe_kinds(ALL);  // every lobe kind
  f3 f = bsdf_f<5, KINDS>(b, wo, wi);
  float p = b.len ? bsdf_pdf<5, KINDS>(b, wo, wi) : 0.0f;
  Pcg rng = pcg_new(seeds[i]);
  Sampled sf = bsdf_sample<5, KINDS>(b, wo, rng);
  float* o = out + 12 * (size_t)i;
  o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = p;
  o[4] = sf.wi.x; o[5] = sf.wi.y; o[6] = sf.wi.z;
  o[7] = sf.f.x; o[8] = sf.f.y; o[9] = sf.f.z; o[10] = sf.pdf; o[11] = (float)b.len;
}

hipError_t launch_bsdf_eval(const SceneView& S, uint32_t material, int inst_index, uint32_t n, const float* nrm3, const float* uv,
                            const float* wo3, const float* wi3, const uint32_t* seeds, float* out, hipStream_t st) {
  hipLaunchKernelGGL(bsdf_eval_kernel, dim3((n + 63) / 64), dim3(64), 0, st, S, material, inst_index, n, nrm3, uv, wo3, wi3, seeds, out);
  return hipGetLastError();
}

// per-function medium probe (rene_medium_eval), layout in include/rene_hip.h
__global__ void __launch_bounds__(64) medium_eval_kernel(SceneView S, uint32_t medium, uint32_t n, const float* rd3,
                                                         const float* t_max, const float* wo3, const float* wi3,
                                                         const uint32_t* seeds, float* out) {
  uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  MediumRec m = load_medium(S, medium);
  f3 rd = mk3(rd3[3 * i], rd3[3 * i + 1], rd3[3 * i + 2]);
  f3 wo = mk3(wo3[3 * i], wo3[3 * i + 1], wo3[3 * i + 2]), wi = mk3(wi3[3 * i], wi3[3 * i + 1], wi3[3 * i + 2]);
  float* o = out + 16 * (size_t)i;
  const bool vac = m.type == RENE_MEDIUM_VACUUM;  // EnumMedium dispatch, medium.rs:180-208
  f3 tr = vac ? splat(1.0f) : medium_tr(m, rd, t_max[i]);
  Pcg rng = pcg_new(seeds[i]);
  SampledMedium sm{false, splat(0.0f), splat(1.0f)};
  if (!vac) sm = medium_sample(m, splat(0.0f), rd, t_max[i], rng);
  f3 p = vac ? splat(0.0f) : medium_sample_p(m, wo, rng);
  o[0] = tr.x; o[1] = tr.y; o[2] = tr.z; o[3] = vac ? 0.0f : medium_phase(m, wo, wi);
  o[4] = sm.sampled ? 1.0f : 0.0f; o[5] = sm.position.x; o[6] = sm.position.y; o[7] = sm.position.z;
  o[8] = sm.tr.x; o[9] = sm.tr.y; o[10] = sm.tr.z; o[11] = p.x; o[12] = p.y; o[13] = p.z;
  o[14] = __uint_as_float(pcg_u32(rng)); o[15] = 0.0f;
}

hipError_t launch_medium_eval(const SceneView& S, uint32_t medium, uint32_t n, const float* rd3, const float* t_max,
                              const float* wo3, const float* wi3, const uint32_t* seeds, float* out, hipStream_t st) {
  hipLaunchKernelGGL(medium_eval_kernel, dim3((n + 63) / 64), dim3(64), 0, st, S, medium, n, rd3, t_max, wo3, wi3, seeds, out);
  return hipGetLastError();
}

// probe of the transmittance walks (rene_transmittance): one lane per ray, tr.rgb and the queries the walk traced
template <bool SMALL, bool EMIT>
__global__ void __launch_bounds__(BLOCK) transmittance_kernel(SceneView S, uint32_t medium, uint32_t n, const float* o3, const float* d3, float* out) {
  extern __shared__ uint32_t s_stack[];
  uint32_t* stack = s_stack + threadIdx.x;
  uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = i < n;
  if (!live) i = n - 1;  // keep the wave converged for the coherent item loop
  LaneCounters lc;
  f3 o = mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
  f3 tr = transmittance<SMALL, true, false, EMIT>(S, o, d, medium, stack, lc);
  if (!live) return;
  float* q = out + 4 * (size_t)i;
  q[0] = tr.x; q[1] = tr.y; q[2] = tr.z; q[3] = (float)lc.shadow;
}

hipError_t launch_transmittance(const LaunchConfig& cfg, const SceneView& S, bool emit, uint32_t medium, uint32_t n, const float* o, const float* d,
                                float* out4, hipStream_t st) {
  size_t lds = (size_t)cfg.stack_depth * BLOCK * sizeof(uint32_t);
  dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
  if (cfg.features & FEAT_SMALL) {
    if (emit) hipLaunchKernelGGL((transmittance_kernel<true, true>), grid, block, 0, st, S, medium, n, o, d, out4);
    else hipLaunchKernelGGL((transmittance_kernel<true, false>), grid, block, 0, st, S, medium, n, o, d, out4);
  } else {
    if (emit) hipLaunchKernelGGL((transmittance_kernel<false, true>), grid, block, lds, st, S, medium, n, o, d, out4);
    else hipLaunchKernelGGL((transmittance_kernel<false, false>), grid, block, lds, st, S, medium, n, o, d, out4);
  }
  return hipGetLastError();
}

// ---- host-side dispatch of the render kernels ----------------------------------------------------
// the path integrator's item-loop family (small scenes) is instantiated in this translation unit: every leaf, once
static RenderKernel item_render_kernel(const KernelChoice& k) {
  constexpr uint32_t METAL = FEAT_SPHERES | FEAT_GENERAL_BSDF | FEAT_SMALL, GEN1 = shade_feat(ShadeClass::Single) | FEAT_SMALL;
  // (FEAT_SMALL alone: Matte, triangle emitters only -- Cornell; Metal the only general material: veach-mis)
  return find_leaf<FEAT_SMALL, FEAT_LIGHTS | FEAT_SMALL, METAL | FEAT_NO_SPECULAR | FEAT_NO_BLEND, METAL, GEN1, FEAT_ALL | FEAT_SMALL>(k);
}
// the launch of a persistent render kernel, whatever its family
static hipError_t launch_kernel(const KernelChoice& k, RenderKernel kernel, const LaunchConfig& cfg, const SceneView& S, const RenderParams& P0, hipStream_t st) {
  if (!kernel) return hipErrorInvalidDeviceFunction;  // a choice no unit instantiates is an error, not a reason to launch something else
  dim3 grid(cfg.grid), block(BLOCK);
  RenderParams P = P0;
  SceneView V = S;
  V.lds_insts = k.lds_insts;
  if (k.stack_entries) P.stack_entries = cfg.stack_depth;
  // what the kernel keeps in LDS (the scene's LDS image, device_scene.h, or the traversal stack and the tables behind it) + the launch's seed tables
  // ... + the prepared path starts of the kernels that keep them (device_code.inc, RENE_START_SLOT), a column of START_SLOT_DWORDS words per lane
  size_t lds = k.lds;
  const size_t slot_bytes = k.family == KernelFamily::ItemLoop ? start_slot_bytes(k.feat) : 0u;
  seed_tables_place(P, lds, slot_bytes);
  P.start_slot = (uint32_t)(lds / 4u);
  lds += slot_bytes;
  if (k.family == KernelFamily::ItemLoop && !(k.feat & FEAT_VOLPATH)) {
    static const size_t lds_pad = std::getenv("RENE_LDS_PAD") ? (size_t)std::atoi(std::getenv("RENE_LDS_PAD")) : 0;  // occupancy experiments
    lds += lds_pad;
  }
  fit_grid(kernel, lds, cfg, P, grid);
  if (k.reads_frame_stream) {  // a missing table is an error, not a reason to read through a null pointer
    if (!P.frame_stream) return hipErrorInvalidValue;
    const hipError_t e = launch_frame_stream_fill(S, P.seed_state0, P.first_frame, P.frame_stride, P.n_frames, P.frame_stream, st);
    if (e != hipSuccess) return e;
  }
  log_render_launch(reinterpret_cast<const void*>(kernel), st);  // (RENE_TEST_KERNEL_LOG, kernels.h)
  hipLaunchKernelGGL(kernel, grid, block, lds, st, V, P);
  return hipGetLastError();
}

hipError_t launch_render(const LaunchConfig& cfg, const SceneView& S, const RenderParams& P, hipStream_t st) {
  const KernelChoice k = select_kernel(cfg, S, P.flags);
  return launch_kernel(k, (k.feat & FEAT_VOLPATH) ? vol_render_kernel(k) : (k.feat & FEAT_SMALL) ? item_render_kernel(k) : bvh_render_kernel(k), cfg, S, P, st);
}

hipError_t launch_trace(const LaunchConfig& cfg, const SceneView& S, int which, uint32_t n, const float* o,
                        const float* d, float tmin, float tmax, rene_hit* out, hipStream_t st) {
  size_t lds = (size_t)cfg.stack_depth * BLOCK * sizeof(uint32_t);
  dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
  if (cfg.features & FEAT_SMALL) hipLaunchKernelGGL(trace_kernel<true>, grid, block, 0, st, S, which, n, o, d, tmin, tmax, out);
  else hipLaunchKernelGGL(trace_kernel<false>, grid, block, lds, st, S, which, n, o, d, tmin, tmax, out);
  return hipGetLastError();
}

int render_block_size() { return BLOCK; }

}  // namespace rene
