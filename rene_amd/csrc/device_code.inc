// device_code.inc -- all device functions of the render path; included by kernels.hip (small-scene family,
// probes), kernels_bvh.hip (BVH megakernels), kernels_vol.hip (volpath) and kernels_wave.hip (wavefront):
// separate translation units so that the kernel families compile in parallel.
// kernels.hip -- the render hot path on gfx950 (CDNA4): ray generation, BVH traversal +
// intersection, hit shading / BSDF sampling, rene's one-sample light/BSDF mixture ("NEE") and
// radiance accumulation.
//
// Reference statement order: rene-shader/src/lib.rs:141-357 (main_ray_generation_path); hit
// shaders lib.rs:805-1066; BxDFs reflection/bxdf.rs; microfacet.rs; fresnel.rs; material.rs;
// texture.rs; light.rs; area_light.rs; surface_sample.rs; camera.rs; rand.rs; math.rs.
//
// Execution model (MI355X-first, not Vulkan's raygen/hit/miss shader split):
//   * one persistent launch renders N frames; a lane owns one pixel at a time and keeps its three
//     accumulation sums in registers for all N frames (one framebuffer read + write per pixel per
//     launch instead of rene's read-modify-write per add_image, lib.rs:165-172);
//   * path regeneration: a lane whose path ended starts the next frame of its pixel (or fetches a
//     new pixel from a wave-aggregated atomic work counter) while its neighbours keep bouncing, so
//     the 64-wide wavefront stays full although path lengths range from 1 to 50 bounces;
//   * sums are added in exactly the reference's order (frame by frame, bounce by bounce), so a
//     pixel's result does not depend on scheduling, on the number of launches or on GPU count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <unordered_map>

#include "device_math.h"
#include "device_scene.h"
#include "kernels.h"
#include "box_slabs.h"

namespace rene {

constexpr int BLOCK = 256;

// =================================================================================================
// traversal
// =================================================================================================
struct HitRec {
  float t, u, v;
  uint32_t slot;  // 0xffffffff = miss
};

struct LaneCounters {
  uint32_t closest = 0, shadow = 0, emitter = 0, paths = 0, hits = 0, adds = 0, nodes = 0, prims = 0;
};

RENE_DEV float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// Moeller-Trumbore, no culling, tmin <= t, closest wins (first found wins ties)
struct TriData {
  float4 a, b, c;
};
RENE_DEV TriData load_triangle(const PrimIsect* isect, uint32_t slot) {
  const float* q = isect[slot].q;
  return TriData{ldg4(q), ldg4(q + 4), ldg4(q + 8)};
}
RENE_DEV void intersect_triangle(const TriData& td, uint32_t slot, f3 o, f3 d, float tmin, HitRec& best, float& tmax) {
  const float4 a = td.a, b = td.b, c = td.c;
  f3 p0 = mk3(a.x, a.y, a.z), e1 = mk3(a.w, b.x, b.y), e2 = mk3(b.z, b.w, c.x);
  // no early-outs: the three loads above are issued together and nothing below depends on a branch, so a
  // leaf costs one memory round trip instead of two (the kernels are bound by dependent loads, not by VALU)
  f3 pv = cross(d, e2);
  float det = dot(e1, pv);
  float inv_det = fast_rcp(det);
  f3 tv = o - p0;
  float u = dot(tv, pv) * inv_det;
  f3 qv = cross(tv, e1);
  float v = dot(d, qv) * inv_det;
  float t = dot(e2, qv) * inv_det;
  bool inside = det != 0.0f && u >= 0.0f && u <= 1.0f && v >= 0.0f && u + v <= 1.0f;
  bool accept = inside && t >= tmin && (best.slot == 0xffffffffu ? t <= tmax : t < tmax);
  if (accept) {
    tmax = t;
    best.t = t;
    best.u = u;
    best.v = v;
    best.slot = slot;
  }
}
RENE_DEV void intersect_triangle(const PrimIsect* isect, uint32_t slot, f3 o, f3 d, float tmin, HitRec& best, float& tmax) {
  intersect_triangle(load_triangle(isect, slot), slot, o, d, tmin, best, tmax);
}
// a leaf of `count` triangles from slot `first`: the records of the first two (the builder's leaves hold at most
// two) are loaded together, so the leaf costs one memory round trip, not one per triangle
RENE_DEV void intersect_leaf(const PrimIsect* isect, uint32_t first, uint32_t count, f3 o, f3 d, float tmin,
                             HitRec& best, float& tmax, uint32_t& n_tests) {
  const TriData t0 = load_triangle(isect, first);
  const TriData t1 = load_triangle(isect, count > 1u ? first + 1u : first);
  intersect_triangle(t0, first, o, d, tmin, best, tmax);
  if (count > 1u) intersect_triangle(t1, first + 1u, o, d, tmin, best, tmax);
  for (uint32_t k = 2; k < count; ++k) intersect_triangle(isect, first + k, o, d, tmin, best, tmax);
  n_tests += count;
}

// sphere_intersection, rene-shader/src/lib.rs:805-839: unit sphere in object space
RENE_DEV void intersect_sphere(const PrimIsect* isect, const Sphere* spheres, uint32_t slot, f3 o, f3 d,
                               float tmin, HitRec& best, float& tmax) {
  uint32_t sidx = __float_as_uint(isect[slot].q[11]);
  const float* w2o = spheres[sidx].w2o;
  f3 oc = aff_point(w2o, o);
  f3 od = aff_vector(w2o, d);
  float a = length_squared(od);
  float half_b = dot(oc, od);
  float c = length_squared(oc) - 1.0f;
  float disc = half_b * half_b - a * c;
  if (disc < 0.0f) return;
  float sq = fast_sqrt(disc);
  float root0 = qdiv(-half_b - sq, a);
  float root1 = qdiv(-half_b + sq, a);
  float r;
  if (root0 >= tmin && root0 <= tmax) r = root0;
  else if (root1 >= tmin && root1 <= tmax) r = root1;
  else return;
  tmax = r;
  best.t = r;
  best.u = 0.0f;
  best.v = 0.0f;
  best.slot = slot;
}

typedef float float16v __attribute__((ext_vector_type(16)));  // a SmallItem: one s_load_dwordx16
typedef float v2f __attribute__((ext_vector_type(2)));         // operand pair of v_pk_{fma,mul,add}_f32
RENE_DEV v2f splat2(float a) { return v2f{a, a}; }
RENE_DEV v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }

// Reciprocal direction for the node tests.  The quantised form t = fma(byte, step * inv, (origin - o) * inv)
// needs a finite inv: with inv = inf it turns into inf - inf = NaN, the axis drops out of the test and a ray
// with one exactly-zero direction component (probability 2^-24 per cosine sample: a few per frame) walks
// every node in its shadow -- measured: one such ray made a 1.4 ms frame take 35 ms.  A zero (or denormal)
// component is therefore replaced by +-1e-20 here; the ray itself is untouched.
RENE_DEV float safe_rcp(float d) { return __builtin_amdgcn_rcpf(fabsf(d) < 1e-20f ? copysignf(1e-20f, d) : d); }
RENE_DEV f3 safe_inv(f3 d) { return mk3(safe_rcp(d.x), safe_rcp(d.y), safe_rcp(d.z)); }

// One BVH4 node: slab-test the four quantised child boxes and return them sorted by entry distance
// (t = +inf for a miss).  With A = (origin - o) * inv and B = step * inv per axis, a corner's ray parameter
// is fma(byte, B, A): the corner itself is never reconstructed.
RENE_DEV float ubyte_f(uint32_t w, int k) {  // v_cvt_f32_ubyte0..3
  return (float)((w >> (8 * k)) & 0xffu);
}
RENE_DEV void node4_test(const float* q, f3 o, f3 inv, float tmin, float tmax, float t[4], uint32_t w[4]) {
  float4 q0 = ldg4(q), q1 = ldg4(q + 4), q2 = ldg4(q + 8), q3 = ldg4(q + 12);
  const float bx = q3.z * inv.x, by = q3.w * inv.y, bz = q0.w * inv.z;
  const float ax = (q0.x - o.x) * inv.x, ay = (q0.y - o.y) * inv.y, az = (q0.z - o.z) * inv.z;
  // the ray's direction signs decide once per node which corner bytes are the entry and which the exit planes
  const uint32_t lx = __float_as_uint(q2.x), ly = __float_as_uint(q2.y), lz = __float_as_uint(q2.z);
  const uint32_t hx = __float_as_uint(q2.w), hy = __float_as_uint(q3.x), hz = __float_as_uint(q3.y);
  const bool px = inv.x >= 0.0f, py = inv.y >= 0.0f, pz = inv.z >= 0.0f;
  const uint32_t nx = px ? lx : hx, ny = py ? ly : hy, nz = pz ? lz : hz;
  const uint32_t fx = px ? hx : lx, fy = py ? hy : ly, fz = pz ? hz : lz;
  w[0] = __float_as_uint(q1.x);
  w[1] = __float_as_uint(q1.y);
  w[2] = __float_as_uint(q1.z);
  w[3] = __float_as_uint(q1.w);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    // (entry, exit) parameter of each axis as one v_pk_fma_f32
    const v2f tx = pk_fma(v2f{ubyte_f(nx, c), ubyte_f(fx, c)}, splat2(bx), splat2(ax));
    const v2f ty = pk_fma(v2f{ubyte_f(ny, c), ubyte_f(fy, c)}, splat2(by), splat2(ay));
    const v2f tz = pk_fma(v2f{ubyte_f(nz, c), ubyte_f(fz, c)}, splat2(bz), splat2(az));
    float lo = fmaxf(fmaxf(tx.x, ty.x), fmaxf(tz.x, tmin));
    float hi = fminf(fminf(tx.y, ty.y), fminf(tz.y, tmax));
    // slack: the parameters carry the rounding of A and B; a box must never reject a hit its primitive accepts.
    // An absent child (lo bytes 255, hi bytes 0) fails on every axis; should the slack ever bridge that for a
    // far, tiny node, its word is a one-primitive leaf at slot 0: one wasted, exact primitive test.
    // `slack >= 0 ? lo : inf` without a compare and a select (half rate each, profiles/r03_valu_rates.txt; dragon-class and teapot-class
    // + 0.9 %, bit-identical): the slack's sign bit smeared over the word and OR-ed into the entry distance -- a miss becomes 0xffffffff,
    // which sorts behind every distance (and behind +inf) as an unsigned key and is a NaN to node4_descend's `t < inf`.  lo >= tmin > 0
    // and an exact-zero slack is +0, so the set of accepted children is the one of the compare
    t[c] = __uint_as_float(__float_as_uint(lo) | (uint32_t)((int32_t)__float_as_uint(fmaf(hi, 1.00002f, -lo)) >> 31));
  }
  // sorting network, ascending by entry distance.  Entry distances are >= tmin > 0 (or +inf), so their bit patterns
  // order like the floats: one unsigned compare per exchange decides the distance pair (v_min_u32 / v_max_u32) and
  // the word pair (two v_cndmask on the same condition); equal distances keep their child order
  uint32_t k0 = __float_as_uint(t[0]), k1 = __float_as_uint(t[1]), k2 = __float_as_uint(t[2]), k3 = __float_as_uint(t[3]);
  uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
#define RENE_CE(ka, kb, wa, wb)              \
  {                                          \
    const bool le_ = ka <= kb;               \
    const uint32_t lo_ = ka < kb ? ka : kb, hi_ = ka < kb ? kb : ka; \
    const uint32_t wl_ = le_ ? wa : wb, wh_ = le_ ? wb : wa;         \
    ka = lo_; kb = hi_; wa = wl_; wb = wh_;  \
  }
  RENE_CE(k0, k1, w0, w1) RENE_CE(k2, k3, w2, w3) RENE_CE(k0, k2, w0, w2) RENE_CE(k1, k3, w1, w3) RENE_CE(k1, k2, w1, w2)
#undef RENE_CE
  t[0] = __uint_as_float(k0); w[0] = w0;
  t[1] = __uint_as_float(k1); w[1] = w1;
  t[2] = __uint_as_float(k2); w[2] = w2;
  t[3] = __uint_as_float(k3); w[3] = w3;
}
// after node4_test: continue with the nearest hit child, push the others farthest first; false = nothing hit
RENE_DEV bool node4_descend(const float t[4], const uint32_t w[4], uint32_t* stack, int& sp, uint32_t& cur) {
  if (!(t[0] < __builtin_inff())) return false;
  if (t[3] < __builtin_inff()) { stack[sp * BLOCK] = w[3]; sp++; }
  if (t[2] < __builtin_inff()) { stack[sp * BLOCK] = w[2]; sp++; }
  if (t[1] < __builtin_inff()) { stack[sp * BLOCK] = w[1]; sp++; }
  cur = w[0];
  return true;
}

// While-while BVH4 traversal with a per-lane stack in LDS ([depth][lane] so that a push/pop is
// conflict-free).  ANY: occlusion query, returns at the first accepted hit.
template <bool ANY, bool SPHERES, bool COUNT>
RENE_DEV HitRec traverse(const Accel& A, const Sphere* spheres, f3 o, f3 d, float tmin, float tmax,
                         uint32_t* stack, LaneCounters& lc) {
  HitRec best;
  best.t = 0.0f;
  best.u = 0.0f;
  best.v = 0.0f;
  best.slot = 0xffffffffu;
  const f3 inv = safe_inv(d);
  int sp = 0;
  uint32_t cur = 0;  // root is always an inner node
  for (;;) {
    // ---- inner nodes ----
    while (!(cur & LEAF_BIT)) {
      if (COUNT) lc.nodes++;
      float t4[4];
      uint32_t w4[4];
      node4_test(A.nodes[cur].q, o, inv, tmin, tmax, t4, w4);
      if (!node4_descend(t4, w4, stack, sp, cur)) {
        if (sp == 0) return best;
        sp--;
        cur = stack[sp * BLOCK];
      }
    }
    // ---- leaf ----
    {
      uint32_t first = cur & LEAF_FIRST_MASK;
      uint32_t count = ((cur >> LEAF_COUNT_SHIFT) & 15u) + 1u;
      if (SPHERES && (cur & SPHERE_BIT)) {
        if (COUNT) lc.prims++;
        intersect_sphere(A.isect, spheres, first, o, d, tmin, best, tmax);
      } else {
        uint32_t n_tests = 0;
        intersect_leaf(A.isect, first, count, o, d, tmin, best, tmax, n_tests);
        if (COUNT) lc.prims += n_tests;
      }
      if (ANY && best.slot != 0xffffffffu) return best;
      if (sp == 0) return best;
      sp--;
      cur = stack[sp * BLOCK];
    }
  }
}

// -------------------------------------------------------------------------------------------------
// Small scenes: wave-coherent loop over every item (device_scene.h, SmallItem).  The item index is
// wave-uniform, so the 64-byte record is fetched once per wave through the scalar cache (s_load)
// and its fields are SGPR operands of the per-lane arithmetic; there is no stack, no divergent
// control flow and no vector memory traffic.  A parallelogram item covers two triangles.
// -------------------------------------------------------------------------------------------------


// ---- the LDS-resident tables of a small scene (device_scene.h, "LDS image") ---------------------------------
typedef const __attribute__((address_space(3))) float* lds_ptr;
typedef float lds_v4 __attribute__((ext_vector_type(4)));
RENE_DEV float4 lds4(lds_ptr p) {  // ds_read_b128
  const lds_v4 v = *(const __attribute__((address_space(3))) lds_v4*)p;
  return make_float4(v.x, v.y, v.z, v.w);
}
struct SmallLds {
  lds_ptr items_main, items_emit, hit, emit, eobj, etri, spheres;
};
RENE_DEV SmallLds small_lds(const SceneView& S, const uint32_t* lds_base) {
  lds_ptr b = (lds_ptr)lds_base;
  return SmallLds{b, b + (S.small_off[SMALL_OFF_EMIT_ITEMS] >> 2), b + (S.small_off[SMALL_OFF_HIT] >> 2),
                  b + (S.small_off[SMALL_OFF_EMIT] >> 2), b + (S.small_off[SMALL_OFF_EOBJ] >> 2), b + (S.small_off[SMALL_OFF_ETRI] >> 2),
                  b + (S.small_off[SMALL_OFF_SPHERES] >> 2)};
}
// every workgroup copies the image once, when the (persistent) launch starts
RENE_DEV void small_lds_fill(const SceneView& S, uint32_t* lds_base) {
  const uint32_t n16 = S.small_bytes >> 4;
  const lds_v4* src = reinterpret_cast<const lds_v4*>(S.small_image);
  __attribute__((address_space(3))) lds_v4* dst = (__attribute__((address_space(3))) lds_v4*)lds_base;
  for (uint32_t i = threadIdx.x; i < n16; i += BLOCK) dst[i] = src[i];
}
// ---- the launch's frame seeds: two-level tables in LDS (device_scene.h, SEED_TAB_*), filled once per workgroup --------
// state of launch frame i = T1[i >> shift] * T2[j].mul + T2[j].add with j = i & (2^shift - 1): three LDS reads and a
// multiply-add per path start whatever the launch's length -- one launch renders a whole job (8192 frames of the teapot
// configuration: 1.3 KB of tables where a seed per frame would be 32 KB).
RENE_DEV void seed_tables_fill(const RenderParams& P, uint32_t* lds_base) {
  if (P.seed_tab == SEED_TAB_NONE) return;
  const uint32_t shift = P.seed_tab >> 24;
  __attribute__((address_space(3))) uint32_t* T2 = (__attribute__((address_space(3))) uint32_t*)lds_base + (P.seed_tab & 0xffffffu);
  if (shift == 0u) {  // direct: the seeds themselves
    for (uint32_t i = threadIdx.x; i < P.n_frames; i += BLOCK) T2[i] = frame_seed(P.seed_state0, P.first_frame + i * P.frame_stride);
    return;
  }
  const uint32_t B = 1u << shift, n1 = (P.n_frames + B - 1u) >> shift;
  __attribute__((address_space(3))) uint32_t* T1 = T2 + 2u * B;
  for (uint32_t j = threadIdx.x; j < B; j += BLOCK) {
    uint32_t m, a;
    lcg_pow(j * P.frame_stride, m, a);
    T2[2u * j] = m;
    T2[2u * j + 1u] = a;
  }
  for (uint32_t k = threadIdx.x; k < n1; k += BLOCK) T1[k] = frame_state(P.seed_state0, P.first_frame + (k << shift) * P.frame_stride);
}
RENE_DEV uint32_t launch_seed(const RenderParams& P, const uint32_t* lds_base, uint32_t i) {
  if (P.seed_tab == SEED_TAB_NONE) return frame_seed(P.seed_state0, P.first_frame + i * P.frame_stride);
  const uint32_t shift = P.seed_tab >> 24;
  const __attribute__((address_space(3))) uint32_t* T2 = (const __attribute__((address_space(3))) uint32_t*)lds_base + (P.seed_tab & 0xffffffu);
  if (shift == 0u) return T2[i];
  const uint32_t B = 1u << shift, j = i & (B - 1u);
  return pcg_output(T2[2u * B + (i >> shift)] * T2[2u * j] + T2[2u * j + 1u]);
}
// ---- a lane's prepared path start (render_kernel, RENE_START_SLOT): [dword][BLOCK] at word `at` of the workgroup's LDS, the lane's own column --------
// (dword-planar: a wave's 64 accesses to one plane are 64 consecutive words; a lane reads and writes only its own column, in program order)
RENE_DEV void start_slot_store(uint32_t* lds_base, uint32_t at, f3 rd, uint32_t state) {
  __attribute__((address_space(3))) uint32_t* q = (__attribute__((address_space(3))) uint32_t*)lds_base + at + threadIdx.x;
  q[0] = __float_as_uint(rd.x);
  q[BLOCK] = __float_as_uint(rd.y);
  q[2 * BLOCK] = __float_as_uint(rd.z);
  q[3 * BLOCK] = state;
}
RENE_DEV void start_slot_load(const uint32_t* lds_base, uint32_t at, f3& rd, uint32_t& state) {
  const __attribute__((address_space(3))) uint32_t* q = (const __attribute__((address_space(3))) uint32_t*)lds_base + at + threadIdx.x;
  rd = mk3(__uint_as_float(q[0]), __uint_as_float(q[BLOCK]), __uint_as_float(q[2 * BLOCK]));
  state = q[3 * BLOCK];
}

// A triangle / parallelogram item against the ray: the plane first, then the point's coordinates in the reciprocal basis of the two edges (SmallItem)
struct PlaneHit {
  float t, s, r;
  bool inside;  // (s, r) inside the item: s, r >= 0 and s + r <= 1 (triangle, kind 1) or s, r <= 1 (parallelogram, kind 0)
};
RENE_DEV PlaneHit plane_item(const float16v q, f3 o, f3 d) {
  const float kind = q[12];
  const float n_o = o.x * q[0] + (o.y * q[1] + o.z * q[2]);
  const float n_d = d.x * q[0] + (d.y * q[1] + d.z * q[2]);
  float t = (q[3] - n_o) * __builtin_amdgcn_rcpf(n_d);  // n.d == 0 -> inf / nan -> rejected by the callers' compares
  f3 P = mk3(fmaf(t, d.x, o.x), fmaf(t, d.y, o.y), fmaf(t, d.z, o.z));
  // (scalar fma chains: v_pk_fma_f32 pairs measured 2 % slower once the compiler's own SLP packing was switched off --
  // packed operands need adjacent registers, i.e. moves, and a packed instruction occupies the SIMD as long as its two halves)
  const float sr_x = fmaf(P.x, q[4], fmaf(P.y, q[6], P.z * q[8])) + q[10];
  const float sr_y = fmaf(P.x, q[5], fmaf(P.y, q[7], P.z * q[9])) + q[11];
  const float lim_x = fmaf(-kind, sr_y, 1.0f - sr_x), lim_y = fmaf(-kind, sr_x, 1.0f - sr_y);
  return PlaneHit{t, sr_x, sr_y, fminf(fminf(sr_x, sr_y), fminf(lim_x, lim_y)) >= 0.0f};
}
// ITEMS_LDS: the loop's items still come through the scalar cache (wave-uniform index), but the per-lane look-up of
// the winning item after the loop reads the copy in LDS (`lds_items`) instead of gathering through L1 / L2
// CAPTURE (the closest-hit query of a bounce in the kernels that fuse the emitter query into it, render_kernel below): at the main item marked
// SMALL_ITEM_EMIT_TWIN -- bit for bit the emitter structure's only item -- the loop also records what the emitter query of the same ray, the
// one-item loop over that item, would have found: inside, t >= tmin, t within tmax by the first-hit compare, whatever else is closer.
struct EmitCapture {
  float s = -1.0f, r = 0.0f;  // the emitter query's hit on its item; s == -1 (no hit passes the inside test with it): a miss
  uint32_t seen = 0u;         // wave-uniform: the list has a marked item, i.e. this scene's emitter query is fused
};
// BOX (box_slabs.h): which form of the box item's test the loop uses
template <bool ANY, bool SPHERES, bool COUNT, bool ITEMS_LDS = false, bool CAPTURE = false, int BOX = BOX_FORM_PLAIN>
RENE_DEV HitRec traverse_small(const Accel& A, const Sphere* spheres, f3 o, f3 d, float tmin, float tmax,
                               LaneCounters& lc, lds_ptr lds_items = nullptr, EmitCapture* cap = nullptr) {
  static_assert(BOX == BOX_FORM_PLAIN || !SPHERES, "box_slabs.h's forms are for the kernels without sphere items");
  static_assert(BOX_KIND_BITS == 0x40400000u && SMALL_KIND_BOX == 3.0f, "BOX_KIND_BITS is the bit pattern of SMALL_KIND_BOX");
  // `t <= tmax` for the first hit and `t < best` afterwards, as one strict comparison
  const float first_t = __uint_as_float(__float_as_uint(tmax) + 1u);
  float best_t = first_t, best_s = 0.0f, best_r = 0.0f;
  uint32_t best_item = 0xffffffffu;
  const uint32_t n = A.n_items;
  typedef const __attribute__((address_space(4))) float16v* item_ptr;
  item_ptr base = (item_ptr)(const void*)A.items;
  // one item against the ray (`continue` in the loop this was = `return`)
  auto test_item = [&](const float16v q, const uint32_t k) {
    const float kind = q[12];  // also the coefficient c below: 1 triangle, 0 parallelogram (2 sphere)
    if (COUNT) lc.prims++;
    if (SPHERES && kind == SMALL_KIND_BALL) {
      // sphere_intersection (lib.rs:805-839) for a translated, uniformly scaled unit sphere, multiplied through by
      // radius^2: with oc = o - C the quadratic is |d|^2 t^2 + 2 (oc.d) t + |oc|^2 - r^2, same roots, no matrix
      f3 oc = mk3(o.x - q[0], o.y - q[1], o.z - q[2]);
      float a = length_squared(d);
      float half_b = dot(oc, d);
      float c = length_squared(oc) - q[3];
      float disc = half_b * half_b - a * c;
      if (disc >= 0.0f) {
        float sq = fast_sqrt(disc);
        float inv_a = fast_rcp(a);
        float root0 = (-half_b - sq) * inv_a;
        float root1 = (-half_b + sq) * inv_a;
        float r = -1.0f;
        if (root0 >= tmin && root0 < best_t) r = root0;
        else if (root1 >= tmin && root1 < best_t) r = root1;
        if (r >= tmin && r < best_t) {
          best_t = r;
          best_s = 0.0f;
          best_r = 0.0f;
          best_item = k;
        }
      }
      return;
    }
    if (SPHERES && kind == SMALL_KIND_SPHERE) {  // sphere_intersection, lib.rs:805-839
      uint32_t slot = __float_as_uint(q[13]);
      uint32_t sidx = __float_as_uint(A.isect[slot].q[11]);
      const float* w2o = spheres[sidx].w2o;
      f3 oc = aff_point(w2o, o);
      f3 od = aff_vector(w2o, d);
      float a = length_squared(od);
      float half_b = dot(oc, od);
      float c = length_squared(oc) - 1.0f;
      float disc = half_b * half_b - a * c;
      if (disc >= 0.0f) {
        float sq = fast_sqrt(disc);
        float root0 = qdiv(-half_b - sq, a);
        float root1 = qdiv(-half_b + sq, a);
        float r = -1.0f;
        if (root0 >= tmin && root0 < best_t) r = root0;
        else if (root1 >= tmin && root1 < best_t) r = root1;
        if (r >= tmin && r < best_t) {
          best_t = r;
          best_s = 0.0f;
          best_r = 0.0f;
          best_item = k;
        }
      }
      return;
    }
    if (kind == SMALL_KIND_BOX) {  // wave-uniform: a parallelepiped as three slab pairs in its own coordinates
      // coordinate along axis x of the point o + t d:  c0 + t c1  with c0 = o . x' - O . x', c1 = d . x'; the faces are at
      // 0 and 1.  Only the entry and exit parameters are carried through the three axes; which face was hit is read off
      // the hit point after the loop (a third of the loop's instructions when every accepting box did it on the spot:
      // Cornell's room accepts for every ray, and a block in front of it then did it all again).
      float t_in = -__builtin_inff(), t_out = __builtin_inff(), t0 = 0.0f, t1 = 0.0f;
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        const float c0 = o.x * q[4 * ax] + (o.y * q[4 * ax + 1] + (o.z * q[4 * ax + 2] + q[4 * ax + 3]));
        const float c1 = d.x * q[4 * ax] + (d.y * q[4 * ax + 1] + d.z * q[4 * ax + 2]);
        const float inv = __builtin_amdgcn_rcpf(c1);
        t0 = -c0 * inv;
        t1 = t0 + inv;
        t_in = fmaxf(t_in, fminf(t0, t1));
        t_out = fminf(t_out, fmaxf(t0, t1));
      }
      // a line meets a convex box in its entry and its exit face; the closest with t >= tmin is the hit.  A box may have
      // one open face, on its third axis (q[14]: 1 = the face at coordinate 0, 2 = at 1): the ray passes through it.
      const uint32_t open_face = __float_as_uint(q[14]);  // wave-uniform
      bool use_in = t_in >= tmin, dead = false;
      if (open_face != 0u) {
        const float t_open = open_face == 1u ? t0 : t1;
        use_in = use_in && t_in != t_open;
        dead = !use_in && t_out == t_open;
      }
      const float t = use_in ? t_in : t_out;
      if (t_in <= t_out && !dead && t >= tmin && t < best_t) {  // which face, and where on it: after the loop, once, for the winner
        best_t = t;
        best_item = k;
      }
      return;
    }
    const PlaneHit p = plane_item(q, o, d);
    const float t = p.t, sr_x = p.s, sr_y = p.r;
    bool accept = p.inside && t >= tmin && t < best_t;
    if constexpr (CAPTURE) {
      if (__float_as_uint(q[15]) & SMALL_ITEM_EMIT_TWIN) {  // wave-uniform
        const bool alone = p.inside && t >= tmin && t < first_t;
        cap->s = alone ? sr_x : -1.0f;
        cap->r = sr_y;
        cap->seen = 1u;
      }
    }
    if (accept) {
      best_t = t;
      best_s = sr_x;
      best_r = sr_y;
      best_item = k;
    }
  };
  // (Written out per item by hand -- item k + 1 on its way from the scalar cache while item k is tested, two SGPR tuples
  // alternating behind asm loads and waits -- the loop spills twenty SGPRs and is 4 % slower on Cornell: profiles/r03_bvh_experiments.txt.)
  // The same for the kernels that ask for one of box_slabs.h's forms (Matte: boxes, triangles, parallelograms).  Either kind only proposes a
  // hit; ONE set of selects behind the join takes it, so that the loop's running values are touched in one place and stay in their registers (the
  // kinds updating them each on its own path cost a register copy per value and item).  A box that wins overwrites best_s / best_r with whatever it has at hand:
  // they are recomputed from the hit point behind the loop for a box.  The kind is dispatched by an integer compare of the SGPR's bits.
  auto test_item_box = [&](const float16v q, const uint32_t k) {
    if (COUNT) lc.prims++;
    float t, s, r;
    bool hit;
    [[maybe_unused]] bool twin = false;
    [[maybe_unused]] float twin_s = 0.0f;
    if (__float_as_uint(q[12]) == BOX_KIND_BITS) {  // wave-uniform
      const BoxSlabs b = box_slabs_valu(q, o.x, o.y, o.z, d.x, d.y, d.z);
      hit = box_accept(b, __float_as_uint(q[14]), tmin, best_t, t);
      s = b.t_in, r = b.t_out;  // anything that is in a register already
    } else {
      const PlaneHit p = plane_item(q, o, d);
      t = p.t, s = p.s, r = p.r;
      hit = p.inside && t >= tmin && t < best_t;
      if constexpr (CAPTURE) {
        twin = (__float_as_uint(q[15]) & SMALL_ITEM_EMIT_TWIN) != 0u;  // wave-uniform
        twin_s = p.inside && t >= tmin && t < first_t ? s : -1.0f;
      }
    }
    best_t = hit ? t : best_t;
    best_s = hit ? s : best_s;
    best_r = hit ? r : best_r;
    best_item = hit ? k : best_item;
    if constexpr (CAPTURE) {
      if (twin) {
        asm volatile("");  // keeps this a scalar branch: as selects it is two instructions for every item, and one item has the mark
        cap->s = twin_s;
        cap->r = r;
        cap->seen = 1u;
      }
    }
  };
  for (uint32_t k = 0; k < n; ++k) {
    if constexpr (BOX == BOX_FORM_PLAIN) test_item(base[k], k);
    else test_item_box(base[k], k);
  }
  HitRec h;
  h.t = best_t;
  h.u = 0.0f;
  h.v = 0.0f;
  h.slot = 0xffffffffu;
  if (ANY && best_item != 0xffffffffu) {  // an occlusion query: the callers only ask whether something was hit
    h.slot = 0u;
    return h;
  }
  if (best_item != 0xffffffffu) {
    // map (item, s, r) back to (triangle slot, barycentric u, v) of the BVH path's conventions
    float4 m = ITEMS_LDS ? lds4(lds_items + 16u * best_item + 12u) : ldg4(A.items[best_item].q + 12);  // kind, slot1, slot2, perm1 | perm2 << 8
    if (m.x == SMALL_KIND_BOX) {  // the face's own parallelogram: slots, perms and how its (s, r) run (device_scene.h)
      // box coordinates of the hit point: the one farthest from 1/2 names the face (it is 0 or 1 up to rounding, the other
      // two are inside [0, 1]) and the other two, in ascending axis order, are the in-face coordinates
      float4 b0, b1, b2;
      if (ITEMS_LDS) {
        lds_ptr bq = lds_items + 16u * best_item;
        b0 = lds4(bq); b1 = lds4(bq + 4); b2 = lds4(bq + 8);
      } else {
        const float* bq = A.items[best_item].q;
        b0 = ldg4(bq); b1 = ldg4(bq + 4); b2 = ldg4(bq + 8);
      }
      const f3 P = mk3(fmaf(best_t, d.x, o.x), fmaf(best_t, d.y, o.y), fmaf(best_t, d.z, o.z));
      const float pa = P.x * b0.x + (P.y * b0.y + (P.z * b0.z + b0.w)), pb = P.x * b1.x + (P.y * b1.y + (P.z * b1.z + b1.w)),
                  pc = P.x * b2.x + (P.y * b2.y + (P.z * b2.z + b2.w));
      const float ea = fabsf(pa - 0.5f), eb = fabsf(pb - 0.5f), ec = fabsf(pc - 0.5f);
      const uint32_t axis = ea >= eb ? (ea >= ec ? 0u : 2u) : (eb >= ec ? 1u : 2u);
      const float pf = axis == 0u ? pa : (axis == 1u ? pb : pc);
      best_s = axis == 0u ? pb : pa;
      best_r = axis == 2u ? pb : pc;
      const uint32_t face = 2u * axis + (pf > 0.5f ? 1u : 0u);
      uint32_t w0, w1;
      if (ITEMS_LDS) {
        lds_ptr aux = lds_items + 16u * __float_as_uint(m.y) + 2u * face;
        w0 = __float_as_uint(aux[0]);
        w1 = __float_as_uint(aux[1]);
      } else {
        const float* aux = A.items[__float_as_uint(m.y)].q + 2u * face;
        w0 = __float_as_uint(aux[0]);
        w1 = __float_as_uint(aux[1]);
      }
      const float c0 = best_s, c1 = best_r;
      float s = (w1 & 1u) ? c1 : c0, r = ((w1 >> 3) & 1u) ? c1 : c0;
      best_s = (w1 & 4u) ? 1.0f - s : s;
      best_r = (w1 & 32u) ? 1.0f - r : r;
      m.x = SMALL_KIND_QUAD;
      m.y = __uint_as_float(w0 & 0xffu);
      m.z = __uint_as_float((w0 >> 8) & 0xffu);
      m.w = __uint_as_float(w0 >> 16);
    }
    bool second = m.x == SMALL_KIND_QUAD && best_s + best_r > 1.0f;
    uint32_t perm = __float_as_uint(m.w) >> (second ? 8u : 0u);
    float w0 = second ? best_s + best_r - 1.0f : 1.0f - best_s - best_r;
    float w1 = second ? 1.0f - best_r : best_s;
    float w2 = second ? 1.0f - best_s : best_r;
    uint32_t iu = perm & 3u, iv = (perm >> 2) & 3u;
    h.u = iu == 0u ? w0 : (iu == 1u ? w1 : w2);
    h.v = iv == 0u ? w0 : (iv == 1u ? w1 : w2);
    h.slot = __float_as_uint(second ? m.z : m.y);
  } else {
    h.t = tmax;
  }
  return h;
}

template <bool SMALL, bool ANY, bool SPHERES, bool COUNT, bool ITEMS_LDS = false>
RENE_DEV HitRec trace_accel(const Accel& A, const Sphere* spheres, f3 o, f3 d, float tmin, float tmax,
                            uint32_t* stack, LaneCounters& lc, lds_ptr lds_items = nullptr) {
  if (SMALL) return traverse_small<ANY, SPHERES, COUNT, ITEMS_LDS>(A, spheres, o, d, tmin, tmax, lc, lds_items);
  return traverse<ANY, SPHERES, COUNT>(A, spheres, o, d, tmin, tmax, stack, lc);
}

// =================================================================================================
// textures / materials / BSDF
// =================================================================================================
struct uv2 {
  float x, y;
};

// asm.rs:26-46 (OpConvertFToU), saturating where SPIR-V is undefined
RENE_DEV uint32_t f32_to_u32(float v) {
  if (!(v > 0.0f)) return 0u;
  if (v >= 4294967296.0f) return 0xffffffffu;
  return (uint32_t)v;
}
RENE_DEV float fract(float v) { return v - floorf(v); }  // GLSL Fract, asm.rs:54-69

// bilinear, REPEAT addressing, texel centres at +0.5 (VK_FILTER_LINEAR, rene/src/main.rs:2390-2397)
RENE_DEV f3 image_sample_at(const float* base, uint32_t width, uint32_t height, float u, float v);
RENE_DEV f3 image_sample(const SceneView& S, uint32_t img, float u, float v) {
  ImageRef im = S.images[img];
  return image_sample_at(S.image_pool + im.offset, im.width, im.height, u, v);
}
RENE_DEV f3 image_sample_at(const float* base, uint32_t width, uint32_t height, float u, float v) {
  struct { uint32_t width, height; } im{width, height};
  float x = u * (float)im.width - 0.5f, y = v * (float)im.height - 0.5f;
  float fx = floorf(x), fy = floorf(y);
  float ax = x - fx, ay = y - fy;
  int w = (int)im.width, h = (int)im.height;
  // REPEAT: the texel index modulo the image's size.  A signed `%` by a runtime divisor is ~30 mostly half-rate instructions, and every
  // look-up has two; coordinates are nearly always within one period of the image (an environment map's are in [0, 1]), where the
  // remainder is one conditional add or subtract -- the general form runs only for the lanes that need it (same result either way)
  auto wrap = [](int i, int n) {
    if ((uint32_t)(i + n) < 3u * (uint32_t)n) return i < 0 ? i + n : (i >= n ? i - n : i);
    int r = i % n;
    return r < 0 ? r + n : r;
  };
  int x0 = wrap((int)fx, w), y0 = wrap((int)fy, h);
  int x1 = x0 + 1 == w ? 0 : x0 + 1, y1 = y0 + 1 == h ? 0 : y0 + 1;
  float4 p00 = ldg4(base + 4 * ((size_t)y0 * w + x0)), p10 = ldg4(base + 4 * ((size_t)y0 * w + x1));
  float4 p01 = ldg4(base + 4 * ((size_t)y1 * w + x0)), p11 = ldg4(base + 4 * ((size_t)y1 * w + x1));
  f3 top = mk3(p00.x, p00.y, p00.z) * (1.0f - ax) + mk3(p10.x, p10.y, p10.z) * ax;
  f3 bot = mk3(p01.x, p01.y, p01.z) * (1.0f - ax) + mk3(p11.x, p11.y, p11.z) * ax;
  return top * (1.0f - ay) + bot * ay;
}

// texture.rs:175-190
template <uint32_t FEAT>
RENE_DEV f3 tex_color_non_recursive(const SceneView& S, uint32_t index, uv2 uv) {
  const Texture& t = S.textures[index];
  if (!(FEAT & FEAT_TEXTURES)) return mk3(t.v0[0], t.v0[1], t.v0[2]);
  uint32_t type = t.type;
  if (type == RENE_TEXTURE_SOLID) return mk3(t.v0[0], t.v0[1], t.v0[2]);
  if (type == RENE_TEXTURE_IMAGEMAP) return image_sample(S, t.u0[0], uv.x, 1.0f - uv.y);  // texture.rs:121-127
  return splat(1.0f);
}
// texture.rs:192-211
template <uint32_t FEAT>
RENE_DEV f3 tex_color(const SceneView& S, uint32_t index, uv2 uv) {
  const Texture& t = S.textures[index];
  if (!(FEAT & FEAT_TEXTURES)) return mk3(t.v0[0], t.v0[1], t.v0[2]);
  uint32_t type = t.type;
  if (type == RENE_TEXTURE_SOLID) return mk3(t.v0[0], t.v0[1], t.v0[2]);
  if (type == RENE_TEXTURE_IMAGEMAP) return image_sample(S, t.u0[0], uv.x, 1.0f - uv.y);
  if (type == RENE_TEXTURE_CHECKERBOARD) {  // texture.rs:97-118
    float x = uv.x * t.v0[0], y = uv.y * t.v0[1];
    uint32_t idx = ((f32_to_u32(x) % 2u == 0u) == (f32_to_u32(y) % 2u == 0u)) ? t.u0[0] : t.u0[1];
    return tex_color_non_recursive<FEAT>(S, idx, uv2{fract(x), fract(y)});
  }
  return tex_color_non_recursive<FEAT>(S, t.u0[0], uv) * tex_color_non_recursive<FEAT>(S, t.u0[1], uv);
}

// main_miss's texture lookup (lib.rs:120-139), with the background texture resolved at upload where it is a Solid texture or an
// ImageMap (Uniforms::bg_*): the same colour without the texture record -> image record chain
template <uint32_t FEAT>
RENE_DEV f3 background_tex(const SceneView& S, uv2 uv) {
  const Uniforms* U = S.uni;
  const uint32_t kind = U->bg_kind;
  if (kind == 1u) return mk3(U->bg_solid[0], U->bg_solid[1], U->bg_solid[2]);
  if (kind == 2u) return image_sample_at(S.image_pool + U->bg_image_offset, U->bg_image_width, U->bg_image_height, uv.x, 1.0f - uv.y);
  return tex_color<FEAT | FEAT_TEXTURES>(S, S.bg_texture, uv);
}

// ---- local shading frame: Onb, onb_from_w and onb_from_w_select live in device_math.h (selftest/onb_probe.hip runs them on their own) ----------
// ---- what a bounce of the Matte small-scene kernels leaves out (DESIGN.md section 4a, profiles/bounce_trims_ab.txt) ---------------------------------
// Each bit rearranges the same floating-point operations on the same operands: every layer and every counter stays bit for bit what it was
// (tests/test_gpu_bounce_trims.py).  The mask a kernel gets is bounce_trims(FEAT) below the frame stream's: 0 everywhere but in FEAT 64 / 72.
#ifndef RENE_BOUNCE_TRIMS
#define RENE_BOUNCE_TRIMS 0xdu  // all but TRIM_ONB_SELECT, which costs four VGPRs and with them a wave; -DRENE_BOUNCE_TRIMS=0: these kernels as they were (A/B builds: make variant)
#endif
enum : uint32_t {
  TRIM_SHARED_RD = 1u,     // normalize(rd) once per pass, for the deferred emitter pdf and for wo
  TRIM_ONB_SELECT = 2u,    // onb_from_w_select
  TRIM_STATIC_MATTE = 4u,  // compute_bsdf / material_albedo without the table walk; no division by a lobe count that is 1
  TRIM_ALBEDO_PI = 8u,     // with TRIM_STATIC_MATTE: the lobe holds kd * (1 / pi), computed once ahead of the light / BSDF coin
  TRIM_UNIT_LEN = 16u,     // set by the caller where the BSDF is known to hold its one lobe (behind bsdf_contains): b.len == 1
};
constexpr bool trim_albedo_pi(uint32_t trim) { return (trim & (TRIM_STATIC_MATTE | TRIM_ALBEDO_PI)) == (TRIM_STATIC_MATTE | TRIM_ALBEDO_PI); }
RENE_DEV f3 to_world(const Onb& o, f3 a) { return a.x * o.u + a.y * o.v + a.z * o.w; }
RENE_DEV f3 to_local(const Onb& o, f3 a) { return mk3(dot(a, o.u), dot(a, o.v), dot(a, o.w)); }

RENE_DEV float abs_cos_theta(f3 w) { return fabsf(w.z); }
RENE_DEV float cos2_theta(f3 w) { return w.z * w.z; }
RENE_DEV float sin2_theta(f3 w) { return fmaxf(1.0f - w.z * w.z, 0.0f); }
RENE_DEV float sin_theta(f3 w) { return fast_sqrt(sin2_theta(w)); }
RENE_DEV float tan_theta(f3 w) { return qdiv(sin_theta(w), w.z); }
RENE_DEV float tan2_theta(f3 w) { return qdiv(sin2_theta(w), cos2_theta(w)); }
RENE_DEV float cos_phi(f3 w) {
  float s = sin_theta(w);
  return s == 0.0f ? 1.0f : clampf(qdiv(w.x, s), -1.0f, 1.0f);
}
RENE_DEV float sin_phi(f3 w) {
  float s = sin_theta(w);
  return s == 0.0f ? 0.0f : clampf(qdiv(w.y, s), -1.0f, 1.0f);
}
RENE_DEV bool same_hemisphere(f3 a, f3 b) { return a.z * b.z > 0.0f; }

// math.rs:45-56
RENE_DEV f3 random_cosine_direction(Pcg& rng) {
  float r1 = pcg_f32(rng);
  float r2 = pcg_f32(rng);
  float z = fast_sqrt(1.0f - r2);
  float r2_sqrt = fast_sqrt(r2);
  return mk3(cos_2pi(r1) * r2_sqrt, sin_2pi(r1) * r2_sqrt, z);  // phi = 2 pi r1
}
// math.rs:8-20
RENE_DEV f3 random_in_unit_sphere(Pcg& rng) {
  for (;;) {
    float a = pcg_range(rng, -1.0f, 1.0f);
    float b = pcg_range(rng, -1.0f, 1.0f);
    float c = pcg_range(rng, -1.0f, 1.0f);
    f3 v = mk3(a, b, c);
    if (length_squared(v) < 1.0f) return v;
  }
}

// ---- Fresnel: bxdf.rs:138-165, fresnel.rs:78-102 ----------------------------------------------------
RENE_DEV float fr_dielectric(float cos_theta_i, float eta_i, float eta_t) {
  cos_theta_i = clampf(cos_theta_i, -1.0f, 1.0f);
  if (!(cos_theta_i > 0.0f)) {
    float t = eta_i;
    eta_i = eta_t;
    eta_t = t;
  }
  cos_theta_i = fabsf(cos_theta_i);
  float sin_theta_i = fast_sqrt(1.0f - cos_theta_i * cos_theta_i);
  float sin_theta_t = qdiv(eta_i, eta_t) * sin_theta_i;
  if (sin_theta_t >= 1.0f) return 1.0f;
  float cos_theta_t = fast_sqrt(1.0f - sin_theta_t * sin_theta_t);
  float r_parl = qdiv((eta_t * cos_theta_i) - (eta_i * cos_theta_t), (eta_t * cos_theta_i) + (eta_i * cos_theta_t));
  float r_perp = qdiv((eta_i * cos_theta_i) - (eta_t * cos_theta_t), (eta_i * cos_theta_i) + (eta_t * cos_theta_t));
  return 0.5f * (r_parl * r_parl + r_perp * r_perp);
}
RENE_DEV f3 fr_conductor(float cos_theta_i, f3 eta_i, f3 eta_t, f3 k) {
  cos_theta_i = clampf(cos_theta_i, -1.0f, 1.0f);
  f3 eta = eta_t / eta_i;
  f3 eta_k = k / eta_i;
  float c2 = cos_theta_i * cos_theta_i;
  float s2 = 1.0f - c2;
  f3 eta2 = eta * eta;
  f3 eta_k2 = eta_k * eta_k;
  f3 t0 = eta2 - eta_k2 - splat(s2);
  f3 a2plusb2 = sqrt3(t0 * t0 + 4.0f * eta2 * eta_k2);
  f3 t1 = a2plusb2 + splat(c2);
  f3 a = sqrt3(0.5f * (a2plusb2 + t0));
  f3 t2 = 2.0f * cos_theta_i * a;
  f3 rs = (t1 - t2) / (t1 + t2);
  f3 t3 = c2 * a2plusb2 + splat(s2 * s2);
  f3 t4 = t2 * s2;
  f3 rp = rs * (t3 - t4) / (t3 + t4);
  return 0.5f * (rp + rs);
}

enum : uint32_t { FR_CONDUCTOR = 0, FR_NOOP = 1, FR_DIELECTRIC = 2 };
enum : uint32_t { BX_LAMBERT = 0, BX_FRESNEL_SPECULAR, BX_FRESNEL_BLEND, BX_MICROFACET, BX_SPEC_REFL, BX_SPEC_TRANS };
// The lobe kinds a kernel instantiation has to know, as a mask of 1 << BX_*: 0 for the Matte-only kernels, else
// everything the scene's FEAT_NO_* bits do not rule out.  Passed as the GENERAL template argument of the lobe / Bsdf
// functions below ("general" = non-zero); a kind that is masked out is compiled out.
constexpr uint32_t lobe_kinds(uint32_t feat) {
  return !(feat & FEAT_GENERAL_BSDF) ? 0u
       : (1u << BX_LAMBERT) | ((feat & FEAT_NO_SPECULAR) ? 0u : (1u << BX_FRESNEL_SPECULAR) | (1u << BX_SPEC_REFL) | (1u << BX_SPEC_TRANS)) |
         ((feat & FEAT_NO_BLEND) ? 0u : (1u << BX_FRESNEL_BLEND)) | ((feat & FEAT_NO_MICROFACET) ? 0u : (1u << BX_MICROFACET));
}
#define RENE_KIND_ON(t) (((GENERAL) >> (t)) & 1u)
enum : uint32_t { K_REFLECTION = 1, K_TRANSMISSION = 2, K_DIFFUSE = 4 };

// one BxDF lobe (EnumBxdfData, reflection.rs:94-100); only the fields its type reads are set
struct Lobe {
  uint32_t type;
  f3 a;            // albedo / rd / r / t ; FresnelSpecular: ir in a.x
  f3 b;            // rs ; SpecularTransmission: eta_a, eta_b
  float ax, ay;    // Trowbridge-Reitz alpha
  uint32_t fr;     // fresnel type
  f3 eta, k;       // conductor: eta_t, k (eta_i = 1); dielectric: eta.x = eta_i, eta.y = eta_t
};

RENE_DEV f3 fresnel_eval(const Lobe& l, float cos_i) {  // fresnel.rs:160-171
  if (l.fr == FR_NOOP) return splat(1.0f);
  if (l.fr == FR_CONDUCTOR) return fr_conductor(fabsf(cos_i), splat(1.0f), l.eta, l.k);
  return splat(fr_dielectric(cos_i, l.eta.x, l.eta.y));
}

// ---- TrowbridgeReitz, microfacet.rs:46-195 -------------------------------------------------------------
RENE_DEV float roughness_to_alpha(float roughness) {
  roughness = fmaxf(roughness, 1e-3f);
  float x = logf(roughness);
  return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}
RENE_DEV float tr_d(float ax, float ay, f3 wh) {
  float t2 = tan2_theta(wh);
  if (isinf(t2)) return 0.0f;
  float c2 = cos2_theta(wh);
  float cp = cos_phi(wh), spv = sin_phi(wh);
  float e = (qdiv(cp * cp, ax * ax) + qdiv(spv * spv, ay * ay)) * t2;
  return fast_rcp(kPi * ax * ay * (c2 * c2) * (1.0f + e) * (1.0f + e));
}
RENE_DEV float tr_lambda(float ax, float ay, f3 w) {  // Q9: Beckmann's fit
  float abs_tan = fabsf(tan_theta(w));
  if (isinf(abs_tan)) return 0.0f;
  float cp = cos_phi(w), spv = sin_phi(w);
  float alpha = fast_sqrt(cp * cp * ax * ax + spv * spv * ay * ay);
  float a = fast_rcp(alpha * abs_tan);
  if (a >= 1.6f) return 0.0f;
  return qdiv(1.0f - 1.259f * a + 0.396f * a * a, 3.535f * a + 2.181f * a * a);
}
RENE_DEV float tr_g(float ax, float ay, f3 wo, f3 wi) { return fast_rcp(1.0f + tr_lambda(ax, ay, wo) + tr_lambda(ax, ay, wi)); }
RENE_DEV float tr_pdf(float ax, float ay, f3 wo, f3 wh) {
  return qdiv(tr_d(ax, ay, wh) * fast_rcp(1.0f + tr_lambda(ax, ay, wo)) * fabsf(dot(wo, wh)), abs_cos_theta(wo));
}
RENE_DEV void tr_sample11(float cos_theta, Pcg& rng, float& sx, float& sy) {  // microfacet.rs:77-122
  float u1 = pcg_f32(rng);
  float u2 = pcg_f32(rng);
  if (cos_theta > 0.9999f) {
    float r = fast_sqrt(qdiv(u1, 1.0f - u1));
    sx = r * cos_2pi(u2);
    sy = r * sin_2pi(u2);
    return;
  }
  float sin_t = fast_sqrt(fmaxf(1.0f - cos_theta * cos_theta, 0.0f));
  float tan_t = qdiv(sin_t, cos_theta);
  float a0 = fast_rcp(tan_t);
  float g1 = qdiv(2.0f, 1.0f + (1.0f + fast_rcp(fast_sqrt(a0 * a0))));  // Q11
  float a = qdiv(2.0f * u1, g1) - 1.0f;
  float tmp = fminf(fast_rcp(a * a - 1.0f), 1e10f);
  float b = tan_t;
  float d = fast_sqrt(fmaxf(b * b * tmp * tmp - (a * a - b * b) * tmp, 0.0f));
  float s1 = b * tmp - d, s2 = b * tmp + d;
  sx = (a < 0.0f || s2 > a0) ? s1 : s2;
  float s;
  if (u2 > 0.5f) {
    s = 1.0f;
    u2 = 2.0f * (u2 - 0.5f);
  } else {
    s = -1.0f;
    u2 = 2.0f * (0.5f - u2);
  }
  float z = (u2 * (u2 * (u2 * 0.27385f - 0.73369f) + 0.46341f)) /
            (u2 * (u2 * (u2 * 0.093073f + 0.309420f) - 1.000000f) + 0.597999f);
  sy = s * z * fast_sqrt(1.0f + sx * sx);
}
RENE_DEV f3 tr_sample_wh(float ax, float ay, f3 wo, Pcg& rng) {  // microfacet.rs:124-138, 176-190
  bool flip = wo.z < 0.0f;
  f3 wi = flip ? -wo : wo;
  f3 ws = normalize(mk3(ax * wi.x, ay * wi.y, wi.z));
  float sx, sy;
  tr_sample11(ws.z, rng, sx, sy);
  float cp = cos_phi(ws), spv = sin_phi(ws);
  float slope_x = cp * sx - spv * sy;
  float slope_y = spv * sx + cp * sy;
  slope_x = ax * slope_x;
  slope_y = ay * slope_y;
  f3 wh = normalize(mk3(-slope_x, -slope_y, 1.0f));
  return flip ? -wh : wh;
}

// ---- BxDFs, bxdf.rs ---------------------------------------------------------------------------------------
RENE_DEV uint32_t lobe_kind(uint32_t type) {
  switch (type) {
    case BX_LAMBERT: case BX_FRESNEL_BLEND: case BX_MICROFACET: return K_REFLECTION | K_DIFFUSE;  // bxdf.rs:83, 262, 357
    case BX_FRESNEL_SPECULAR: return K_REFLECTION | K_TRANSMISSION;                               // bxdf.rs:185
    case BX_SPEC_REFL: return K_REFLECTION;                                                       // bxdf.rs:429
    default: return K_TRANSMISSION;                                                               // bxdf.rs:473
  }
}
RENE_DEV f3 reflect(f3 wo, f3 n) { return -wo + 2.0f * dot(wo, n) * n; }
RENE_DEV bool refract(f3 wi, f3 n, float eta, f3& out) {  // bxdf.rs:121-136
  float cos_i = dot(n, wi);
  float sin2_i = fmaxf(1.0f - cos_i * cos_i, 0.0f);
  float sin2_t = eta * eta * sin2_i;
  if (sin2_t >= 1.0f) {
    out = splat(0.0f);
    return false;
  }
  float cos_t = fast_sqrt(1.0f - sin2_t);
  out = eta * -wi + (eta * cos_i - cos_t) * n;
  return true;
}
RENE_DEV float pow5(float v) { return (v * v) * (v * v) * v; }

template <uint32_t GENERAL, uint32_t TRIM = 0>
RENE_DEV f3 lobe_f(const Lobe& l, f3 wo, f3 wi) {
  if constexpr (trim_albedo_pi(TRIM)) return l.a;  // kd * (1 / pi), from compute_bsdf
  if (!GENERAL || l.type == BX_LAMBERT) return l.a * kInvPi;  // bxdf.rs:87-89
  if (RENE_KIND_ON(BX_FRESNEL_BLEND) && l.type == BX_FRESNEL_BLEND) {                           // bxdf.rs:266-290
    f3 diffuse = (28.0f / (23.0f * kPi)) * l.a * (splat(1.0f) - l.b) *
                 (1.0f - pow5(1.0f - 0.5f * abs_cos_theta(wi))) * (1.0f - pow5(1.0f - 0.5f * abs_cos_theta(wo)));
    f3 wh = wi + wo;
    if (is_zero(wh)) return splat(0.0f);
    wh = normalize(wh);
    float c = dot(wi, wh);
    f3 schlick = l.b + pow5(1.0f - c) * (splat(1.0f) - l.b);
    f3 specular = qdiv(tr_d(l.ax, l.ay, wh), 4.0f * fabsf(c) * fmaxf(abs_cos_theta(wi), abs_cos_theta(wo))) * schlick;
    return diffuse + specular;
  }
  if (RENE_KIND_ON(BX_MICROFACET) && l.type == BX_MICROFACET) {  // bxdf.rs:361-381
    float co = abs_cos_theta(wo), ci = abs_cos_theta(wi);
    f3 wh = wi + wo;
    if (ci == 0.0f || co == 0.0f || is_zero(wh)) return splat(0.0f);
    wh = normalize(wh);
    f3 whf = wh.z < 0.0f ? -wh : wh;  // face_forward(wh, +z), bxdf.rs:348-354
    f3 fr = fresnel_eval(l, dot(wi, whf));
    return l.a * tr_d(l.ax, l.ay, wh) * tr_g(l.ax, l.ay, wo, wi) * fr / (4.0f * ci * co);
  }
  return splat(0.0f);
}
template <uint32_t GENERAL>
RENE_DEV float lobe_pdf(const Lobe& l, f3 wo, f3 wi) {
  if (!GENERAL || l.type == BX_LAMBERT) return same_hemisphere(wo, wi) ? abs_cos_theta(wi) * kInvPi : 0.0f;  // bxdf.rs:107-113
  if (RENE_KIND_ON(BX_FRESNEL_BLEND) && l.type == BX_FRESNEL_BLEND) {  // bxdf.rs:318-328
    if (!same_hemisphere(wo, wi)) return 0.0f;
    f3 wh = normalize(wo + wi);
    return 0.5f * (abs_cos_theta(wi) * kInvPi + qdiv(tr_pdf(l.ax, l.ay, wo, wh), 4.0f * dot(wo, wh)));
  }
  if (RENE_KIND_ON(BX_MICROFACET) && l.type == BX_MICROFACET) {  // bxdf.rs:407-414
    if (!same_hemisphere(wo, wi)) return 0.0f;
    f3 wh = normalize(wo + wi);
    return qdiv(tr_pdf(l.ax, l.ay, wo, wh), 4.0f * dot(wo, wh));
  }
  return 0.0f;
}
struct Sampled {
  f3 wi, f;
  float pdf;
};
RENE_DEV Sampled sampled_default() { return Sampled{splat(0.0f), splat(0.0f), 0.0f}; }

template <uint32_t GENERAL, uint32_t TRIM = 0>
RENE_DEV Sampled lobe_sample(const Lobe& l, f3 wo, Pcg& rng) {
  Sampled s;
  if (!GENERAL || l.type == BX_LAMBERT) {  // bxdf.rs:91-105
    f3 wi = random_cosine_direction(rng);
    if (wo.z < 0.0f) wi.z = -wi.z;
    s.wi = wi;
    s.pdf = same_hemisphere(wo, wi) ? abs_cos_theta(wi) * kInvPi : 0.0f;
    if constexpr (trim_albedo_pi(TRIM)) s.f = l.a;  // kd * (1 / pi), from compute_bsdf
    else s.f = l.a * kInvPi;
    return s;
  }
  switch (l.type) {
    case BX_FRESNEL_SPECULAR: { if (!RENE_KIND_ON(BX_FRESNEL_SPECULAR)) break;  // bxdf.rs:193-227
      float ir = l.a.x;
      float fr = fr_dielectric(wo.z, 1.0f, ir);
      if (pcg_f32(rng) < fr) {
        f3 wi = mk3(-wo.x, -wo.y, wo.z);
        s.wi = wi;
        s.f = splat(fr) / abs_cos_theta(wi);
        s.pdf = fr;
        return s;
      }
      float eta_i = wo.z > 0.0f ? 1.0f : ir, eta_t = wo.z > 0.0f ? ir : 1.0f;
      f3 wi;
      bool ok = refract(wo, mk3(0.0f, 0.0f, wo.z > 0.0f ? 1.0f : -1.0f), qdiv(eta_i, eta_t), wi);
      s.wi = wi;
      s.f = splat(1.0f) * (1.0f - fr) / abs_cos_theta(wi);
      s.pdf = ok ? 1.0f - fr : 0.0f;
      return s;
    }
    case BX_FRESNEL_BLEND: { if (!RENE_KIND_ON(BX_FRESNEL_BLEND)) break;  // bxdf.rs:292-316
      f3 wi;
      if (pcg_f32(rng) < 0.5f) {
        wi = random_cosine_direction(rng);
        if (wo.z < 0.0f) wi.z = -wi.z;
      } else {
        f3 wh = tr_sample_wh(l.ax, l.ay, wo, rng);
        wi = reflect(wo, wh);
        if (!same_hemisphere(wo, wi)) return sampled_default();
      }
      s.wi = wi;
      s.f = lobe_f<GENERAL>(l, wo, wi);
      s.pdf = lobe_pdf<GENERAL>(l, wo, wi);
      return s;
    }
    case BX_MICROFACET: { if (!RENE_KIND_ON(BX_MICROFACET)) break;  // bxdf.rs:383-405
      if (wo.z == 0.0f) return sampled_default();
      f3 wh = tr_sample_wh(l.ax, l.ay, wo, rng);
      if (dot(wo, wh) < 0.0f) return sampled_default();
      f3 wi = reflect(wo, wh);
      if (!same_hemisphere(wo, wi)) return sampled_default();
      s.pdf = qdiv(tr_pdf(l.ax, l.ay, wo, wh), 4.0f * dot(wo, wh));
      s.wi = wi;
      s.f = lobe_f<GENERAL>(l, wo, wi);
      return s;
    }
    case BX_SPEC_REFL: { if (!RENE_KIND_ON(BX_SPEC_REFL)) break;  // bxdf.rs:437-443
      f3 wi = mk3(-wo.x, -wo.y, wo.z);
      s.wi = wi;
      s.f = fresnel_eval(l, wi.z) * l.a / abs_cos_theta(wi);
      s.pdf = 1.0f;
      return s;
    }
    default: {  // SpecularTransmission, bxdf.rs:481-512
      bool entering = wo.z > 0.0f;
      float eta_a = l.b.x, eta_b = l.b.y;
      float eta_i = entering ? eta_a : eta_b, eta_t = entering ? eta_b : eta_a;
      f3 wi;
      if (!refract(wo, mk3(0.0f, 0.0f, wo.z > 0.0f ? 1.0f : -1.0f), qdiv(eta_i, eta_t), wi)) return sampled_default();
      float fx = fr_dielectric(wi.z, eta_a, eta_b);
      s.wi = wi;
      s.f = l.a * (splat(1.0f) - splat(fx)) / abs_cos_theta(wi);
      s.pdf = 1.0f;
      return s;
    }
  }
}

// ---- Bsdf, reflection.rs:228-343: up to MAXL lobes held in registers (static indices only) ----------
// A BSDF is one full lobe (every single-lobe material) or, for Uber / Plastic, up to five lobes kept as the
// parameters they are built from -- a colour per lobe, a 3-bit code per lobe, one pair of alphas and one eta -- and
// rebuilt one at a time where they are used.  (Five full 64-byte lobes were an array the compiler kept in scratch
// memory: 376 bytes per lane and 310+ VGPRs for the multi-lobe kernels.)
enum : uint32_t { ML_TRANS_OPACITY = 0, ML_LAMBERT = 1, ML_MICROFACET = 2, ML_SPEC_REFL = 3, ML_SPEC_TRANS = 4 };
template <int MAXL>
struct Bsdf {
  f3 ng;
  Onb onb;
  uint32_t len;
  Lobe l0;           // len == 1 and codes == 0xffffffff: the lobe itself
  uint32_t codes;    // multi-lobe: ML_* of lobe i in bits 3i .. 3i+2
  f3 c0, c1, c2, c3, c4;  // multi-lobe: colour of lobe i
  float ax, ay, eta_i, eta_t;
};
template <int MAXL>
RENE_DEV void bsdf_push(Bsdf<MAXL>& b, const Lobe& lobe) {  // a single-lobe material
  b.l0 = lobe;
  b.codes = 0xffffffffu;
  b.len = 1;
}
template <int MAXL>
RENE_DEV void bsdf_push_multi(Bsdf<MAXL>& b, uint32_t code, f3 colour) {
  const uint32_t i = b.len;
  if (i == 0u) b.c0 = colour;
  if (i == 1u) b.c1 = colour;
  if (i == 2u) b.c2 = colour;
  if (i == 3u) b.c3 = colour;
  if (i == 4u) b.c4 = colour;
  b.codes = (b.codes & ~(7u << (3u * i))) | (code << (3u * i));
  b.len = i + 1u;
}
// lobe i (a compile-time constant after unrolling) of a BSDF
template <int MAXL>
RENE_DEV Lobe bsdf_lobe(const Bsdf<MAXL>& b, int i) {
  if (MAXL == 1) return b.l0;
  // one return, chosen field by field: two struct-valued return paths become an aggregate copy through scratch
  const bool one = b.codes == 0xffffffffu;
  const uint32_t code = (b.codes >> (3u * (uint32_t)i)) & 7u;
  const f3 colour = i == 0 ? b.c0 : (i == 1 ? b.c1 : (i == 2 ? b.c2 : (i == 3 ? b.c3 : b.c4)));
  const float eta_b = code == ML_SPEC_TRANS ? b.eta_t : 1.0f;  // SpecularTransmission: eta_a = 1, eta_b
  Lobe l;
  l.type = one ? b.l0.type
               : (code == ML_LAMBERT ? (uint32_t)BX_LAMBERT : (code == ML_MICROFACET ? (uint32_t)BX_MICROFACET : (code == ML_SPEC_REFL ? (uint32_t)BX_SPEC_REFL : (uint32_t)BX_SPEC_TRANS)));
  l.a = mk3(one ? b.l0.a.x : colour.x, one ? b.l0.a.y : colour.y, one ? b.l0.a.z : colour.z);
  l.b = mk3(one ? b.l0.b.x : 1.0f, one ? b.l0.b.y : eta_b, one ? b.l0.b.z : 0.0f);
  l.ax = one ? b.l0.ax : b.ax;
  l.ay = one ? b.l0.ay : b.ay;
  l.fr = one ? b.l0.fr : (uint32_t)FR_DIELECTRIC;
  l.eta = mk3(one ? b.l0.eta.x : b.eta_i, one ? b.l0.eta.y : b.eta_t, one ? b.l0.eta.z : 0.0f);
  l.k = mk3(one ? b.l0.k.x : 0.0f, one ? b.l0.k.y : 0.0f, one ? b.l0.k.z : 0.0f);
  return l;
}
template <int MAXL, uint32_t GENERAL>
RENE_DEV bool bsdf_contains(const Bsdf<MAXL>& b, uint32_t kind) {  // reflection.rs:267-282
  if (!GENERAL) return b.len > 0 && (kind & (K_REFLECTION | K_DIFFUSE));
  bool r = false;
#pragma unroll
  for (int i = 0; i < MAXL; ++i)
    if ((uint32_t)i < b.len && (lobe_kind(bsdf_lobe(b, i).type) & kind)) r = true;
  return r;
}
// TRIM (the Matte small-scene kernels, bounce_trims): TRIM_UNIT_LEN where the caller knows b.len == 1 -- the tests against it and the divisions
// by it go.  p * rcp(1) is p bit for bit: v_rcp_f32(1.0f) is exactly 1.0f (selftest/onb_probe.hip checks it on the device), and the multiply by
// it could only change a denormal p, which it flushes -- but p is 0, or |cos theta| * (1 / pi) out of a v_mul_f32 that has flushed its own result
// already, or a sum with 0 of such; and the consumers (0.5 * p + q, p < 1e-5) flush their inputs like the multiply did (the probe runs both).
template <int MAXL, uint32_t GENERAL, uint32_t TRIM = 0>
RENE_DEV f3 bsdf_f(const Bsdf<MAXL>& b, f3 wo_world, f3 wi_world) {  // reflection.rs:286-309
  f3 wi = to_local(b.onb, wi_world);
  f3 wo = to_local(b.onb, wo_world);
  if (wo.z == 0.0f) return splat(0.0f);
  bool refl = dot(wi_world, b.ng) * dot(wo_world, b.ng) > 0.0f;
  f3 f = splat(0.0f);
#pragma unroll
  for (int i = 0; i < MAXL; ++i) {
    if ((TRIM & TRIM_UNIT_LEN) || (uint32_t)i < b.len) {
      const Lobe l = bsdf_lobe(b, i);
      uint32_t k = GENERAL ? lobe_kind(l.type) : (K_REFLECTION | K_DIFFUSE);
      if ((refl && (k & K_REFLECTION)) || (!refl && (k & K_TRANSMISSION))) f = f + lobe_f<GENERAL, TRIM>(l, wo, wi);
    }
  }
  return f;
}
template <int MAXL, uint32_t GENERAL, uint32_t TRIM = 0>
RENE_DEV float bsdf_pdf(const Bsdf<MAXL>& b, f3 wo_world, f3 wi_world) {  // reflection.rs:328-342
  float p = 0.0f;
  f3 wo = to_local(b.onb, wo_world);
  f3 wi = to_local(b.onb, wi_world);
#pragma unroll
  for (int i = 0; i < MAXL; ++i)
    if ((TRIM & TRIM_UNIT_LEN) || (uint32_t)i < b.len) p += lobe_pdf<GENERAL>(bsdf_lobe(b, i), wo, wi);
  if constexpr ((TRIM & TRIM_UNIT_LEN) != 0u) return p;
  return qdiv(p, (float)b.len);
}
template <int MAXL, uint32_t GENERAL, uint32_t TRIM = 0>
RENE_DEV Sampled bsdf_sample(const Bsdf<MAXL>& b, f3 wo_world, Pcg& rng) {  // reflection.rs:311-326
  static_assert(!(TRIM & TRIM_UNIT_LEN) || MAXL == 1, "one lobe");
  if (!(TRIM & TRIM_UNIT_LEN) && b.len == 0) return sampled_default();
  uint32_t index = umod(pcg_u32(rng), (TRIM & TRIM_UNIT_LEN) ? 1u : b.len);
  f3 wo = to_local(b.onb, wo_world);
  Sampled s = sampled_default();
  if (MAXL == 1) {
    s = lobe_sample<GENERAL, TRIM>(b.l0, wo, rng);
  } else {
    // the sampled lobe, chosen field by field (a whole-struct assignment is an aggregate copy through scratch)
    Lobe sel = bsdf_lobe(b, 0);
#pragma unroll
    for (int i = 1; i < MAXL; ++i) {
      const Lobe t = bsdf_lobe(b, i);
      const bool pick = (uint32_t)i == index;
      sel.type = pick ? t.type : sel.type;
      sel.a = mk3(pick ? t.a.x : sel.a.x, pick ? t.a.y : sel.a.y, pick ? t.a.z : sel.a.z);
      sel.b = mk3(pick ? t.b.x : sel.b.x, pick ? t.b.y : sel.b.y, pick ? t.b.z : sel.b.z);
      sel.ax = pick ? t.ax : sel.ax;
      sel.ay = pick ? t.ay : sel.ay;
      sel.fr = pick ? t.fr : sel.fr;
      sel.eta = mk3(pick ? t.eta.x : sel.eta.x, pick ? t.eta.y : sel.eta.y, pick ? t.eta.z : sel.eta.z);
      sel.k = mk3(pick ? t.k.x : sel.k.x, pick ? t.k.y : sel.k.y, pick ? t.k.z : sel.k.z);
    }
    s = lobe_sample<GENERAL>(sel, wo, rng);
  }
  if constexpr (!(TRIM & TRIM_UNIT_LEN)) s.pdf = qdiv(s.pdf, (float)b.len);
  s.wi = to_world(b.onb, s.wi);
  return s;
}

RENE_DEV Lobe lobe_zero() {
  Lobe l;
  l.type = BX_LAMBERT;
  l.a = splat(0.0f);
  l.b = splat(0.0f);
  l.ax = 0.0f;
  l.ay = 0.0f;
  l.fr = FR_CONDUCTOR;
  l.eta = splat(0.0f);
  l.k = splat(0.0f);
  return l;
}

// EnumMaterial::albedo, material.rs:720-737
template <uint32_t FEAT, uint32_t TRIM = 0>
RENE_DEV f3 material_albedo(const SceneView& S, const Inst& inst, uv2 uv) {
  if (inst.kd[3] != 0.0f) return mk3(inst.kd[0], inst.kd[1], inst.kd[2]);
  if constexpr ((TRIM & TRIM_STATIC_MATTE) != 0u) return splat(0.0f);  // material None (compute_bsdf below)
  const Material& m = S.materials[inst.material];
  switch (m.type) {
    case RENE_MATERIAL_MATTE: case RENE_MATERIAL_SUBSTRATE: case RENE_MATERIAL_MIRROR:
    case RENE_MATERIAL_UBER: case RENE_MATERIAL_PLASTIC:
      return tex_color<FEAT>(S, m.u0[0], uv);
    case RENE_MATERIAL_METAL: return tex_color<FEAT>(S, m.u0[1], uv);  // k, material.rs:309-316
    default: return splat(0.0f);
  }
}

// EnumMaterial::compute_bsdf, material.rs:739-769
template <uint32_t FEAT, int MAXL, uint32_t TRIM = 0>
RENE_DEV void compute_bsdf(const SceneView& S, const Inst& inst, uv2 uv, Bsdf<MAXL>& b) {
  if (inst.kd[3] != 0.0f) {  // Matte over a solid texture (material.rs:127-135), resolved at upload
    Lobe l = lobe_zero();
    l.a = mk3(inst.kd[0], inst.kd[1], inst.kd[2]);
    if constexpr (trim_albedo_pi(TRIM)) l.a = l.a * kInvPi;  // what lobe_f and lobe_sample return, once for both sides of the coin
    bsdf_push(b, l);
    return;
  }
  // TRIM_STATIC_MATTE: a kernel with neither FEAT_TEXTURES nor a general lobe kind has no table to walk.  The packer resolves every Matte
  // instance over a Solid texture into kd (.w = 1), and without FEAT_TEXTURES every texture is Solid (scene_pack.cpp refuses a scene where one
  // is left unresolved): kd.w == 0 is material None, no lobe.
  static_assert(!(TRIM & TRIM_STATIC_MATTE) || (!(FEAT & FEAT_TEXTURES) && lobe_kinds(FEAT) == 0u), "Matte over solid textures only");
  if constexpr ((TRIM & TRIM_STATIC_MATTE) != 0u) return;
  constexpr uint32_t GENERAL = lobe_kinds(FEAT);
  if ((FEAT & FEAT_TEXTURES) && inst.res_type == INST_RES_MATTE_CHECKER) {  // texture.rs:97-118 with both children solid
    const float x = uv.x * inst.res_ru, y = uv.y * inst.res_rv;
    const bool same = (f32_to_u32(x) % 2u == 0u) == (f32_to_u32(y) % 2u == 0u);
    Lobe l = lobe_zero();
    l.a = same ? mk3(inst.res_c0[0], inst.res_c0[1], inst.res_c0[2]) : mk3(inst.res_c1[0], inst.res_c1[1], inst.res_c1[2]);
    bsdf_push(b, l);
    return;
  }
  if ((FEAT & FEAT_GENERAL_BSDF) && inst.res_type != 0u && inst.res_type != INST_RES_MATTE_CHECKER) {  // a single-lobe material over solid textures, resolved at upload (Inst::res_*)
    Lobe l = lobe_zero();
    const f3 c0 = mk3(inst.res_c0[0], inst.res_c0[1], inst.res_c0[2]), c1 = mk3(inst.res_c1[0], inst.res_c1[1], inst.res_c1[2]);
    float ru = inst.res_ru, rv = inst.res_rv;
    if (inst.res_remap != 0u) {
      ru = roughness_to_alpha(ru);
      rv = roughness_to_alpha(rv);
    }
    switch (inst.res_type) {
      case RENE_MATERIAL_GLASS: if (!RENE_KIND_ON(BX_FRESNEL_SPECULAR)) return;
        l.type = BX_FRESNEL_SPECULAR;
        l.a.x = c0.x;
        break;
      case RENE_MATERIAL_SUBSTRATE: if (!RENE_KIND_ON(BX_FRESNEL_BLEND)) return;
        l.type = BX_FRESNEL_BLEND;
        l.a = c0;
        l.b = c1;
        l.ax = ru;
        l.ay = rv;
        break;
      case RENE_MATERIAL_METAL: if (!RENE_KIND_ON(BX_MICROFACET)) return;
        l.type = BX_MICROFACET;
        l.a = splat(1.0f);
        l.ax = ru;
        l.ay = rv;
        l.fr = FR_CONDUCTOR;
        l.eta = c0;
        l.k = c1;
        break;
      default: if (!RENE_KIND_ON(BX_SPEC_REFL)) return;  // RENE_MATERIAL_MIRROR
        l.type = BX_SPEC_REFL;
        l.a = c0;
        l.fr = FR_NOOP;
        break;
    }
    bsdf_push(b, l);
    return;
  }
  const Material& m = S.materials[inst.material];
  uint32_t type = m.type;
  if (type == RENE_MATERIAL_MATTE) {
    Lobe l = lobe_zero();
    l.a = tex_color<FEAT>(S, m.u0[0], uv);
    bsdf_push(b, l);
    return;
  }
  if (!(FEAT & FEAT_GENERAL_BSDF)) return;
  switch (type) {
    case RENE_MATERIAL_GLASS: { if (!RENE_KIND_ON(BX_FRESNEL_SPECULAR)) break;  // material.rs:342-350
      Lobe l = lobe_zero();
      l.type = BX_FRESNEL_SPECULAR;
      l.a.x = m.v0[0];
      bsdf_push(b, l);
      break;
    }
    case RENE_MATERIAL_SUBSTRATE: { if (!RENE_KIND_ON(BX_FRESNEL_BLEND)) break;  // material.rs:188-216
      Lobe l = lobe_zero();
      l.type = BX_FRESNEL_BLEND;
      l.a = tex_color<FEAT>(S, m.u0[0], uv);
      l.b = tex_color<FEAT>(S, m.u0[1], uv);
      float ru = tex_color<FEAT>(S, m.u0[2], uv).x, rv = tex_color<FEAT>(S, m.u0[3], uv).x;
      if (m.u1[0] != 0) {
        ru = roughness_to_alpha(ru);
        rv = roughness_to_alpha(rv);
      }
      l.ax = ru;
      l.ay = rv;
      bsdf_push(b, l);
      break;
    }
    case RENE_MATERIAL_METAL: { if (!RENE_KIND_ON(BX_MICROFACET)) break;  // material.rs:279-307
      Lobe l = lobe_zero();
      l.type = BX_MICROFACET;
      float ru = tex_color<FEAT>(S, m.u0[2], uv).x, rv = tex_color<FEAT>(S, m.u0[3], uv).x;
      if (m.u1[0] != 0) {
        ru = roughness_to_alpha(ru);
        rv = roughness_to_alpha(rv);
      }
      l.a = splat(1.0f);
      l.ax = ru;
      l.ay = rv;
      l.fr = FR_CONDUCTOR;
      l.eta = tex_color<FEAT>(S, m.u0[0], uv);
      l.k = tex_color<FEAT>(S, m.u0[1], uv);
      bsdf_push(b, l);
      break;
    }
    case RENE_MATERIAL_MIRROR: { if (!RENE_KIND_ON(BX_SPEC_REFL)) break;  // material.rs:363-373
      Lobe l = lobe_zero();
      l.type = BX_SPEC_REFL;
      l.a = tex_color<FEAT>(S, m.u0[0], uv);
      l.fr = FR_NOOP;
      bsdf_push(b, l);
      break;
    }
    case RENE_MATERIAL_UBER: {  // material.rs:579-630
      if (MAXL < 5) break;
      float e = m.v0[0];
      b.codes = 0u;
      b.eta_i = 1.0f;
      b.eta_t = e;
      b.ax = 0.0f;
      b.ay = 0.0f;
      f3 op = tex_color<FEAT>(S, m.u1[0], uv);
      f3 t = splat(1.0f) - op;
      if (!is_zero(t)) bsdf_push_multi(b, ML_TRANS_OPACITY, t);  // SpecularTransmission(t, 1, 1)
      f3 kd = tex_color<FEAT>(S, m.u0[0], uv);
      if (!is_zero(kd)) bsdf_push_multi(b, ML_LAMBERT, kd);
      f3 ks = tex_color<FEAT>(S, m.u0[1], uv);
      if (!is_zero(ks)) {  // MicrofacetReflection(ks, TrowbridgeReitz, dielectric(1, e))
        float ru = tex_color<FEAT>(S, m.u1[2], uv).x, rv = tex_color<FEAT>(S, m.u1[3], uv).x;
        if (m.u1[1] != 0) {
          ru = roughness_to_alpha(ru);
          rv = roughness_to_alpha(rv);
        }
        b.ax = ru;
        b.ay = rv;
        bsdf_push_multi(b, ML_MICROFACET, ks);
      }
      f3 kr = op * tex_color<FEAT>(S, m.u0[2], uv);
      if (!is_zero(kr)) bsdf_push_multi(b, ML_SPEC_REFL, kr);  // SpecularReflection(kr, dielectric(1, e))
      f3 kt = op * tex_color<FEAT>(S, m.u0[3], uv);
      if (!is_zero(kt)) bsdf_push_multi(b, ML_SPEC_TRANS, kt);  // SpecularTransmission(kt, 1, e)
      break;
    }
    case RENE_MATERIAL_PLASTIC: {  // material.rs:680-707
      if (MAXL < 2) break;
      b.codes = 0u;
      b.eta_i = 1.5f;
      b.eta_t = 1.0f;
      b.ax = 0.0f;
      b.ay = 0.0f;
      f3 kd = tex_color<FEAT>(S, m.u0[0], uv);
      if (!is_zero(kd)) bsdf_push_multi(b, ML_LAMBERT, kd);
      f3 ks = tex_color<FEAT>(S, m.u0[1], uv);
      if (!is_zero(ks)) {  // MicrofacetReflection(ks, TrowbridgeReitz(rough, rough), dielectric(1.5, 1))
        float rough = tex_color<FEAT>(S, m.u0[3], uv).x;
        if (m.u1[2] != 0) rough = roughness_to_alpha(rough);  // Q8: u1.z is never set, material.rs:674-676
        b.ax = rough;
        b.ay = rough;
        bsdf_push_multi(b, ML_MICROFACET, ks);
      }
      break;
    }
    default: break;  // None: no lobes
  }
}

// =================================================================================================
// hit shaders
// =================================================================================================
struct Surface {
  f3 position, normal;  // normal as the closest-hit shader leaves it (lib.rs:944-951 / 874-880)
  uv2 uv;
  uint32_t instance;
};

// math.rs:70-76
RENE_DEV uv2 sphere_uv(f3 p) {
  float theta = acosf(p.z);
  float phi = atan2f(p.y, p.x);
  if (phi < 0.0f) phi = phi + 2.0f * kPi;
  return uv2{phi * 0.5f * kInvPi, (theta - kPi) * -kInvPi};
}

template <bool SPHERES>
RENE_DEV Surface shade_hit(const SceneView& S, const HitRec& h, f3 ro, f3 rd) {
  Surface sf;
  const float* q = S.main.isect[h.slot].q;
  float4 c = ldg4(q + 8);
  sf.instance = __float_as_uint(c.y);
  uint32_t sidx = __float_as_uint(c.w);
  if (SPHERES && sidx != 0xffffffffu) {  // sphere_closest_hit, lib.rs:852-881
    const Sphere& sp = S.spheres[sidx];
    f3 oo = aff_point(sp.w2o, ro), od = aff_vector(sp.w2o, rd);
    f3 ohp = oo + h.t * od;
    sf.position = ro + h.t * rd;
    sf.uv = sphere_uv(ohp);
    // normal = (w2o.x . p, w2o.y . p, w2o.z . p) with w2o.{x,y,z} the COLUMNS of world_to_object
    sf.normal = mk3(sp.w2o[0] * ohp.x + sp.w2o[1] * ohp.y + sp.w2o[2] * ohp.z,
                    sp.w2o[3] * ohp.x + sp.w2o[4] * ohp.y + sp.w2o[5] * ohp.z,
                    sp.w2o[6] * ohp.x + sp.w2o[7] * ohp.y + sp.w2o[8] * ohp.z);
    return sf;
  }
  // triangle_closest_hit, lib.rs:892-952 (vertices are pre-transformed to world space)
  float4 a = ldg4(q), b = ldg4(q + 4);
  f3 p0 = mk3(a.x, a.y, a.z), e1 = mk3(a.w, b.x, b.y), e2 = mk3(b.z, b.w, c.x);
  sf.position = p0 + h.u * e1 + h.v * e2;
  const float* s = S.shade[h.slot].q;
  float4 s0 = ldg4(s), s1 = ldg4(s + 4), s2 = ldg4(s + 8), s3 = ldg4(s + 12);
  float b0 = 1.0f - h.u - h.v;
  sf.normal = normalize(mk3(s0.x, s0.y, s0.z) * b0 + mk3(s1.x, s1.y, s1.z) * h.u + mk3(s2.x, s2.y, s2.z) * h.v);
  sf.uv = uv2{s0.w * b0 + s2.w * h.u + s3.y * h.v, s1.w * b0 + s3.x * h.u + s3.z * h.v};
  return sf;
}

// *_closest_hit_pdf / main_miss_pdf, lib.rs:959-1066
template <bool SPHERES>
RENE_DEV float emitter_pdf(const SceneView& S, const HitRec& h, f3 ro, f3 rd) {
  if (h.slot == 0xffffffffu) return 0.0f;
  const float* q = S.emit.isect[h.slot].q;
  float4 c = ldg4(q + 8);
  uint32_t inst = __float_as_uint(c.y);
  uint32_t sidx = __float_as_uint(c.w);
  if (SPHERES && sidx != 0xffffffffu) {  // Q4, lib.rs:1047-1066
    const float* m = S.spheres[sidx].o2w;
    float radius = (fabsf(m[0]) + fabsf(m[4]) + fabsf(m[8])) / 3.0f;
    f3 center = mk3(m[9], m[10], m[11]);
    float cos_theta_max = fast_sqrt(fmaxf(1.0f - qdiv(radius * radius, length_squared(center - ro)), 0.0f));
    float solid_angle = 2.0f * kPi * (1.0f - cos_theta_max);
    return fast_rcp(solid_angle);
  }
  float4 a = ldg4(q), b = ldg4(q + 4);
  f3 p0 = mk3(a.x, a.y, a.z), e1 = mk3(a.w, b.x, b.y), e2 = mk3(b.z, b.w, c.x);
  f3 hit_pos = p0 + h.u * e1 + h.v * e2;
  float4 pr = ldg4(S.emit_pdf[h.slot].q);
  float distance_squared = length_squared(ro - hit_pos);
  float cosine = fabsf(dot(normalize(rd), mk3(pr.x, pr.y, pr.z)));
  return qdiv(qdiv(distance_squared, cosine * pr.w), S.insts[inst].primitive_count);
}

// EnumSurfaceSample::sample, surface_sample.rs:69-117
template <bool SPHERES>
RENE_DEV f3 emit_sample(const SceneView& S, uint32_t obj, Pcg& rng) {
  const EmitObject& e = S.emit_objects[obj];
  if (SPHERES && e.type == 1) {
    f3 v = normalize(random_in_unit_sphere(rng));
    return aff_point(e.matrix, v);
  }
  uint32_t p = umod(pcg_u32(rng), e.prim_count);  // Q6
  const float* q = S.emit_tris[e.first_tri + p].q;
  float4 a = ldg4(q), b = ldg4(q + 4), c = ldg4(q + 8);
  float r = pcg_f32(rng);
  float s = pcg_f32(rng);
  if (r + s > 1.0f) {
    r = 1.0f - r;
    s = 1.0f - s;
  }
  return mk3(a.x, a.y, a.z) * (1.0f - r - s) + mk3(a.w, b.x, b.y) * r + mk3(b.z, b.w, c.x) * s;
}

// ---- the same three steps over the LDS-resident tables of a small scene (SmallLds): one index, every load of the
// step issued at once ----------------------------------------------------------------------------------------------
RENE_DEV Inst inst_from(float4 i0, float4 i1, float4 i2, float4 i3, float4 i4, float4 i5) {
  Inst in;
  in.res_type = __float_as_uint(i3.x);
  in.res_remap = __float_as_uint(i3.y);
  in.res_ru = i3.z;
  in.res_rv = i3.w;
  in.res_c0[0] = i4.x; in.res_c0[1] = i4.y; in.res_c0[2] = i4.z; in.res_c0[3] = i4.w;
  in.res_c1[0] = i5.x; in.res_c1[1] = i5.y; in.res_c1[2] = i5.z; in.res_c1[3] = i5.w;
  in.material = __float_as_uint(i0.x);
  in.area_light = __float_as_uint(i0.y);
  in.primitive_count = i0.z;
  in.material_type = __float_as_uint(i0.w);
  in.kd[0] = i1.x; in.kd[1] = i1.y; in.kd[2] = i1.z; in.kd[3] = i1.w;
  in.emit[0] = i2.x; in.emit[1] = i2.y; in.emit[2] = i2.z; in.emit[3] = i2.w;
  return in;
}
template <bool SPHERES>
RENE_DEV Surface shade_hit_lds(const SceneView& S, const SmallLds& T, const HitRec& h, f3 ro, f3 rd, Inst& inst) {
  Surface sf;
  lds_ptr q = T.hit + SMALL_HIT_FLOATS * h.slot;
  const float4 a = lds4(q), b = lds4(q + 4), c = lds4(q + 8);
  const float4 s0 = lds4(q + 12), s1 = lds4(q + 16), s2 = lds4(q + 20), s3 = lds4(q + 24);
  inst = inst_from(lds4(q + 28), lds4(q + 32), lds4(q + 36), lds4(q + 40), lds4(q + 44), lds4(q + 48));
  sf.instance = __float_as_uint(c.y);
  uint32_t sidx = __float_as_uint(c.w);
  if (SPHERES && sidx != 0xffffffffu) {  // sphere_closest_hit, lib.rs:852-881
    const lds_ptr sq = T.spheres + 24u * sidx + 12u;  // Sphere::w2o
    const float4 w0 = lds4(sq), w1 = lds4(sq + 4), w2 = lds4(sq + 8);
    const float w2o[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
    f3 oo = aff_point(w2o, ro), od = aff_vector(w2o, rd);
    f3 ohp = oo + h.t * od;
    sf.position = ro + h.t * rd;
    sf.uv = sphere_uv(ohp);
    sf.normal = mk3(w2o[0] * ohp.x + w2o[1] * ohp.y + w2o[2] * ohp.z,
                    w2o[3] * ohp.x + w2o[4] * ohp.y + w2o[5] * ohp.z,
                    w2o[6] * ohp.x + w2o[7] * ohp.y + w2o[8] * ohp.z);
    return sf;
  }
  // triangle_closest_hit, lib.rs:892-952 (vertices are pre-transformed to world space)
  f3 p0 = mk3(a.x, a.y, a.z), e1 = mk3(a.w, b.x, b.y), e2 = mk3(b.z, b.w, c.x);
  sf.position = p0 + h.u * e1 + h.v * e2;
  float b0 = 1.0f - h.u - h.v;
  sf.normal = normalize(mk3(s0.x, s0.y, s0.z) * b0 + mk3(s1.x, s1.y, s1.z) * h.u + mk3(s2.x, s2.y, s2.z) * h.v);
  sf.uv = uv2{s0.w * b0 + s2.w * h.u + s3.y * h.v, s1.w * b0 + s3.x * h.u + s3.z * h.v};
  return sf;
}
// NORMALISED: rd is normalize() of the ray's direction already (the caller shares it with the hit branch's wo)
template <bool SPHERES, bool NORMALISED = false>
RENE_DEV float emitter_pdf_lds(const SceneView& S, const SmallLds& T, const HitRec& h, f3 ro, f3 rd) {
  if (h.slot == 0xffffffffu) return 0.0f;
  lds_ptr q = T.emit + SMALL_EMIT_FLOATS * h.slot;
  const float4 a = lds4(q), b = lds4(q + 4), c = lds4(q + 8), pr = lds4(q + 12);
  const float primitive_count = q[16];
  uint32_t sidx = __float_as_uint(c.w);
  if (SPHERES && sidx != 0xffffffffu) {  // Q4, lib.rs:1047-1066
    const lds_ptr sq = T.spheres + 24u * sidx;  // Sphere::o2w
    const float4 m0 = lds4(sq), m1 = lds4(sq + 4), m2 = lds4(sq + 8);
    const float m[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
    float radius = (fabsf(m[0]) + fabsf(m[4]) + fabsf(m[8])) / 3.0f;
    f3 center = mk3(m[9], m[10], m[11]);
    float cos_theta_max = fast_sqrt(fmaxf(1.0f - qdiv(radius * radius, length_squared(center - ro)), 0.0f));
    float solid_angle = 2.0f * kPi * (1.0f - cos_theta_max);
    return fast_rcp(solid_angle);
  }
  f3 p0 = mk3(a.x, a.y, a.z), e1 = mk3(a.w, b.x, b.y), e2 = mk3(b.z, b.w, c.x);
  f3 hit_pos = p0 + h.u * e1 + h.v * e2;
  float distance_squared = length_squared(ro - hit_pos);
  float cosine = fabsf(dot(NORMALISED ? rd : normalize(rd), mk3(pr.x, pr.y, pr.z)));
  return qdiv(qdiv(distance_squared, cosine * pr.w), primitive_count);
}
// the emitter query's answer from what the closest-hit loop captured at the emitter item's twin (EmitCapture): the tail of traverse_small
// for a triangle / parallelogram item, on the emitter structure's item 0
RENE_DEV HitRec emit_twin_hit(const SmallLds& T, const EmitCapture& cap, float tmax) {
  HitRec h;
  h.t = tmax;  // (not read: emitter_pdf_lds wants slot, u and v)
  h.u = 0.0f;
  h.v = 0.0f;
  h.slot = 0xffffffffu;
  if (cap.s != -1.0f) {
    const float4 m = lds4(T.items_emit + 12u);  // kind, slot1, slot2, perm1 | perm2 << 8
    const float best_s = cap.s, best_r = cap.r;
    bool second = m.x == SMALL_KIND_QUAD && best_s + best_r > 1.0f;
    uint32_t perm = __float_as_uint(m.w) >> (second ? 8u : 0u);
    float w0 = second ? best_s + best_r - 1.0f : 1.0f - best_s - best_r;
    float w1 = second ? 1.0f - best_r : best_s;
    float w2 = second ? 1.0f - best_s : best_r;
    uint32_t iu = perm & 3u, iv = (perm >> 2) & 3u;
    h.u = iu == 0u ? w0 : (iu == 1u ? w1 : w2);
    h.v = iv == 0u ? w0 : (iv == 1u ? w1 : w2);
    h.slot = __float_as_uint(second ? m.z : m.y);
  }
  return h;
}
template <bool SPHERES>
RENE_DEV f3 emit_sample_lds(const SmallLds& T, uint32_t obj, Pcg& rng) {
  lds_ptr e = T.eobj + 16u * obj;
  const float4 head = lds4(e);  // type, first_tri, prim_count, pad
  if (SPHERES && __float_as_uint(head.x) == 1u) {
    f3 v = normalize(random_in_unit_sphere(rng));
    const float4 m0 = lds4(e + 4), m1 = lds4(e + 8), m2 = lds4(e + 12);
    const float m[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
    return aff_point(m, v);
  }
  uint32_t p = umod(pcg_u32(rng), __float_as_uint(head.z));  // Q6
  lds_ptr q = T.etri + 12u * (__float_as_uint(head.y) + p);
  const float4 a = lds4(q), b = lds4(q + 4), c = lds4(q + 8);
  float r = pcg_f32(rng);
  float s = pcg_f32(rng);
  if (r + s > 1.0f) {
    r = 1.0f - r;
    s = 1.0f - s;
  }
  return mk3(a.x, a.y, a.z) * (1.0f - r - s) + mk3(a.w, b.x, b.y) * r + mk3(b.z, b.w, c.x) * s;
}

// =================================================================================================
// participating media (volpath), rene-shader/src/medium.rs
// =================================================================================================
struct MediumRec {
  f3 sigma_a, sigma_s;
  float g;
  uint32_t type;
};
RENE_DEV MediumRec load_medium(const SceneView& S, uint32_t index) {
  const Medium& m = S.mediums[index];
  float4 a = ldg4(m.sa_g), b = ldg4(m.ss_t);
  return MediumRec{mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), a.w, __float_as_uint(b.w)};
}
RENE_DEV f3 exp3(f3 a) { return mk3(__expf(a.x), __expf(a.y), __expf(a.z)); }
RENE_DEV f3 medium_tr(const MediumRec& m, f3 rd, float t_max) {  // medium.rs:106-108
  return exp3(-(m.sigma_a + m.sigma_s) * length(rd) * t_max);
}
struct SampledMedium {
  bool sampled;
  f3 position, tr;
};
RENE_DEV SampledMedium medium_sample(const MediumRec& m, f3 ro, f3 rd, float t_max, Pcg& rng) {  // medium.rs:110-133
  uint32_t channel = pcg_u32(rng) % 3u;
  f3 sigma_t = m.sigma_a + m.sigma_s;
  float st = channel == 0u ? sigma_t.x : (channel == 1u ? sigma_t.y : sigma_t.z);
  float dist = qdiv(-__logf(1.0f - pcg_f32(rng)), st);
  float len = length(rd);
  float t = qdiv(dist, len);
  bool sampled = t < t_max;
  t = fminf(t, t_max);
  f3 tr = exp3(-sigma_t * t * len);
  f3 density = sampled ? sigma_t * tr : tr;
  float pdf = (density.x + density.y + density.z) / 3.0f;
  if (pdf == 0.0f) pdf = 1.0f;
  return SampledMedium{sampled, ro + t * rd, sampled ? tr * m.sigma_s / pdf : tr / pdf};
}
RENE_DEV float medium_phase(const MediumRec& m, f3 wo, f3 wi) {  // Henyey-Greenstein, medium.rs:135-140
  float cos_theta = dot(wo, wi);
  float denom = 1.0f + m.g * m.g + 2.0f * m.g * cos_theta;
  return qdiv(1.0f / (4.0f * kPi) * (1.0f - m.g * m.g), denom * fast_sqrt(denom));
}
RENE_DEV f3 medium_sample_p(const MediumRec& m, f3 wo, Pcg& rng) {  // medium.rs:142-157
  float u0 = pcg_f32(rng);
  float u1 = pcg_f32(rng);
  float g = m.g;
  float cos_theta;
  if (fabsf(g) < 1e-3f) {
    cos_theta = 1.0f - 2.0f * u0;
  } else {
    float sqr_term = qdiv(1.0f - g * g, 1.0f + g - 2.0f * g * u0);
    cos_theta = qdiv(-(1.0f + g * g - sqr_term * sqr_term), 2.0f * g);
  }
  float sin_theta = fast_sqrt(fmaxf(1.0f - cos_theta * cos_theta, 0.0f));
  Onb o = onb_from_w(wo);  // coordinate_system(wo) -> (v1, v2), math.rs:89-97
  return sin_theta * cos_2pi(u1) * o.u + sin_theta * sin_2pi(u1) * o.v + cos_theta * wo;
}

// =================================================================================================
// the integrator
// =================================================================================================
RENE_DEV uint32_t lane_id() { return __lane_id(); }

// ---- accumulation-image records: 16 bytes = the r, g, b sums of a pixel + the *version* of the work item that
// committed them (epoch << VERSION_LEVEL_BITS | items of the pixel committed so far in that launch), written and read as one aligned
// global_{store,load}_dwordx4 with "sc0 sc1" (write-through / cache-bypassing), so that a pixel's running sums can
// be handed from one lane to another lane on another CU / XCD -- inside a launch, or from one launch to the next.  A reader that finds the version it waits for has the sums that belong to it: one aligned
// 16-byte access of one lane is a single request all the way to memory.  No separate flag, no ordering between a
// pixel's three layer records (each carries its own version), no drain after the stores, and the three loads of an
// item start are in flight together.  No plain load of the image exists in the kernels.  The reference never
// touches alpha (lib.rs:170); rene_download returns 0 there.
typedef float v4f __attribute__((ext_vector_type(4)));
RENE_DEV void fb_store(float* p, f3 a, uint32_t version) {
  v4f v = {a.x, a.y, a.z, __uint_as_float(version)};
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}
RENE_DEV void fb_load1(const float* p, v4f& a) {
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(a) : "v"(p) : "memory");
}
RENE_DEV void fb_load3(const float* p0, const float* p1, const float* p2, v4f& a, v4f& b, v4f& c) {
  asm volatile(
      "global_load_dwordx4 %0, %3, off sc0 sc1\n\tglobal_load_dwordx4 %1, %4, off sc0 sc1\n\t"
      "global_load_dwordx4 %2, %5, off sc0 sc1\n\ts_waitcnt vmcnt(0)"
      : "=&v"(a), "=&v"(b), "=&v"(c)
      : "v"(p0), "v"(p1), "v"(p2)
      : "memory");
}



RENE_DEV unsigned long long wave_sum(uint32_t v) {
  unsigned long long s = v;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

// tr / tr_emit, lib.rs:359-468: transmittance along a ray that may cross None-material boundaries
// (each crossing switches the current medium); any other surface blocks.  EMIT: the ray is aimed at an
// emitter, so a miss contributes nothing and the first area light met returns its radiance.
template <bool SMALL, bool SPHERES, bool COUNT, bool EMIT>
RENE_DEV f3 transmittance(const SceneView& S, f3 ro, f3 rd, uint32_t medium_index, uint32_t* stack, LaneCounters& lc) {
  f3 tr = splat(1.0f);
  for (int guard = 0; guard < 4096; ++guard) {  // every wave leaves: at most one surface per iteration
    lc.shadow++;
    HitRec h = trace_accel<SMALL, false, SPHERES, COUNT>(S.main, S.spheres, ro, rd, 0.001f, 1e5f, stack, lc);
    if (h.slot == 0xffffffffu) return EMIT ? splat(0.0f) : tr;
    Surface sf = shade_hit<SPHERES>(S, h, ro, rd);
    const Inst& inst = S.insts[sf.instance];
    if (EMIT && inst.emit[3] != 0.0f) {  // area_light.emit(-normalize(rd), payload.normal), lib.rs:447-451
      f3 wo = -normalize(rd);
      return dot(wo, sf.normal) > 0.0f ? tr * mk3(inst.emit[0], inst.emit[1], inst.emit[2]) : splat(0.0f);
    }
    if (inst.material_type != RENE_MATERIAL_NONE) return splat(0.0f);
    MediumRec m = load_medium(S, medium_index);
    if (m.type != RENE_MEDIUM_VACUUM) tr = tr * medium_tr(m, rd, h.t);
    InstMedium im = S.inst_medium[sf.instance];
    medium_index = dot(rd, sf.normal) > 0.0f ? im.exterior : im.interior;
    ro = sf.position;
  }
  return tr;
}

// host side: the launch's seed tables go behind whatever the kernel keeps in LDS (`lds` bytes so far) unless they would
// cost a workgroup per CU (160 KB / workgroups: the traversal stack of a deep tree fills a quarter of it to the brim).  `behind`: bytes the kernel
// keeps behind the tables (the prepared path starts, RENE_START_SLOT), which count towards that and are not added to `lds` here
static inline void seed_tables_place(RenderParams& P, size_t& lds, size_t behind = 0) {
  const size_t cu = 160u * 1024u;
  P.seed_tab = SEED_TAB_NONE;
  if (std::getenv("RENE_NO_LDS_SEEDS")) return;  // (the knob: A/B tests)
  auto groups = [&](size_t b) { return std::min<size_t>(8, cu / b); };  // at most 8 workgroups of 4 waves per CU anyway
  // the form the launch's length asks for (a seed per frame up to 1024 frames: one ds_read per path start) -- or, where those 4 KB would cost a
  // workgroup, the two-level form whatever the length (384 bytes for 1024 frames; three ds_reads, a multiply-add and the output permutation).
  // (Round 4: dragon-class's one launch of 1024 frames sits behind a 36-entry stack + tables = 37.2 KB of a workgroup's 40: the 4 KB table did not
  // fit and every path start composed the generator's jump, ~ 150 integer instructions -- since round 3 made a job one launch.)
  uint32_t shift = seed_tab_shift(P.n_frames);
  size_t bytes = (size_t)seed_tab_words(P.n_frames) * sizeof(uint32_t);
  if (lds != 0 && groups(lds + behind) != groups(lds + behind + bytes) && shift == 0) {
    shift = 5;
    bytes = (size_t)(2u * (1u << shift) + ((P.n_frames + (1u << shift) - 1u) >> shift)) * sizeof(uint32_t);
  }
  const bool fits = !(lds != 0 && groups(lds + behind) != groups(lds + behind + bytes));
  if (std::getenv("RENE_DEBUG")) {
    static size_t last_lds = ~(size_t)0, last_bytes = 0;
    if (last_lds != lds || last_bytes != bytes) std::fprintf(stderr, "[rene] seed tables for %u frames behind %zu bytes of LDS: %s (%zu bytes)\n", P.n_frames, lds, !fits ? "NONE -- every path start composes the generator's jump" : shift ? "two-level" : "one seed per frame", bytes);
    last_lds = lds;
    last_bytes = bytes;
  }
  if (!fits) return;
  P.seed_tab = (uint32_t)(lds / 4u) | (shift << 24);
  lds += bytes;
}

// host side: clamp a persistent launch to the blocks that are co-resident and enable the static first batch
template <typename Kern>
static inline void fit_grid(Kern kernel, size_t lds, const LaunchConfig& cfg, RenderParams& P, dim3& grid) {
  static std::mutex mu;
  static std::unordered_map<uintptr_t, int> cache;
  P.static_waves = 0;
  if (cfg.cus == 0) return;
  const uintptr_t key = reinterpret_cast<uintptr_t>(reinterpret_cast<const void*>(kernel)) ^ (uintptr_t)(lds * 0x9E3779B97F4A7C15ull);
  int occ = 0;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(key);
    if (it != cache.end()) occ = it->second;
    else {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, BLOCK, lds) != hipSuccess) occ = 0;
      cache[key] = occ;
      if (std::getenv("RENE_DEBUG")) std::fprintf(stderr, "[rene] kernel %p lds %zu: %d co-resident blocks per CU\n", reinterpret_cast<const void*>(kernel), lds, occ);
    }
  }
  if (occ < 1) return;
  const uint32_t resident = cfg.cus * (uint32_t)occ;
  if (grid.x > resident) grid.x = resident;
  // a static first batch belongs to one wave: only when every wave of the launch becomes resident at once, which a
  // device shared with another process's launches cannot promise (rene_render always sets DYNAMIC_FIRST)
  if (!(P.flags & RENE_FLAG_DYNAMIC_FIRST)) P.static_waves = grid.x * (BLOCK / 64);
  g_launched_blocks = grid.x;
}

#ifndef RENE_POLL_EVERY
#define RENE_POLL_EVERY 4u  // passes of a wave between two polls of a lane that waits for a hand-off (a power of two)
#endif
#ifndef RENE_BOX_FORM
#define RENE_BOX_FORM 1  // box_slabs.h, BOX_FORM_*: the box item's test in the closest-hit loop of the Matte small-scene kernels (FEAT 64 / 72); 0 = these kernels as they were (A/B in DESIGN.md section 4a)
#endif
#ifndef RENE_SMALL_MATTE_WAVES
#define RENE_SMALL_MATTE_WAVES 1  // min waves per SIMD requested for the Matte small-scene kernel (forcing 6 or 8 spills and loses: 48.6 -> 45.2 / 33.8 Grays/s)
#endif
// Cold kernel arguments.  The RenderParams fields that only the work-item bookkeeping needs (once per pixel and
// launch) are read from the kernarg segment where they are used instead of sitting in SGPRs through the whole
// persistent loop: the kernel is at the SGPR limit and every value parked there is spilled into a VGPR lane and
// brought back with v_readlane -- VALU work in a VALU-bound kernel.  asm volatile keeps the loads where they are
// written (a plain load would be hoisted out of the loop and spilled again).
static_assert(sizeof(SceneView) % 8 == 0, "RenderParams follows SceneView in the kernarg segment at sizeof(SceneView)");
#define RENE_KARG(field) (uint32_t)(sizeof(SceneView) + offsetof(RenderParams, field))
typedef const __attribute__((address_space(4))) void* karg_ptr;  // the kernarg segment (constant address space)
template <uint32_t OFF>
RENE_DEV uint32_t karg_u32(karg_ptr base) {
  uint32_t v;
  asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(base), "n"(OFF));
  return v;
}
template <uint32_t OFF>
RENE_DEV uint64_t karg_u64(karg_ptr base) {
  uint64_t v;
  asm volatile("s_load_dwordx2 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(base), "n"(OFF));
  return v;
}
// Work ids are handed out in wave batches of work_batch ids of ONE level (work_batch divides n_work): batch b is level
// b / level_batches, level-local ids (b % level_batches) * work_batch ... -- decoded once per batch, wave-uniform, so a lane's id is
// its level-local one (a level holds up to 2^31 ids: 16384^2 pixels x CHAINS) and the level count is not bounded by the id width.
// The counter counts batches in 32 bits (the host makes batches long enough that a launch has fewer than 2^31).  A wave keeps its
// batch in two scalars, like the (next, end) of one 32-bit id range before: the next level-local id, and level << 16 | ids left
// (a third one held across the loop cost the bench kernel an occupancy step; decoding b again on every pass that takes ids cost
// it 1.3 % in kernel-argument round trips).
RENE_DEV void batch_take(karg_ptr KB, uint32_t b, uint32_t& batch_next, uint32_t& batch_ll) {
  const uint32_t per = karg_u32<RENE_KARG(level_batches)>(KB), work_batch = karg_u32<RENE_KARG(work_batch)>(KB);
  if ((uint64_t)b >= (uint64_t)karg_u32<RENE_KARG(n_levels)>(KB) * per) {
    batch_ll = 0u;  // past the last level: nothing left
    return;
  }
  // (b < 2^32, levels < 2^11: at most one off, corrected below; the conversion runs on the vector unit, the read-back keeps the rest scalar)
  uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((float)b * __uint_as_float(karg_u32<RENE_KARG(inv_level_batches)>(KB))));
  uint64_t at = (uint64_t)l * per;
  if (at > b) {
    l--;
    at -= per;
  } else if (b - at >= per) {
    l++;
    at += per;
  }
  batch_next = (uint32_t)(b - at) * work_batch;
  batch_ll = (l << 16) | work_batch;
}
// The first batch of every co-resident wave is assigned statically (wave w owns batch w):
// ~5000 waves starting together would otherwise queue up on one atomic counter (measured: 0.4 ms per
// launch, independent of the launch's size).  Later batches come from the counter, which counts batches
// beyond the static region.  The host guarantees static_waves <= the co-resident wave count.
RENE_DEV void first_batch(const RenderParams& P, karg_ptr KB, uint32_t& batch_next, uint32_t& batch_ll) {
  uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)));
  if (wave < P.static_waves) batch_take(KB, wave, batch_next, batch_ll);
}
// The next batch from the launch's counter (one atomic from lane 0); false: none left.  Wave-uniform.
RENE_DEV bool batch_refill(karg_ptr KB, uint32_t& batch_next, uint32_t& batch_ll) {
  uint32_t b = 0;
  if (lane_id() == 0) b = atomicAdd(reinterpret_cast<uint32_t*>(karg_u64<RENE_KARG(work_counter)>(KB)), 1u);
  batch_take(KB, (uint32_t)__builtin_amdgcn_readfirstlane((int)b) + karg_u32<RENE_KARG(static_waves)>(KB), batch_next, batch_ll);
  return (batch_ll & 0xffffu) != 0u;
}

// The engine clock during the launch: wave 0 of workgroup 0 notes the shader clock (s_memtime: ticks of the core clock) and the
// constant 100 MHz clock (s_memrealtime) when it starts -- in memory, not in four SGPRs held across the persistent loop -- and adds
// both differences to counters[24], [25] when it ends: rene_get_stats turns them into MHz (bench.py reports `sclk_mhz` with its
// roofline, whose peak is priced at the nominal 2.4 GHz).
RENE_DEV void clock_probe(const RenderParams& P, bool end) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long t = __builtin_amdgcn_s_memtime(), r = __builtin_amdgcn_s_memrealtime();
  if (!end) {
    P.counters[26] = t;
    P.counters[27] = r;
  } else {
    atomicAdd(&P.counters[24], t - P.counters[26]);
    atomicAdd(&P.counters[25], r - P.counters[27]);
  }
}

// RENE_DEBUG: when a wave started and ended (host-side timeline of a launch)
RENE_DEV void wave_stamp(karg_ptr KB, uint32_t which) {
  unsigned long long* t = reinterpret_cast<unsigned long long*>(karg_u64<RENE_KARG(wave_times)>(KB));
  if (t != nullptr && lane_id() == 0) t[2u * (blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)) + which] = __builtin_amdgcn_s_memrealtime();
}

// 12-byte accesses (the traversal-restart kernels' records, item_flag_publish below)
typedef float v3f __attribute__((ext_vector_type(3)));
RENE_DEV f3 fb_load_rgb(const float* p) {
  v3f v;
  asm volatile("global_load_dwordx3 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return mk3(v.x, v.y, v.z);
}
RENE_DEV void fb_store_rgb(float* p, f3 a) {
  v3f v = {a.x, a.y, a.z};
  asm volatile("global_store_dwordx3 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}
RENE_DEV void fb_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// A lane that waits for the item its own continues from notes when it began (the constant 100 MHz clock, in units of
// 2.56 us) and DROPS its item after eight seconds: the predecessor's waves can have been parked by the driver behind this
// launch's own (a queue eviction while the process's memory map changes restores the queues in its own order), and then
// only this launch leaving the device lets them back in.  The host launches the launch again (rene_hip.cpp, drain).
// (An earlier bound counted polls: 2^22 of them are four seconds for an idle wave.)
RENE_DEV int wait_start() { return (int)(uint32_t)(__builtin_amdgcn_s_memrealtime() >> 8); }
RENE_DEV bool wait_timed_out(int start) {
  constexpr uint32_t kLimit = 8u * 390625u;  // 8 s in units of 256 ticks of 10 ns (a launch lasts a fraction of a second; a wait that is cut
                                             // short costs a replay of the launch, not the image)
  return (uint32_t)(__builtin_amdgcn_s_memrealtime() >> 8) - (uint32_t)start > kLimit;
}
// ... and once one lane has given up (counters[8] != 0, until the host's next rene_reset), every other waiting lane of this
// and of the following launches gives up at its next poll: the image is lost anyway, and the context must come back to the
// host with its error (RENE_ERR_DEVICE at the next drain) within seconds, not after every pixel's chain has timed out in turn
RENE_DEV uint32_t flag_load(const uint32_t* p);
RENE_DEV bool wait_abandoned(const RenderParams& P) {
  return flag_load(reinterpret_cast<const uint32_t*>(P.counters + 8)) != 0u;
}
// counters[8]: lanes that gave up; [9..11]: what the first of them waited for (pixel and chain x | y << 14 | chain << 28; launch epoch << 32 | version
// seen; version wanted) for the host's error message
RENE_DEV void wait_report(const RenderParams& P, karg_ptr KB, uint32_t pxy, uint32_t ver, uint32_t seen);

// A lane identifies its work item by `ver`, the version the item will leave on its pixel's records: epoch << VERSION_LEVEL_BITS |
// (level + 1); 0 = the lane has no item.  (Until round 3 it kept the work id -- level * n_work + pixel slot -- and every commit,
// every load and every poll divided it by n_work again behind three scalar loads of cold kernel arguments: a work-item switch was
// ~175 instructions of the whole wave, a fourteenth of the Cornell kernel's instruction count at sixteen items per pixel.)
// The item of level l > 0 continues from the item of level l - 1 of the same launch and waits until the pixel's records
// carry (epoch << VERSION_LEVEL_BITS | l) = ver - 1; a level-0 item continues from the context's previous launch and waits for the
// version that launch left behind (prev_final; 0 = a zeroed image; launches are serial: it is there).  The sums are taken
// from the very load that showed the version, so a pixel's frames are added in the same order however the items are cut
// (bit-identical images).
RENE_DEV uint32_t item_version_want(karg_ptr KB, uint32_t ver) {
  return (ver & MAX_LEVELS) == 1u ? karg_u32<RENE_KARG(prev_final)>(KB) : ver - 1u;
}
// Which frames of the launch an item of `level` renders: n_uniform items of level_step frames, then what is left in
// halving items (rest R: level n_uniform + l starts at R - ceil(R / 2^l) of it, the last one takes what remains) -- the end of
// a launch is then a handful of frames of its slowest pixels.  (Halving from the start was measured and lost: the item a
// pixel continues from is handed out one sweep of the image earlier, and a sweep of items half as long leaves half the
// slack -- every pixel a third more expensive than the average then waits; DESIGN.md section 4f.)
RENE_DEV void item_frames(karg_ptr KB, uint32_t level, uint32_t& frame, uint32_t& frame_end) {
  const uint32_t step = karg_u32<RENE_KARG(level_step)>(KB), n_uniform = karg_u32<RENE_KARG(n_uniform)>(KB);
  if (level < n_uniform) {
    frame = level * step;
    frame_end = frame + step;
  } else {
    const uint32_t n_frames = karg_u32<RENE_KARG(group_frames)>(KB), n_levels = karg_u32<RENE_KARG(n_levels)>(KB);  // (the frames of ONE chain: RenderParams.group_frames)
    const uint32_t l = level - n_uniform, rest = n_frames - n_uniform * step;
    frame = n_frames - ((rest + (1u << l) - 1u) >> l);
    frame_end = level + 1u >= n_levels ? n_frames : n_frames - ((rest + (2u << l) - 1u) >> (l + 1u));
  }
}
// What turning a work id into (pixel, frames, version) reads, fetched together: four scalar loads behind ONE wait (one load
// and its wait per argument were nine scalar-cache round trips the wave stood behind at every item switch, a quarter of the
// Cornell kernel's passes)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
struct ItemArgs {
  uint32_t n_work, shard_rank, shard_count, tiles_x, epoch, level_step, n_uniform;
  float inv_level_batches, inv_tiles_x;
  uint64_t active_tiles;  // RenderParams::active_tiles (0: every tile is active)
};
static_assert(offsetof(RenderParams, shard_rank) == offsetof(RenderParams, n_work) + 4 && offsetof(RenderParams, shard_count) == offsetof(RenderParams, n_work) + 8 &&
              offsetof(RenderParams, tiles_x) == offsetof(RenderParams, n_work) + 12 && offsetof(RenderParams, n_uniform) == offsetof(RenderParams, level_step) + 4 &&
              offsetof(RenderParams, inv_tiles_x) == offsetof(RenderParams, inv_level_batches) + 4, "item_args loads these together");
RENE_DEV ItemArgs item_args(karg_ptr KB) {
  u32x4 a;
  u32x2 b, c;
  uint32_t e;
  uint64_t m;  // (the mask's address rides behind the same wait: the default path pays no round trip of its own for it)
  asm volatile("s_load_dwordx4 %0, %5, %6\n\ts_load_dwordx2 %1, %5, %7\n\ts_load_dwordx2 %2, %5, %8\n\ts_load_dword %3, %5, %9\n\ts_load_dwordx2 %4, %5, %10\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(e), "=&s"(m)
               : "s"(KB), "n"(RENE_KARG(n_work)), "n"(RENE_KARG(level_step)), "n"(RENE_KARG(inv_level_batches)), "n"(RENE_KARG(epoch)), "n"(RENE_KARG(active_tiles)));
  return ItemArgs{a.x, a.y, a.z, a.w, e, b.x, b.y, __uint_as_float(c.x), __uint_as_float(c.y), m};
}
// Adaptive sampling (RenderParams::active_tiles): is owned tile k switched off for this launch?  Asked where a lane takes an item, and only under a
// mask: one cached vector load of the word that holds bit k.  The item of an inactive tile is made EMPTY (frame = frame_end) and goes through the
// version protocol like any other: it waits for its predecessor, loads and commits the same sums -- prev_final, replays and the epoch wrap see no
// per-tile case, and no bit of the sums changes.
RENE_DEV bool tile_inactive(const ItemArgs& IA, uint32_t k) {
  if (IA.active_tiles == 0ull) return false;
  const uint32_t* m = reinterpret_cast<const uint32_t*>(IA.active_tiles);
  return ((m[k >> 5] >> (k & 31u)) & 1u) == 0u;
}
// Where a pixel's records are (device_scene.h, pixel slots): record index chain * 3 * n_slots + slot of the chain's first layer (the
// layers follow n_slots records apart); the version word of the traversal-restart kernels is chain * n_slots + slot.  x and yi (the
// image row, top first) lie in a tile the context owns; its owned-tile index (t - shard_rank) / shard_count is exact, so a float
// reciprocal rounded to the nearest integer finds it (t < 2^18).  Taken where a record is touched -- a commit, a load, a poll --
// not kept: a lane holds its pixel as coordinates.  (The Matte small-scene kernels keep the slot as well: item_switch below.)
RENE_DEV uint32_t pixel_slot(karg_ptr KB, uint32_t x, uint32_t yi, uint32_t& n_slots) {
  u32x4 a;
  uint32_t inv;
  asm volatile("s_load_dwordx4 %0, %2, %3\n\ts_load_dword %1, %2, %4\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(a), "=&s"(inv)
               : "s"(KB), "n"(RENE_KARG(n_work)), "n"(RENE_KARG(inv_shard_count)));
  n_slots = a.x >> CHAINS_LOG2;
  return pixel_slot_of(x, yi, a.w, a.y, __uint_as_float(inv));  // (item_slot.h)
}
RENE_DEV size_t pixel_record(karg_ptr KB, uint32_t x, uint32_t yi, uint32_t chain) {
  uint32_t n_slots;
  const uint32_t slot = pixel_slot(KB, x, yi, n_slots);
  return (size_t)(chain * 3u) * n_slots + slot;
}
RENE_DEV void item_frames(karg_ptr KB, const ItemArgs& IA, uint32_t level, uint32_t& frame, uint32_t& frame_end) {
  if (level < IA.n_uniform) {
    frame = level * IA.level_step;
    frame_end = frame + IA.level_step;
  } else {
    item_frames(KB, level, frame, frame_end);
  }
}
// Frame chains (device_scene.h, CHAINS): item_frames cuts [0, group_frames) -- the frames ANY chain may have in this launch -- into levels;
// chain `chain` owns the launch's frames first, first + CHAINS, ... (first = (chain - chain_phase) mod CHAINS), `count` of them: turns the
// item's range of chain-local numbers into launch frame numbers, clipped to the chain's own count (a chain one frame short of the longest
// one has a shorter -- possibly empty -- last item; an empty item commits what it loaded).  The caller steps `frame` by CHAINS.
RENE_DEV void chain_frames(karg_ptr KB, uint32_t chain, uint32_t& frame, uint32_t& frame_end) {
  const uint32_t n = karg_u32<RENE_KARG(n_frames)>(KB), phase = karg_u32<RENE_KARG(chain_phase)>(KB);
  const uint32_t first = (chain - phase) & (CHAINS - 1u);
  const uint32_t count = first < n ? (n - first + CHAINS - 1u) >> CHAINS_LOG2 : 0u;
  frame = first + ((frame < count ? frame : count) << CHAINS_LOG2);
  frame_end = first + ((frame_end < count ? frame_end : count) << CHAINS_LOG2);
}
RENE_DEV void wait_report(const RenderParams& P, karg_ptr KB, uint32_t pxy, uint32_t ver, uint32_t seen) {
  if (atomicAdd(&P.counters[8], 1ull) == 0ull) {
    P.counters[9] = pxy;
    P.counters[10] = ((unsigned long long)karg_u32<RENE_KARG(epoch)>(KB) << 32) | seen;
    P.counters[11] = item_version_want(KB, ver);
  }
}
// fault injection (RENE_TEST_DROP): which items of the launch behave as if their hand-off had timed out -- one pixel in 97
RENE_DEV bool item_test_drop(uint32_t pxy) { return ((pxy * 2654435761u) >> 7) % 97u == 5u; }
template <bool AOV>
RENE_DEV void item_commit(uint32_t ver, float* p, size_t layer_stride, f3 acc0, f3 acc1, f3 acc2) {
  if (AOV) {
    fb_store(p + layer_stride, acc1, ver);
    fb_store(p + 2 * layer_stride, acc2, ver);
  }
  fb_store(p, acc0, ver);
}
// What a pixel's version says to an item: ITEM_WAIT -- its predecessor has not committed yet; ITEM_READY -- the records carry
// the version the item continues from; ITEM_DONE -- this item (or a later one of the pixel) has been committed already: a
// launch that is being REPLAYED (rene_hip.cpp, drain: a launch some of whose items were dropped is launched again, alone)
// skips it, which is what makes a launch restartable.  Versions are epoch << VERSION_LEVEL_BITS | items committed in that launch.
enum : uint32_t { ITEM_WAIT = 0, ITEM_READY = 1, ITEM_DONE = 2 };
RENE_DEV uint32_t item_state(uint32_t seen, uint32_t want, uint32_t done) {
  if (seen == want) return ITEM_READY;
  const uint32_t es = seen >> VERSION_LEVEL_BITS, ed = done >> VERSION_LEVEL_BITS;
  return (es == ed ? (seen & MAX_LEVELS) >= (done & MAX_LEVELS) : es > ed) ? ITEM_DONE : ITEM_WAIT;
}
// loads the pixel's records into acc*; ITEM_READY when they carry the version the item continues from (until then the
// sums are not the item's yet: the caller keeps waiting and loads again)
template <bool AOV>
RENE_DEV uint32_t item_load(karg_ptr KB, uint32_t ver, const float* p, size_t layer_stride, f3& acc0, f3& acc1, f3& acc2) {
  const uint32_t want = item_version_want(KB, ver), done = ver;
  v4f a;
  bool ok = true;
  if (AOV) {
    v4f b, c;
    fb_load3(p, p + layer_stride, p + 2 * layer_stride, a, b, c);
    acc1 = mk3(b.x, b.y, b.z);
    acc2 = mk3(c.x, c.y, c.z);
    ok = __float_as_uint(b.w) == want && __float_as_uint(c.w) == want;
  } else {
    fb_load1(p, a);
  }
  acc0 = mk3(a.x, a.y, a.z);
  // (record 0 is the last one an item stores: its version decides what has been committed)
  const uint32_t st = item_state(__float_as_uint(a.w), want, done);
  return st == ITEM_READY && !ok ? (uint32_t)ITEM_WAIT : st;
}

// The traversal-restart kernels (render_wf.inc) have no registers to spare in their logic step for 16-byte tuples:
// they keep the versions in a separate array, P.item_done[pixel slot], and 12-byte records -- Guideline 16's
// flag-then-payload form: payload stored sc0 sc1 and drained (s_waitcnt vmcnt(0)), then the flag; the consumer polls the
// flag and then reads the sums, all four kinds of access with sc0 sc1.  Same version numbers, same order of
// additions; a context uses one kernel family, so the two forms never meet on one image.
// The flag accesses are system-scope ("sc0 sc1") like the records': an agent-scope atomic load (sc1 only) is served by the
// polling XCD's own L2, and a line that L2 fetched BEFORE the producer on another XCD stored its version stays there --
// stale -- for as long as polling keeps it hot.  Seen at full size with launches of one to three frames (most lanes
// waiting, little other traffic to evict the line): every lane whose first poll came too early waited until the safety
// net; with longer launches the same staleness only cost time.  sc0 sc1 loads bypass the L2 as well.
RENE_DEV uint32_t flag_load(const uint32_t* p) {
  uint32_t v;
  asm volatile("global_load_dword %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}
RENE_DEV void flag_store(uint32_t* p, uint32_t v) {
  asm volatile("global_store_dword %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}
// (the flag of a pixel sits at its linear index in the image, like its records)
RENE_DEV void item_flag_publish(karg_ptr KB, uint32_t ver, uint32_t pixel) {
  fb_drain();  // the sc1 stores have reached memory before the flag can be seen
  flag_store(reinterpret_cast<uint32_t*>(karg_u64<RENE_KARG(item_done)>(KB)) + pixel, ver);
}
RENE_DEV uint32_t item_flag_state(karg_ptr KB, uint32_t ver, uint32_t pixel) {  // ITEM_WAIT / ITEM_READY / ITEM_DONE
  return item_state(flag_load(reinterpret_cast<const uint32_t*>(karg_u64<RENE_KARG(item_done)>(KB)) + pixel), item_version_want(KB, ver), ver);
}

// SceneView is the first kernel argument (kernarg offset 0).  The traversal-restart kernels read the shading tables
// only in their logic step; fetched there through karg_u64 they are short-lived scalars instead of twenty SGPRs that
// live through the whole state machine and get spilled into VGPR lanes (v_readlane / v_writelane around every use).
#define RENE_SKARG(field) (uint32_t)offsetof(SceneView, field)
// The loads are NOT volatile: a pointer the instantiation never reads is not loaded (as volatile asm all eleven were, each a
// scalar-cache round trip the wave stood behind: Matte-only kernels read two of them).  `tick` -- the persistent loop's pass
// counter, an input the load does not use -- keeps the others inside the loop (a loop-invariant load would be hoisted and parked).
template <uint32_t OFF>
RENE_DEV uint64_t karg_u64_at(karg_ptr base, uint32_t tick) {
  uint64_t v;
  asm("s_load_dwordx2 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(base), "n"(OFF), "s"(tick));
  return v;
}
// (a pointer that comes out of an asm load is a generic one to the compiler, and what it reads through it are FLAT loads -- which
// count on both wait counters and go through the aperture check: 317 of them in the Substrate kernel; cast through the global
// address space it is what the kernel-argument pointers are)
template <typename T>
RENE_DEV const T* global_ptr(uint64_t v) {
  return (const T*)(const __attribute__((address_space(1))) T*)v;
}
RENE_DEV SceneView logic_view(karg_ptr KB, const SceneView& S, uint32_t tick) {
  SceneView V = S;
  V.shade = global_ptr<PrimShade>(karg_u64_at<RENE_SKARG(shade)>(KB, tick));
  V.emit_pdf = global_ptr<EmitPdf>(karg_u64_at<RENE_SKARG(emit_pdf)>(KB, tick));
  V.insts = global_ptr<Inst>(karg_u64_at<RENE_SKARG(insts)>(KB, tick));
  V.emit_objects = global_ptr<EmitObject>(karg_u64_at<RENE_SKARG(emit_objects)>(KB, tick));
  V.emit_tris = global_ptr<EmitTri>(karg_u64_at<RENE_SKARG(emit_tris)>(KB, tick));
  V.materials = global_ptr<Material>(karg_u64_at<RENE_SKARG(materials)>(KB, tick));
  V.textures = global_ptr<Texture>(karg_u64_at<RENE_SKARG(textures)>(KB, tick));
  V.lights = global_ptr<Light>(karg_u64_at<RENE_SKARG(lights)>(KB, tick));
  V.images = global_ptr<ImageRef>(karg_u64_at<RENE_SKARG(images)>(KB, tick));
  V.image_pool = global_ptr<float>(karg_u64_at<RENE_SKARG(image_pool)>(KB, tick));
  V.uni = global_ptr<struct Uniforms>(karg_u64_at<RENE_SKARG(uni)>(KB, tick));
  return V;
}

// ---- the frame-wide sample stream from the launch's table (device_scene.h, FRAME_STREAM_*) -------------------------------------------------
// the instantiations that read it: the Matte small-scene kernels (FEAT_SMALL and FEAT_LIGHTS | FEAT_SMALL).  Anywhere else the stream's position
// depends on the hit material (general BSDFs) or the draws come in another order (volpath).
constexpr bool frame_stream_feat(uint32_t feat) { return (feat & FEAT_SMALL) && !(feat & (FEAT_VOLPATH | FEAT_SPHERES)) && lobe_kinds(feat) == 0; }
// ---- the emitter query, answered by the next bounce's closest-hit loop (DESIGN.md section 4a) ----------------------------------------------------
// A surviving bounce ends with the emitter query of the new ray (Q5: the emitter-only structure, for pdf_l), and the next pass traces the same
// ray, tmin and tmax against the main structure.  Where the emitter structure is ONE triangle / parallelogram item and the main list holds the
// same record (scene_pack.cpp marks it: SMALL_ITEM_EMIT_TWIN; Cornell's light), the second loop answers both: the bounce stops after f |cos|,
// keeps the BSDF half of the pdf, and the lane finishes it -- pdf, the 1e-5 kill, is_zero, the roulette of the depth it left -- behind the next
// closest-hit loop, in the order the bounce had, before that loop's hit means anything.  In these Matte-only kernels every lane that is on a path
// at depth > 0 left its last bounce through that branch (see Q3 below), so `depth > 0` is the deferred mark.  A lane whose throughput
// is exactly zero after f |cos| does not defer: it ends at the bounce, as before (argument there) -- deferring it too cost a quarter of the job, a
// third of Cornell's bounces holding their slots through one more loop (profiles/emit_fusion_ab.txt).
constexpr bool emit_fusion_feat(uint32_t feat) { return frame_stream_feat(feat); }  // the kernels that read the table: Cornell's
// the same kernels' bounce without the work its result does not need (TRIM_* above); TRIM_STATIC_MATTE wants a kernel without textures
constexpr uint32_t bounce_trims(uint32_t feat) { return frame_stream_feat(feat) && !(feat & FEAT_TEXTURES) ? (uint32_t)(RENE_BOUNCE_TRIMS) & 0xfu : 0u; }
// ---- the work-item switch of the same kernels (DESIGN.md section 4, profiles/item_switch_ab.txt) --------------------------------------------------------
// A lane that takes an item has its slot in a register -- the work id without the chain bits -- and the reference form throws it away, keeps (x, y)
// and builds the slot again from them (pixel_slot: a float reciprocal, five masked shifts, five kernel arguments behind a wait) at the commit, at the
// first poll and at every re-poll.
//   ITEM_KEEP_SLOT    the lane keeps the slot in a VGPR beside pxy; a record is chain * 3 * n_slots + slot, n_slots from layer_stride
// What it rests on -- pixel_slot(decode(slot)) == slot -- is item_slot.h's, checked on the host (selftest/item_slot_check.cpp,
// tests/test_item_slot.py).  The mask a kernel gets is item_switch(FEAT): 0 everywhere but in FEAT 64 / 72.  (Bit 2, the tile of a wave's batch
// decoded once per take on the scalar unit, was measured and taken out: 15 VALU instructions fewer per take and no time gained.)
#ifndef RENE_ITEM_SWITCH
#define RENE_ITEM_SWITCH 1u  // -DRENE_ITEM_SWITCH=0: these kernels as they were (A/B builds: make variant)
#endif
enum : uint32_t { ITEM_KEEP_SLOT = 1u };
constexpr uint32_t item_switch(uint32_t feat) { return frame_stream_feat(feat) && !(feat & FEAT_TEXTURES) ? (uint32_t)(RENE_ITEM_SWITCH) & 1u : 0u; }
// ---- the path start of the same kernels, prepared ahead (DESIGN.md section 4, profiles/start_slot_ab.txt) ---------------------------------------------
// A lane's next primary ray is a function of (pixel, frame) and of nothing its path computes, and a masked wave64 instruction costs what a full one
// does: the start block, run on every pass for the third of the lanes whose path has just ended, is issued mostly for lanes that are off.  Each
// lane keeps ONE prepared start in LDS -- START_SLOT_DWORDS planes of BLOCK dwords behind the scene's image and the seed tables
// (RenderParams::start_slot): the direction and the pixel generator's state behind its two draws; origin, throughput, depth and medium are constants
// -- and bit 31 of pxy says that it is there.  The start block runs only in a pass where a lane needs a path and has none prepared, and then for
// EVERY lane of the wave that holds an item with a frame left and an empty slot, whatever that lane is doing: on a path, waiting for its sums,
// about to start.  A lane fills only its own slot, with the start's own operations in their order (the bits are the same), and no lane waits.
// Taking an item overwrites pxy and with it the bit, and that is the only way to an item: no start outlives the item it was prepared for.
#ifndef RENE_START_SLOT
#define RENE_START_SLOT 1u  // -DRENE_START_SLOT=0: these kernels as they were (A/B builds: make variant)
#endif
constexpr uint32_t START_SLOT_DWORDS = 4u, START_SLOT_FULL = 0x80000000u;
constexpr bool start_slot(uint32_t feat) { return frame_stream_feat(feat) && !(feat & FEAT_TEXTURES) && ((uint32_t)(RENE_START_SLOT) & 1u) != 0u; }
constexpr size_t start_slot_bytes(uint32_t feat) { return start_slot(feat) ? (size_t)START_SLOT_DWORDS * BLOCK * sizeof(uint32_t) : 0u; }
// entry [launch frame][depth]: one 16-byte GLOBAL load (global_load_dwordx4 off a scalar base with a 32-bit lane offset -- the table of the longest
// launch, MAX_LAUNCH_FRAMES rows of 1 KB, is 64 MB).  A gather: the lanes of a wave are at different frames and depths.
RENE_DEV float4 frame_stream_load(const float* table, uint32_t launch_frame, uint32_t depth) {
  const uint32_t off = ((launch_frame << FRAME_STREAM_STRIDE_LOG2) + depth) << 4;
  const lds_v4 e = *(const __attribute__((address_space(1))) lds_v4*)((const __attribute__((address_space(1))) char*)table + off);
  return make_float4(e.x, e.y, e.z, e.w);
}
// what one thread of the fill kernel does for one frame: the integrator's draws in the integrator's order, through the same functions
// (lib.rs:274-324, 345-354) -- coin, then emitter object / primitive / barycentrics if it says light, then the roulette number if depth > 12
template <bool SPHERES>
RENE_DEV void frame_stream_row(const SceneView& S, uint32_t seed, float4* row) {
  Pcg fw = pcg_new(seed);
  for (uint32_t depth = 0; depth < FRAME_STREAM_DEPTHS; ++depth) {
    f3 on_light = splat(0.0f);
    uint32_t light = 0u;
    if (S.emit_object_len > 0) {
      if (pcg_f32(fw) > 0.5f) {
        uint32_t obj = umod(pcg_u32(fw), S.emit_object_len);
        on_light = emit_sample<SPHERES>(S, obj, fw);
        light = 0x80000000u;
      }
    }
    float rr_coin = 0.0f;
    if (depth > 12) rr_coin = pcg_f32(fw);
    row[depth] = make_float4(on_light.x, on_light.y, on_light.z, __uint_as_float(__float_as_uint(rr_coin) | light));
  }
}

template <uint32_t FEAT, int MAXL, bool COUNT, bool AOV>
#ifndef RENE_SMALL_GEN1_PLAIN_WAVES
#define RENE_SMALL_GEN1_PLAIN_WAVES 1  // ... for its instantiation without textures / lights / background (135 VGPRs: 3 waves)
#endif
#ifndef RENE_SMALL_GEN1_WAVES
#define RENE_SMALL_GEN1_WAVES 1  // min waves per SIMD requested for the general single-lobe small-scene kernel (155 VGPRs: 3 waves)
#endif
__global__ void __launch_bounds__(BLOCK, (FEAT & FEAT_SMALL) && !(FEAT & FEAT_VOLPATH) ? (!(FEAT & FEAT_GENERAL_BSDF) ? RENE_SMALL_MATTE_WAVES : (MAXL == 1 ? ((FEAT & FEAT_TEXTURES) ? RENE_SMALL_GEN1_WAVES : RENE_SMALL_GEN1_PLAIN_WAVES) : 1)) : 1) render_kernel(SceneView S, RenderParams P) {
  constexpr bool SPHERES = (FEAT & FEAT_SPHERES) != 0;
  constexpr uint32_t GENERAL = lobe_kinds(FEAT);  // 0: Matte only
  constexpr bool SMALL = (FEAT & FEAT_SMALL) != 0;
  constexpr bool VOL = (FEAT & FEAT_VOLPATH) != 0;
  extern __shared__ uint32_t s_stack[];  // [stack depth][BLOCK]; small scenes: the LDS image of their tables instead
  uint32_t* stack = s_stack + threadIdx.x;
  // small scenes (path integrator): hit shading, emitter sampling and the emitter pdf read LDS-resident tables
  constexpr bool LDS = SMALL && !VOL;
  constexpr bool FWTAB = frame_stream_feat(FEAT);  // the frame-wide stream comes from the launch's table: no `fw` generator in the lane
  constexpr bool EFUSE = emit_fusion_feat(FEAT);   // a marked scene's emitter query is answered by the next closest-hit loop (above)
  constexpr int BOXF = EFUSE ? RENE_BOX_FORM : BOX_FORM_PLAIN;  // the same kernels' closest-hit loop tests a box item in this form (box_slabs.h)
  constexpr uint32_t TRIM = bounce_trims(FEAT);    // ... and their bounce leaves these out (TRIM_*)
  constexpr bool SHARED_RD = (TRIM & TRIM_SHARED_RD) != 0u;
  constexpr bool KEEP_SLOT = (item_switch(FEAT) & ITEM_KEEP_SLOT) != 0u;  // the work-item switch (above)
  constexpr bool SLOT = start_slot(FEAT);  // the path start prepared ahead (above): bit 31 of pxy is the lane's "a start is prepared"
  SmallLds T{};
  if constexpr (LDS) {
    small_lds_fill(S, s_stack);
    T = small_lds(S, s_stack);
  }
  seed_tables_fill(P, s_stack);  // behind the image / the traversal stack
  __syncthreads();

  LaneCounters lc;
  const uint32_t W = S.width, H = S.height;
  const float tmin = 0.001f, tmax = 100000.0f;  // lib.rs:182-183

  // work-item state: one item = (pixel, frame range).  A launch of F frames cuts every pixel into n_levels
  // items of level_step frames; all items of one level are handed out before any of the next, so a lane's last
  // item -- the end of the launch -- costs one step of one pixel, and the item a pixel continues from was handed
  // out a whole level earlier.  An item continues the running sums its predecessor committed (same summation
  // order as one lane doing all F frames), found through the version its records carry (fb_store / item_load
  // above); a pixel's first item likewise continues from the previous launch.
  // pxy: launch_id.x | launch_id.y << 14 | chain << 28 (one register: the general variants live at the edge of an occupancy step)
  uint32_t ver = 0, pxy = 0, frame = 0, frame_end = 0;  // ver: the lane's work item (item_version_want above); 0 = none
  const karg_ptr KB = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr();  // cold arguments are re-read where they are used (karg_u32)
  // the item's records: chain g's are the g-th [3][n_slots][4] block of the framebuffer, at the pixel's slot (device_scene.h, CHAINS, pixel slots)
  [[maybe_unused]] uint32_t slot = 0;  // KEEP_SLOT: the item's pixel slot, owned tile << 10 | place in the tile -- what pixel_slot() makes of pxy
  const size_t layer_stride = (size_t)(P.n_work >> CHAINS_LOG2) * 4;  // n_slots records
  auto item_pxy = [&]() -> uint32_t { return SLOT ? pxy & ~START_SLOT_FULL : pxy; };  // pxy as the item wrote it
  auto rec_offset = [&]() -> size_t {
    if constexpr (KEEP_SLOT) return (size_t)((item_pxy() >> 28) * 3u) * layer_stride + (size_t)slot * 4;
    else return pixel_record(KB, pxy & 0x3fffu, H - 1 - ((pxy >> 14) & 0x3fffu), item_pxy() >> 28) * 4;
  };
  bool waiting = false;
  f3 acc0 = splat(0.0f), acc1 = splat(0.0f), acc2 = splat(0.0f);
  // path state
  bool active = false, done = false;
  f3 ro = splat(0.0f), rd = splat(0.0f), color = splat(0.0f);
  Pcg rng{0}, fw{0};
  int depth = 0;
  uint32_t medium_index = 0;  // volpath: the medium the ray is travelling in (0 = vacuum)
  [[maybe_unused]] float pdf_bsdf = 0.0f;  // EFUSE: the BSDF half of the pdf of a bounce whose emitter query is still to be answered

  // wave-uniform batch of work ids: the next level-local id, and its level << 16 | ids left (batch_take)
  uint32_t batch_next = 0, batch_ll = 0;
  bool exhausted = false;
  first_batch(P, KB, batch_next, batch_ll);
  clock_probe(P, false);

  uint32_t iter = 0;  // wave-uniform: a lane that waits for a hand-off polls on every RENE_POLL_EVERY-th pass, not on each
  uint32_t ln_active = 0, ln_wait = 0, ln_idle = 0, ln_start = 0, st_switch = 0, st_poll = 0;  // COUNT: where the lanes of a pass are
  [[maybe_unused]] uint32_t st_refill = 0, ln_refill = 0;  // COUNT, SLOT: passes that ran the start block, and the lanes it ran for
  for (;; ++iter) {
    // ---- item bookkeeping --------------------------------------------------------------------------
    bool finished = !active && !waiting && ver != 0u && frame == frame_end;
    if (finished) {
      float* p = reinterpret_cast<float*>(karg_u64<RENE_KARG(framebuffer)>(KB)) + rec_offset();  // add_image target, lib.rs:166
      item_commit<AOV>(ver, p, layer_stride, acc0, acc1, acc2);
      ver = 0u;
    }
    if (COUNT && __any(finished)) st_switch++;
    bool need = !done && ver == 0u;
    bool fresh = false;  // took its item in this pass
    if (__any(need)) {
      if ((batch_ll & 0xffffu) == 0u && !exhausted) exhausted = !batch_refill(KB, batch_next, batch_ll);  // wave-uniform: one global atomic
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
        const uint32_t chain = w & (CHAINS - 1u);  // a level's ids: pixel slot * CHAINS + chain (a wave's 64 ids: eight pixels, every chain of each)
        w >>= CHAINS_LOG2;
        // item -> pixel: owned 32x32 tiles, 8x8 micro-tiles inside (a wave starts on one micro-tile)
        const uint32_t k = w >> 10, r = w & 1023u;
        const uint32_t tile = IA.shard_rank + k * IA.shard_count;
        uint32_t tx;
        const uint32_t ty = udiv_small(tile, IA.tiles_x, IA.inv_tiles_x, tx);
        const uint32_t x = slot_x(tx, r), yi = slot_yi(ty, r);  // yi: the image row, top first (item_slot.h)
        if (x < W && yi < H) {
          if constexpr (KEEP_SLOT) slot = w;
          ver = (IA.epoch << VERSION_LEVEL_BITS) | (level + 1u);
          pxy = x | ((H - 1 - yi) << 14) | (chain << 28);  // launch_id.x, launch_id.y (resolutions are at most MAX_RESOLUTION, checked at rene_create)
          item_frames(KB, IA, level, frame, frame_end);
          chain_frames(KB, chain, frame, frame_end);
          if (tile_inactive(IA, k)) frame = frame_end;  // a tile switched off: the empty item
          waiting = true;  // sums are loaded below (an item first waits for the one it continues from)
          fresh = true;
          depth = wait_start();  // a lane that waits has no path: its depth register holds when the wait began
        }
      }
    }
    // A poll is a round trip to memory that bypasses the caches, and the whole wave stands behind it: the lane polls when it
    // has just taken the item (nearly always there: its predecessor was handed out a sweep of the image earlier) and then on
    // every RENE_POLL_EVERY-th pass of the wave (measured: DESIGN.md section 4f)
    if (COUNT) {
      if (waiting) ln_wait++;
      else if (active) ln_active++;
      else if (ver == 0u) ln_idle++;
      else ln_start++;
      if (__any(waiting && (fresh || (iter & (RENE_POLL_EVERY - 1u)) == 0u))) st_poll++;
    }
    if (waiting && (fresh || (iter & (RENE_POLL_EVERY - 1u)) == 0u)) {
      const float* p = reinterpret_cast<const float*>(karg_u64<RENE_KARG(framebuffer)>(KB)) + rec_offset();
      // safety net so that every wave can leave: the awaited item always makes progress unless the driver has parked the
      // waves that render it behind this launch's own (seen: DESIGN.md section 4g)
      const uint32_t st = item_load<AOV>(KB, ver, p, layer_stride, acc0, acc1, acc2);
      const bool drop = (P.flags & RENE_FLAG_INTERNAL_TEST_DROP) && item_test_drop(item_pxy()) && st != ITEM_DONE;  // fault injection (tests)
      if (st == ITEM_READY && !drop) {
        waiting = false;
      } else if (st == ITEM_DONE) {  // a replayed launch: this item was committed the first time round
        ver = 0u;
        waiting = false;
      } else if (drop || wait_timed_out(depth) || ((iter & 63u) == 0u && wait_abandoned(P))) {
        // the item is DROPPED, not rendered on top of sums that are not its own: the host finds counters[8] != 0 at its next
        // sync and launches the launch again, alone, where nothing can be in its way; what has been committed is skipped
        wait_report(P, KB, item_pxy(), ver, 0u);
        ver = 0u;
        waiting = false;
      } else if (!__any(active)) {
        // a wave with nothing else to do polls slowly: the item it waits for is being rendered by a wave that needs
        // the issue slots
        __builtin_amdgcn_s_sleep(16);
      }
    }
    if (__all(done)) break;

    // ---- ray generation, lib.rs:174-189 -----------------------------------------------------------
    // (the path start runs on every pass: waiting until 8 / 16 / 24 lanes want one lost, profiles/r04_experiments.txt section 2)
    if constexpr (SLOT) {
      // the start block runs where a lane needs a start it has not got, and then for every lane that has a frame left and none prepared
      const bool start = !active && !waiting && ver != 0u && frame < frame_end;
      if (__any(start && !(pxy & START_SLOT_FULL))) {
        const bool fill = !(pxy & START_SLOT_FULL) && ver != 0u && frame < frame_end;  // (on a path, waiting or starting: pixel and frame are the item's)
        if (COUNT) {
          st_refill++;
          if (fill) ln_refill++;
        }
        if (fill) {
          const uint32_t seed = launch_seed(P, s_stack, frame);  // the frame it prepares FOR: `frame` moves at the start below
          const uint32_t px = pxy & 0x3fffu, py = (pxy >> 14) & 0x3fffu;
          Pcg prng = pcg_new((py * W + px) ^ seed);
          float u = qdiv((float)px + pcg_f32(prng), (float)(W - 1));  // Q2
          float v = qdiv((float)py + pcg_f32(prng), (float)(H - 1));
          cfloat_ptr cam = (cfloat_ptr)(const void*)S.uni;  // c2w[16], proj_inv[16]
          f3 origin = camera_origin(cam);
          f3 target = m4_point(cam + 16, mk3(u * 2.0f - 1.0f, v * 2.0f - 1.0f, 1.0f));  // camera.rs:77-90
          target = m4_point(cam, target);
          const f3 prd = normalize(target - origin);
          start_slot_store(s_stack, P.start_slot, prd, prng.state);
          pxy |= START_SLOT_FULL;
        }
      }
      if (start) {  // its slot is full: filled just now or in an earlier pass
        uint32_t state;
        start_slot_load(s_stack, P.start_slot, rd, state);
        rng.state = state;
        pxy &= ~START_SLOT_FULL;
        frame += CHAINS;  // the chain's next frame
        ro = camera_origin((cfloat_ptr)(const void*)S.uni);
        color = splat(1.0f);
        depth = 0;
        medium_index = 0;  // lib.rs:529
        active = true;
      }
    } else
    if (!active && !waiting && ver != 0u && frame < frame_end) {
      const uint32_t seed = launch_seed(P, s_stack, frame);
      frame += CHAINS;  // the chain's next frame
      const uint32_t px = pxy & 0x3fffu, py = (pxy >> 14) & 0x3fffu;
      rng = pcg_new((py * W + px) ^ seed);
      if constexpr (!FWTAB) fw = pcg_new(seed);
      float u = qdiv((float)px + pcg_f32(rng), (float)(W - 1));  // Q2
      float v = qdiv((float)py + pcg_f32(rng), (float)(H - 1));
      cfloat_ptr cam = (cfloat_ptr)(const void*)S.uni;  // c2w[16], proj_inv[16]
      f3 origin = camera_origin(cam);
      f3 target = m4_point(cam + 16, mk3(u * 2.0f - 1.0f, v * 2.0f - 1.0f, 1.0f));  // camera.rs:77-90
      target = m4_point(cam, target);
      ro = origin;
      rd = normalize(target - origin);
      color = splat(1.0f);
      depth = 0;
      medium_index = 0;  // lib.rs:529
      active = true;
    }

    // ---- one bounce, lib.rs:192-355 ------------------------------------------------------------------
    if (active) {
      if constexpr (!EFUSE) lc.closest++;
      // the frame-wide stream's entry for this bounce (`frame` already names the chain's next frame), loaded behind the query: before it the
      // latency hides behind the item loop at the price of four VGPRs live across it, and that lost (DESIGN.md section 4a)
      float4 fwe = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      HitRec h;
      [[maybe_unused]] EmitCapture cap;
      [[maybe_unused]] f3 nrd = splat(0.0f);  // SHARED_RD: normalize(rd) of this pass's ray
      if constexpr (EFUSE) {
        h = traverse_small<false, SPHERES, COUNT, LDS, true, BOXF>(S.main, S.spheres, ro, rd, tmin, tmax, lc, T.items_main, &cap);
        if constexpr (SHARED_RD) nrd = normalize(rd);  // once, where both of its users see it: the deferred emitter pdf here, wo in the hit branch
        if (cap.seen != 0u && depth > 0) {  // the rest of the bounce this lane left (the hit branch below, from Q5 on; `depth` is already that bounce's + 1)
          const HitRec eh = emit_twin_hit(T, cap, tmax);
          const float pdf_l = emitter_pdf_lds<SPHERES, SHARED_RD>(S, T, eh, ro, SHARED_RD ? nrd : rd);
          float pdf = pdf_bsdf;
          bool alive = true;
          pdf = 0.5f * pdf + qdiv(0.5f * pdf_l, (float)S.emit_object_len);
          if (pdf < 1e-5f) alive = false;
          else color = color / pdf;
          if (alive && is_zero(color)) alive = false;
          if (alive && depth - 1 > 12) {
            const float rr_coin = fabsf(frame_stream_load(P.frame_stream, frame - CHAINS, (uint32_t)(depth - 1)).w);
            float continue_p = max_element(color);
            if (rr_coin > continue_p) alive = false;
            else color = color / continue_p;
          }
          // a lane that ends here has traced a ray its path never had: it counts nothing and adds nothing
          if (COUNT && !alive) lc.prims -= S.main.n_items;
          active = alive;
        }
        if (active) lc.closest++;
      } else {
        h = trace_accel<SMALL, false, SPHERES, COUNT, LDS>(S.main, S.spheres, ro, rd, tmin, tmax, stack, lc, T.items_main);
      }
      if (EFUSE && !active) {  // ended behind the loop, above
      } else if (h.slot == 0xffffffffu) {  // main_miss, lib.rs:120-139, 209-211
        f3 bg = splat(0.0f);
        if (FEAT & FEAT_BACKGROUND) {
          uv2 uv = sphere_uv(normalize(m4_vector(S.uni->bg_matrix, rd)));
          bg = mk3(S.uni->bg_color[0], S.uni->bg_color[1], S.uni->bg_color[2]) * background_tex<FEAT>(S, uv);
        }
        acc0 = acc0 + color * bg;
        lc.adds++;
        active = false;
      } else if (VOL) {  // main_ray_generation_volpath, lib.rs:552-801
        lc.hits++;
        Surface sf = shade_hit<SPHERES>(S, h, ro, rd);
        const Inst& inst = S.insts[sf.instance];
        f3 wo = -normalize(rd);
        f3 normal = normalize(sf.normal);
        f3 position = sf.position;
        MediumRec medium = load_medium(S, medium_index);
        bool scattered = false;
        if (medium.type != RENE_MEDIUM_VACUUM) {  // lib.rs:563-565
          SampledMedium sm = medium_sample(medium, ro, rd, h.t, rng);
          color = color * sm.tr;
          scattered = sm.sampled;
          if (scattered) ro = sm.position;
        }
        bool alive = true;
        if (scattered) {  // a scattering event inside the medium, lib.rs:567-656
          if (FEAT & FEAT_LIGHTS) {
            for (uint32_t li = 0; li < S.lights_len; ++li) {
              float4 ld = ldg4(S.lights[li].dir), lL = ldg4(S.lights[li].L);
              f3 wi = normalize((ro + mk3(ld.x, ld.y, ld.z)) - ro);
              f3 tr = transmittance<SMALL, SPHERES, COUNT, false>(S, ro, wi, medium_index, stack, lc);
              acc0 = acc0 + color * tr * medium_phase(medium, wo, wi) * mk3(lL.x, lL.y, lL.z);
              lc.adds++;
            }
          }
          if (S.emit_object_len > 0) {  // emitter sample drawn from the PIXEL stream here, lib.rs:599-654
            uint32_t obj = umod(pcg_u32(rng), S.emit_object_len);
            f3 wi = normalize(emit_sample<SPHERES>(S, obj, rng) - ro);
            lc.emitter++;
            HitRec eh = trace_accel<SMALL, false, SPHERES, COUNT>(S.emit, S.spheres, ro, wi, tmin, tmax, stack, lc);
            float pdf_l = emitter_pdf<SPHERES>(S, eh, ro, wi);
            f3 tr = transmittance<SMALL, SPHERES, COUNT, true>(S, ro, wi, medium_index, stack, lc);
            float pdf = qdiv(pdf_l, (float)S.emit_object_len);
            if (pdf > 1e-5f) {
              acc0 = acc0 + color * tr * medium_phase(medium, wo, wi) / pdf;
              lc.adds++;
            }
          }
          rd = medium_sample_p(medium, wo, rng);  // lib.rs:656
        } else {  // the surface, lib.rs:657-780
          Bsdf<MAXL> bsdf;
          bsdf.len = 0;
          bsdf.codes = 0xffffffffu;
          bsdf.ng = normal;
          bsdf.onb = onb_from_w(normal);
          compute_bsdf<FEAT, MAXL>(S, inst, sf.uv, bsdf);
          if (inst.emit[3] != 0.0f) {
            f3 e = dot(wo, normal) > 0.0f ? mk3(inst.emit[0], inst.emit[1], inst.emit[2]) : splat(0.0f);
            acc0 = acc0 + color * e;
            lc.adds++;
          }
          if (depth == 0) {
            if (AOV) {
              acc1 = acc1 + normal;
              acc2 = acc2 + material_albedo<FEAT>(S, inst, sf.uv);
            }
            lc.adds += 2;
          }
          if (inst.material_type != RENE_MATERIAL_NONE) {
            if (FEAT & FEAT_LIGHTS) {  // lib.rs:671-701: f, then the transmittance walk
              for (uint32_t li = 0; li < S.lights_len; ++li) {
                float4 ld = ldg4(S.lights[li].dir), lL = ldg4(S.lights[li].L);
                f3 wi = normalize((position + mk3(ld.x, ld.y, ld.z)) - position);
                f3 f = bsdf_f<MAXL, GENERAL>(bsdf, wo, wi);
                f3 tr = transmittance<SMALL, SPHERES, COUNT, false>(S, position, wi, medium_index, stack, lc);
                acc0 = acc0 + color * tr * f * fabsf(dot(wi, normal)) * mk3(lL.x, lL.y, lL.z);
                lc.adds++;
              }
            }
            if (S.emit_object_len > 0 && bsdf_contains<MAXL, GENERAL>(bsdf, K_DIFFUSE)) {  // lib.rs:703-754
              f3 wi, f;
              float pdf;
              if (pcg_f32(fw) > 0.5f) {
                uint32_t obj = umod(pcg_u32(fw), S.emit_object_len);
                wi = normalize(emit_sample<SPHERES>(S, obj, fw) - position);
                pdf = bsdf_pdf<MAXL, GENERAL>(bsdf, wi, normal);
                f = bsdf_f<MAXL, GENERAL>(bsdf, wo, wi);
              } else {
                Sampled s = bsdf_sample<MAXL, GENERAL>(bsdf, wo, rng);
                wi = s.wi;
                pdf = s.pdf;
                f = s.f;
              }
              ro = position;
              rd = wi;
              lc.emitter++;
              HitRec eh = trace_accel<SMALL, false, SPHERES, COUNT>(S.emit, S.spheres, ro, rd, tmin, tmax, stack, lc);
              float pdf_l = emitter_pdf<SPHERES>(S, eh, ro, rd);
              color = color * (f * fabsf(dot(normal, wi)));
              pdf = 0.5f * pdf + qdiv(0.5f * pdf_l, (float)S.emit_object_len);
              if (pdf < 1e-5f) alive = false;
              else color = color / pdf;
            } else {  // lib.rs:755-767
              Sampled s = bsdf_sample<MAXL, GENERAL>(bsdf, wo, rng);
              if (s.pdf < 1e-5f) {
                alive = false;
              } else {
                color = color * (s.f * qdiv(fabsf(dot(normal, s.wi)), s.pdf));
                ro = position;
                rd = s.wi;
              }
            }
          } else {  // a medium boundary: straight through, lib.rs:768-773
            ro = position;
          }
          InstMedium im = S.inst_medium[sf.instance];
          medium_index = dot(wo, normal) < 0.0f ? im.exterior : im.interior;  // lib.rs:775-779
        }
        if (alive && is_zero(color)) alive = false;  // lib.rs:783-785; the roulette is commented out upstream
        depth++;
        if (depth >= 80) alive = false;  // MAX_DEPTH, lib.rs:499
        active = alive;
      } else {
        lc.hits++;
        if constexpr (FWTAB) fwe = frame_stream_load(P.frame_stream, frame - CHAINS, (uint32_t)depth);
        // general-BSDF variants fetch the shading tables here (logic_view) instead of parking their pointers in SGPRs
        // across the whole loop: the kernel is at the SGPR limit, and what is spilled there comes back through
        // v_readlane; the Matte variants read so few tables that they stay where they are
        const SceneView L = GENERAL ? logic_view(KB, S, iter) : S;
        Inst inst_lds;
        Surface sf;
        if constexpr (LDS) sf = shade_hit_lds<SPHERES>(L, T, h, ro, rd, inst_lds);
        else sf = shade_hit<SPHERES>(L, h, ro, rd);
        const Inst& inst = LDS ? inst_lds : L.insts[sf.instance];
        f3 wo = SHARED_RD ? -nrd : -normalize(rd);
        f3 normal = normalize(sf.normal);
        f3 position = sf.position;
        Bsdf<MAXL> bsdf;
        bsdf.len = 0;
        bsdf.codes = 0xffffffffu;
        bsdf.ng = normal;
        bsdf.onb = (TRIM & TRIM_ONB_SELECT) ? onb_from_w_select(normal) : onb_from_w(normal);
        compute_bsdf<FEAT, MAXL, TRIM>(L, inst, sf.uv, bsdf);

        if (inst.emit[3] != 0.0f) {  // lib.rs:225-227, area_light.rs:66-74
          f3 e = dot(wo, normal) > 0.0f ? mk3(inst.emit[0], inst.emit[1], inst.emit[2]) : splat(0.0f);
          acc0 = acc0 + color * e;
          lc.adds++;
        }
        if (depth == 0) {  // lib.rs:229-232
          if (AOV) {
            acc1 = acc1 + normal;
            acc2 = acc2 + material_albedo<FEAT, TRIM>(L, inst, sf.uv);
          }
          lc.adds += 2;
        }
        if (FEAT & FEAT_LIGHTS) {  // lib.rs:234-272
          for (uint32_t li = 0; li < L.lights_len; ++li) {
            float4 ld = ldg4(L.lights[li].dir), lL = ldg4(L.lights[li].L);
            f3 target = position + mk3(ld.x, ld.y, ld.z);  // light.rs:52-55
            f3 wi = normalize(target - position);
            lc.shadow++;
            HitRec sh = trace_accel<SMALL, true, SPHERES, COUNT, LDS>(S.main, S.spheres, position, wi, tmin, 1e5f, stack, lc, T.items_main);
            if (sh.slot == 0xffffffffu) {
              f3 f = bsdf_f<MAXL, GENERAL, TRIM>(bsdf, wo, wi);
              acc0 = acc0 + color * f * fabsf(dot(wi, normal)) * mk3(lL.x, lL.y, lL.z);
              lc.adds++;
            }
          }
        }
        bool alive = true;
        // behind bsdf_contains a static Matte BSDF holds its one lobe: b.len == 1 is a constant there (bsdf_f above)
        constexpr uint32_t TRIM1 = (TRIM & TRIM_STATIC_MATTE) ? TRIM | TRIM_UNIT_LEN : TRIM;
        [[maybe_unused]] bool deferred = false;  // EFUSE: the bounce's pdf, is_zero and roulette are still to come
        if (L.emit_object_len > 0 && bsdf_contains<MAXL, GENERAL>(bsdf, K_DIFFUSE)) {  // lib.rs:274-324
          f3 wi, f;
          float pdf;
          // Q3: frame-wide stream.  FWTAB: the table holds the stream as a path draws it that reaches every depth through THIS branch (and, with
          // no emitter in the scene, through neither: wave-uniform, the table then holds roulette numbers only).  The only other way past this
          // point in a Matte-only kernel is b.len == 0, where bsdf_sample below returns sampled_default(), pdf 0, and the path ends at
          // `s.pdf < 1e-5f`: no live lane is ever at a stream position other than the table's.
          bool pick_light;
          if constexpr (FWTAB) pick_light = (__float_as_uint(fwe.w) >> 31) != 0u;
          else pick_light = pcg_f32(fw) > 0.5f;
          if (pick_light) {
            f3 on_light;
            if constexpr (FWTAB) {
              on_light = mk3(fwe.x, fwe.y, fwe.z);
            } else {
              uint32_t obj = umod(pcg_u32(fw), L.emit_object_len);
              if constexpr (LDS) on_light = emit_sample_lds<SPHERES>(T, obj, fw);
              else on_light = emit_sample<SPHERES>(L, obj, fw);
            }
            wi = normalize(on_light - position);
            pdf = bsdf_pdf<MAXL, GENERAL, TRIM1>(bsdf, wi, normal);  // Q1: (wi, normal), lib.rs:287
            f = bsdf_f<MAXL, GENERAL, TRIM1>(bsdf, wo, wi);
          } else {
            Sampled s = bsdf_sample<MAXL, GENERAL, TRIM1>(bsdf, wo, rng);
            wi = s.wi;
            pdf = s.pdf;
            f = s.f;
          }
          ro = position;
          rd = wi;
          lc.emitter++;
          if (EFUSE && cap.seen != 0u) {  // wave-uniform: Q5 and what follows it wait for the next closest-hit loop (above)
            if (COUNT) lc.prims++;  // the emitter item, tested there as the main list's twin
            color = color * (f * fabsf(dot(normal, wi)));
            pdf_bsdf = pdf;
            deferred = true;
            // A throughput of exactly zero ends the path whatever the emitter query finds, unless the pdf is NaN (pdf < 1e-5: ended; else
            // 0 * rcp(pdf) = 0 for every pdf up to + inf, and is_zero ends it) -- so such a lane ends HERE, as it always did, instead of
            // holding its slot through one more item loop (a third of Cornell's bounces end this way: the black light, light samples below
            // the surface).  The pdf is 0.5 pdf_bsdf + 0.5 pdf_l / n.  Zero products mean f |normal . wi| is finite, so wi = rd is finite
            // and, being normalised, not zero; with ro finite as well (checked, like pdf_bsdf) pdf_l is 0 for a miss or, for a hit at
            // t in [tmin, tmax], a finite positive squared distance times rcp of a finite non-negative cosine * area: never NaN.
            if (is_zero(color) && pdf == pdf && length_squared(ro) < __builtin_inff()) alive = false;
          } else {
            HitRec eh = trace_accel<SMALL, false, SPHERES, COUNT, LDS>(S.emit, S.spheres, ro, rd, tmin, tmax, stack, lc, T.items_emit);  // Q5
            float pdf_l;
            if constexpr (LDS) pdf_l = emitter_pdf_lds<SPHERES>(L, T, eh, ro, rd);  // (the NEW ray: its own normalize)
            else pdf_l = emitter_pdf<SPHERES>(L, eh, ro, rd);
            color = color * (f * fabsf(dot(normal, wi)));
            pdf = 0.5f * pdf + qdiv(0.5f * pdf_l, (float)L.emit_object_len);
            if (pdf < 1e-5f) alive = false;
            else color = color / pdf;
          }
        } else {  // lib.rs:325-337
          Sampled s = bsdf_sample<MAXL, GENERAL, TRIM>(bsdf, wo, rng);
          if (s.pdf < 1e-5f) {
            alive = false;
          } else {
            color = color * (s.f * qdiv(fabsf(dot(normal, s.wi)), s.pdf));
            ro = position;
            rd = s.wi;
          }
        }
        if (!(EFUSE && deferred)) {
          if (alive && is_zero(color)) alive = false;  // lib.rs:340-342
          if (alive && depth > 12) {                   // lib.rs:345-354
            float rr_coin;
            if constexpr (FWTAB) rr_coin = fabsf(fwe.w);
            else rr_coin = pcg_f32(fw);
            float continue_p = max_element(color);
            if (rr_coin > continue_p) alive = false;
            else color = color / continue_p;
          }
        }
        depth++;
        if (depth >= 50) alive = false;  // lib.rs:192 (Q7)
        active = alive;
      }
    }
  }

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
  if (COUNT) {  // where the lanes of a pass were (rene_get_stats prints them under RENE_DEBUG; counters[23] marks this kernel family)
    unsigned long long a = wave_sum(ln_active), b = wave_sum(ln_wait), c = wave_sum(ln_idle), d = wave_sum(ln_start);
    if (lane_id() == 0) {
      atomicAdd(&P.counters[12], (unsigned long long)iter);
      atomicAdd(&P.counters[13], a);
      atomicAdd(&P.counters[14], b);
      atomicAdd(&P.counters[15], c);
      atomicAdd(&P.counters[16], d);
      atomicAdd(&P.counters[17], (unsigned long long)st_switch);
      atomicAdd(&P.counters[18], (unsigned long long)st_poll);
      atomicAdd(&P.counters[23], 1ull);
    }
    if constexpr (SLOT) {  // passes that ran the start block, and the lanes it ran for
      const unsigned long long e = wave_sum(ln_refill);
      if (lane_id() == 0) {
        atomicAdd(&P.counters[19], (unsigned long long)st_refill);
        atomicAdd(&P.counters[20], e);
      }
    }
  }
}


#include "render_wf.inc"

// host side: the instantiation of a choice (kernel_select.h) among those of the leaf FEAT (five lobes for a multi-lobe leaf, else one), or null; then
// among those of a unit's leaves, each of which the unit names once.  What a leaf instantiates: the path integrator's item loop three forms of
// render_kernel, every other leaf two (none for FEAT_NO_EMITTERS); a BVH leaf its restart kernels as well, outside volpath also the one with the
// tables in LDS.  A choice the leaf does not have is null -- an error for the launcher, never another kernel.  (Kept below every kernel of this
// file: the resource report in <unit>.res cites kernels by line.)
template <uint32_t FEAT>
static inline RenderKernel render_leaf(const KernelChoice& k) {
  constexpr int MAXL = (FEAT & FEAT_MULTI_LOBE) ? 5 : 1;
  constexpr bool SMALL = (FEAT & FEAT_SMALL) != 0, VOL = (FEAT & FEAT_VOLPATH) != 0;
  if (k.feat != FEAT || k.maxl != MAXL || (k.count && !k.aov) || (k.tables && (VOL || k.count)) || k.reads_frame_stream != frame_stream_feat(FEAT)) return nullptr;
  if constexpr (!SMALL) {
    if (k.family == KernelFamily::Restart) {
      if constexpr (!VOL) if (k.tables) return render_kernel_wf<FEAT, MAXL, false, true, true>;
      return k.count ? render_kernel_wf<FEAT, MAXL, true, true, false> : (k.aov ? render_kernel_wf<FEAT, MAXL, false, true, false> : render_kernel_wf<FEAT, MAXL, false, false, false>);
    }
  }
  if (k.tables || k.family != (SMALL ? KernelFamily::ItemLoop : KernelFamily::WhileWhile)) return nullptr;
  if constexpr (SMALL && !VOL) if (!k.count && k.aov) return render_kernel<FEAT, MAXL, false, true>;
  if constexpr (!(FEAT & FEAT_NO_EMITTERS)) if (k.count == k.aov) return k.aov ? render_kernel<FEAT, MAXL, true, true> : render_kernel<FEAT, MAXL, false, false>;
  return nullptr;
}
template <uint32_t... FEAT>
static inline RenderKernel find_leaf(const KernelChoice& k) {
  RenderKernel r = nullptr;
  (..., (r = r ? r : render_leaf<FEAT>(k)));
  return r;
}
