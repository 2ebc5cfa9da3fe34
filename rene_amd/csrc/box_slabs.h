// box_slabs.h -- the SMALL_KIND_BOX item test of the small-scene item loop (device_code.inc, traverse_small; device_scene.h, SmallItem):
// a parallelepiped as three slab pairs in its own coordinates.  Along axis x of the box the point o + t d has the coordinate
// c0 + t c1 with c0 = o . x' + w, c1 = d . x' (q[4 ax .. 4 ax + 3] = x', w); the faces are at 0 and 1.  Two forms of the slab evaluation
// that give the same bits and share one accept tail; selftest/box_slabs_probe.hip runs one against the other on the device.  The kernels use
// the vector form: with the matrix form the bench job was 3.3 % slower than without either (profiles/box_mfma_ab.txt).
// Plain floats only: no other header of the project is needed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rene {

#define RENE_BOX_DEV __device__ __forceinline__

// which form a caller of traverse_small asks for (template argument BOX)
constexpr int BOX_FORM_PLAIN = 0;  // the test as every kernel had it before this header existed: left as it is, instruction for instruction
constexpr int BOX_FORM_VALU = 1;   // box_slabs_valu + box_accept

constexpr uint32_t BOX_KIND_BITS = 0x40400000u;  // SMALL_KIND_BOX = 3.0f as the packer writes it into q[12]

struct BoxSlabs {
  float t_in, t_out;        // entry and exit parameter of the line through the three slab pairs
  float t0, t1;             // the third axis' two faces (coordinate 0 and 1): the open face is one of them
  float c0[3], c1[3];       // the dot products (read by the probe only; dead in the kernels)
};

// the three axes, given their dot products.  The first axis starts the running entry / exit instead of going through max(-inf, .) and
// min(+inf, .): fminf / fmaxf return the other operand for a NaN one, so the two differ only where an axis has BOTH parameters NaN -- with the
// infinite start that axis drops out, without it the NaN is carried to the next axis' fmaxf / fminf, which drops it just the same.  The end
// result differs only if all three axes are NaN on both sides, i.e. c0 = c1 = 0 on every axis (or a NaN ray): c1 = 0 on three independent
// axes means d = 0, which a normalised direction excludes.
RENE_BOX_DEV void box_axes(BoxSlabs& s) {
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float inv = __builtin_amdgcn_rcpf(s.c1[ax]);
    s.t0 = -s.c0[ax] * inv;
    s.t1 = s.t0 + inv;
    const float lo = fminf(s.t0, s.t1), hi = fmaxf(s.t0, s.t1);
    s.t_in = ax == 0 ? lo : fmaxf(s.t_in, lo);
    s.t_out = ax == 0 ? hi : fminf(s.t_out, hi);
  }
}

// the dot products on the vector pipe: q = the item's record, wave-uniform (SGPR operands)
template <class Q>
RENE_BOX_DEV BoxSlabs box_slabs_valu(const Q& q, float ox, float oy, float oz, float dx, float dy, float dz) {
  BoxSlabs s;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    s.c0[ax] = fmaf(ox, q[4 * ax], fmaf(oy, q[4 * ax + 1], fmaf(oz, q[4 * ax + 2], q[4 * ax + 3])));
    s.c1[ax] = fmaf(dx, q[4 * ax], fmaf(dy, q[4 * ax + 1], dz * q[4 * ax + 2]));
  }
  box_axes(s);
  return s;
}

// The dot products on the matrix pipe: v_mfma_f32_4x4x1_16b_f32 updates sixteen 4 x 4 blocks by a rank-1 product, D[i][j] = A[i] B[j] + C[i][j].
// Lane l supplies A for row l & 3 of its block of four lanes and B for column l & 3, and receives the four rows of its own column: with
// A = a coefficient of plane (l & 3) and B = the lane's own ray component every lane gets its ray against the box's three planes (row 3, the
// record's q[12..15], is spare: whatever comes out of it is never read).  The result is bit for bit the k-ordered fmaf chain, one rounding
// per product, so c0 is four chained instructions (w . 1, then z, y, x) and c1 three; both start on C = -0 (x y + -0 = x y with its sign, where
// + 0 would turn a product of -0 into + 0 and with it the sign of 1 / c1 for a ray parallel to the slab).
//   EXEC: a matrix instruction executes for every lane whatever EXEC says, and a lane's rows come from the A operands of the three other
//   lanes of its block -- a disabled neighbour whose `a` was never loaded corrupts live lanes.  The caller therefore runs this with every
//   lane enabled (wave-uniform control flow only); a lane without a ray computes garbage into its own column only.
//   Denormals: under -fgpu-flush-denormals-to-zero the vector pipe flushes a subnormal result or operand to zero and the matrix pipe's C / D do
//   not.  That shows only for a subnormal INTERMEDIATE of the chains: a cancellation to below 1.2e-38 of terms whose own spacing is many
//   orders larger (the coordinates are of order one, their ulp 1e-7).  The probe's rays and the byte-identical layers of the bench job were the check.
//   Registers: the accumulators are VGPRs only in a kernel that asks for two waves per SIMD or more (__launch_bounds__(n, 2)); with a budget of 512
//   registers the compiler puts them into AGPRs and reads every result back with a v_accvgpr_read.
typedef float box_v4 __attribute__((ext_vector_type(4)));
RENE_BOX_DEV BoxSlabs box_slabs_matrix(const __attribute__((address_space(3))) float* item, uint32_t lane, float ox, float oy, float oz, float dx,
                                       float dy, float dz) {
  const box_v4 a = *(const __attribute__((address_space(3))) box_v4*)(item + 4u * (lane & 3u));  // plane (lane & 3): x', w -- one ds_read_b128
  const box_v4 z = {-0.0f, -0.0f, -0.0f, -0.0f};
  // c1 first and consumed (its reciprocals) before c0 is needed: the two chains can share four registers
  box_v4 c1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.z, dz, z, 0, 0, 0);
  c1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.y, dy, c1, 0, 0, 0);
  c1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.x, dx, c1, 0, 0, 0);
  box_v4 c0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.w, 1.0f, z, 0, 0, 0);
  c0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.z, oz, c0, 0, 0, 0);
  c0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.y, oy, c0, 0, 0, 0);
  c0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.x, ox, c0, 0, 0, 0);
  BoxSlabs s;
  s.c0[0] = c0.x; s.c0[1] = c0.y; s.c0[2] = c0.z;
  s.c1[0] = c1.x; s.c1[1] = c1.y; s.c1[2] = c1.z;
  box_axes(s);
  return s;
}

// The tail both forms share.  A line meets a convex box in its entry and its exit face; the closest with t >= tmin is the hit.  A box may have
// one open face, on its third axis (open_face, wave-uniform: 1 = the face at coordinate 0, 2 = at 1): the ray passes through it.  A closed
// box -- a scalar branch -- needs none of that.  Which face was hit, and where on it, is read off the hit point after the loop, once, for the
// winner.
RENE_BOX_DEV bool box_accept_open(const BoxSlabs& s, float t_open, float tmin, float best_t, float& t) {
  const bool use_in = s.t_in >= tmin && s.t_in != t_open;
  const bool dead = !use_in && s.t_out == t_open;
  t = use_in ? s.t_in : s.t_out;
  return s.t_in <= s.t_out && !dead && t >= tmin && t < best_t;
}
RENE_BOX_DEV bool box_accept(const BoxSlabs& s, uint32_t open_face, float tmin, float best_t, float& t) {
  if (open_face == 0u) {
    t = s.t_in >= tmin ? s.t_in : s.t_out;
    return s.t_in <= s.t_out && t >= tmin && t < best_t;
  }
  if (open_face == 1u) return box_accept_open(s, s.t0, tmin, best_t, t);
  return box_accept_open(s, s.t1, tmin, best_t, t);
}

}  // namespace rene
