// onb_probe.hip -- the two forms of the shading frame (../device_math.h: onb_from_w with its divergent branch, onb_from_w_select without it)
// against each other on the device it runs on, under the kernels' own flags, and the two facts the static Matte BSDF of the small-scene
// kernels rests on (../device_code.inc, TRIM_UNIT_LEN: p instead of p * rcp(1)).
//
//   onb_probe        no arguments
//
// One workgroup.  Normals: a few thousand random unit vectors, then the crafted ones -- |x| == |y| in every sign combination (the tie of the
// frame's test), (0, 0, +-1), the axis normals, +-0 components, a denormal component, NaN and inf lanes, the zero vector.  Two runs: every lane
// with a normal; and an irregular half of the lanes without one, both forms inside the divergent branch of the live lanes.  u and v are compared
// bit for bit (a NaN equals itself only with the same payload).
// Then v_rcp_f32(1.0f), the 1.0f read from memory so that the instruction runs; and p against p * rcp(1) through the consumers the bounce has
// for a pdf, 0.5 * p + q and p < 1e-5, for p zero, denormal, around 1e-5 and normal, of either sign, and NaN / inf.
// Prints "frame COMPARED MISMATCHED" per run, "rcp1 BITS" and "pdf COMPARED MISMATCHED", a line for the first mismatch of each; exits 0 iff
// nothing mismatched and rcp(1) is 0x3f800000.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../device_math.h"

using namespace rene;

constexpr uint32_t PROBE_BLOCK = 256;

#define CHECK(x)                                              \
  do {                                                        \
    hipError_t e_ = (x);                                      \
    if (e_ != hipSuccess) {                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
      return 2;                                               \
    }                                                         \
  } while (0)

// out[0] = comparisons, out[1] = mismatches, out[2..] = the first mismatch: normal, field, the two values' bits
__global__ void __launch_bounds__(PROBE_BLOCK) frame_kernel(const float* normals, uint32_t n, uint32_t half, uint32_t* out) {
  uint32_t compared = 0;
  for (uint32_t j0 = 0; j0 < n; j0 += PROBE_BLOCK) {  // n is a multiple of the block: every lane makes every pass
    const uint32_t j = j0 + threadIdx.x;
    const bool live = !half || (((threadIdx.x * 2654435761u) ^ (j0 * 40503u)) >> 13 & 1u) != 0u;  // the irregular half: a hash of lane and pass
    if (live) {
      const f3 w = mk3(normals[3 * j], normals[3 * j + 1], normals[3 * j + 2]);
      const Onb a = onb_from_w(w), b = onb_from_w_select(w);
      const uint32_t want[6] = {__float_as_uint(a.u.x), __float_as_uint(a.u.y), __float_as_uint(a.u.z),
                                __float_as_uint(a.v.x), __float_as_uint(a.v.y), __float_as_uint(a.v.z)};
      const uint32_t got[6] = {__float_as_uint(b.u.x), __float_as_uint(b.u.y), __float_as_uint(b.u.z),
                               __float_as_uint(b.v.x), __float_as_uint(b.v.y), __float_as_uint(b.v.z)};
      for (uint32_t f = 0; f < 6u; ++f) {
        compared++;
        if (got[f] != want[f] && atomicAdd(&out[1], 1u) == 0u) {
          out[2] = j; out[3] = f; out[4] = got[f]; out[5] = want[f];
        }
      }
    }
  }
  atomicAdd(&out[0], compared);
}

// one lane per (p, q): out[0] comparisons, out[1] mismatches, out[2..] the first; out[7] = the bits of v_rcp_f32(*one)
__global__ void __launch_bounds__(PROBE_BLOCK) pdf_kernel(const float* one, const float* p, uint32_t n_p, const float* q, uint32_t n_q, uint32_t* out) {
  const float r = fast_rcp(*one);  // what qdiv(p, (float)b.len) multiplies by when b.len == 1
  if (threadIdx.x == 0) out[7] = __float_as_uint(r);
  uint32_t compared = 0;
  for (uint32_t i = threadIdx.x; i < n_p * n_q; i += PROBE_BLOCK) {
    const float a = p[i / n_q], b = q[i % n_q];
    const float m = a * r;  // the multiply the static BSDF leaves out
    const uint32_t want[2] = {__float_as_uint(0.5f * m + b), m < 1e-5f ? 1u : 0u};
    const uint32_t got[2] = {__float_as_uint(0.5f * a + b), a < 1e-5f ? 1u : 0u};
    for (uint32_t f = 0; f < 2u; ++f) {
      compared++;
      if (got[f] != want[f] && atomicAdd(&out[1], 1u) == 0u) {
        out[2] = i / n_q; out[3] = i % n_q; out[4] = f; out[5] = got[f]; out[6] = want[f];
      }
    }
  }
  atomicAdd(&out[0], compared);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static uint64_t g_state = 0x853c49e6748fea9bull;
static uint32_t rnd() {  // PCG-XSH-RR
  const uint64_t old = g_state;
  g_state = old * 6364136223846793005ull + 1442695040888963407ull;
  const uint32_t x = (uint32_t)(((old >> 18u) ^ old) >> 27u), r = (uint32_t)(old >> 59u);
  return (x >> r) | (x << ((32u - r) & 31u));
}
static float uni(float a, float b) { return a + (b - a) * (float)(rnd() >> 8) * (1.0f / 16777216.0f); }
static float bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = bits(0x7fc00000u), den = bits(0x00012345u), s = std::sqrt(0.5f);
  std::vector<float> normals;
  auto push = [&](float x, float y, float z) {
    normals.push_back(x);
    normals.push_back(y);
    normals.push_back(z);
  };
  constexpr uint32_t N_RANDOM = 3584, N_TOTAL = 4096;
  static_assert(N_TOTAL % PROBE_BLOCK == 0, "every lane makes every pass");
  for (uint32_t i = 0; i < N_RANDOM; ++i) {
    float d[3];
    float l;
    do {
      for (float& c : d) c = uni(-1.f, 1.f);
      l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    } while (l < 1e-3f || l > 1.0f);
    push(d[0] / l, d[1] / l, d[2] / l);
  }
  for (int sx = -1; sx <= 1; sx += 2)
    for (int sy = -1; sy <= 1; sy += 2) {
      push(sx * s, sy * s, 0.0f);  // |x| == |y|: the tie, the second form
      push(sx * s, sy * s, -0.0f);
      push(sx * 0.5f, sy * 0.5f, s);
      push(sx * 0.5f, sy * 0.5f, -s);
      push(sx * 0.6f, sy * 0.6f, 0.52915025f);
      push(sx * 0.0f, sy * 0.0f, 1.0f);  // (+-0, +-0, +-1)
      push(sx * 0.0f, sy * 0.0f, -1.0f);
      push(sx * 1.0f, sy * 0.0f, 0.0f);  // the axis normals, +-0 beside them
      push(sx * 0.0f, sy * 1.0f, 0.0f);
      push(sx * 1.0f, 0.0f, sy * 0.0f);
      push(0.0f, sx * 1.0f, sy * 0.0f);
      push(sx * s, sy * 0.0f, s);  // |x| == |z|
      push(sx * 0.0f, sy * s, -s);
      push(sx * den, sy * 1.0f, 0.0f);  // a denormal component: flushed by the compare? by the products?
      push(sx * 1.0f, sy * den, 0.0f);
      push(sx * den, sy * den, 1.0f);
      push(sx * den, 0.0f, sy * den);
      push(0.0f, sx * den, sy * den);
      push(sx * s, sy * s, den);
      push(sx * nan, sy * 0.5f, 0.5f);  // NaN and inf lanes
      push(sx * 0.5f, sy * nan, 0.5f);
      push(sx * 0.5f, sy * 0.25f, nan);
      push(sx * 0.25f, sy * 0.5f, nan);
      push(sx * inf, sy * 0.5f, 0.5f);
      push(sx * 0.5f, sy * inf, 0.5f);
      push(sx * inf, sy * inf, 0.0f);
      push(sx * 0.5f, sy * 0.25f, inf);
      push(sx * 0.25f, sy * 0.5f, -inf);
      push(sx * nan, sy * nan, nan);
      push(sx * 0.0f, sy * 0.0f, 0.0f);  // the zero vector: rcp(sqrt(0)) = inf, 0 * inf
    }
  const uint32_t n_crafted = (uint32_t)(normals.size() / 3u) - N_RANDOM;
  if (N_RANDOM + n_crafted > N_TOTAL) {
    fprintf(stderr, "too many crafted normals\n");
    return 2;
  }
  for (uint32_t i = 0; N_RANDOM + n_crafted + i < N_TOTAL; ++i) {  // the crafted ones again, at other lanes
    const uint32_t k = 3u * (N_RANDOM + i % n_crafted);
    push(normals[k], normals[k + 1], normals[k + 2]);
  }

  // the pdfs: zero, denormal, the smallest normal, around the 1e-5 cut, ordinary, of either sign; inf and NaN
  std::vector<float> p = {0.0f,          -0.0f,         bits(0x00000001u), bits(0x80000001u), den,     -den,   bits(0x007fffffu), bits(0x807fffffu),
                          bits(0x00800000u), bits(0x80800000u), 1e-38f,        9.9999e-6f,        1e-5f,   1.0001e-5f, 0.25f * 0.31830987f, 0.31830987f,
                          -0.31830987f,  1.0f,          3.0f,              inf,               -inf,    nan};
  for (uint32_t i = 0; i < 42; ++i) p.push_back(uni(0.0f, 1.0f) * 0.31830987f);  // |cos theta| / pi
  std::vector<float> q = {0.0f, -0.0f, den, bits(0x00800000u), 1e-6f, 0.5e-5f, 0.1f, 0.5f * 0.31830987f, 7.5f, inf, nan};
  const float one = 1.0f;

  float *d_normals = nullptr, *d_p = nullptr, *d_q = nullptr, *d_one = nullptr;
  uint32_t* d_out = nullptr;
  CHECK(hipMalloc(&d_normals, normals.size() * 4u));
  CHECK(hipMalloc(&d_p, p.size() * 4u));
  CHECK(hipMalloc(&d_q, q.size() * 4u));
  CHECK(hipMalloc(&d_one, 4u));
  CHECK(hipMalloc(&d_out, 8u * 4u));
  CHECK(hipMemcpy(d_normals, normals.data(), normals.size() * 4u, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_p, p.data(), p.size() * 4u, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_q, q.data(), q.size() * 4u, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_one, &one, 4u, hipMemcpyHostToDevice));
  int bad = 0;
  for (uint32_t half = 0; half < 2u; ++half) {
    uint32_t out[8] = {0};
    CHECK(hipMemset(d_out, 0, sizeof out));
    hipLaunchKernelGGL(frame_kernel, dim3(1), dim3(PROBE_BLOCK), 0, 0, d_normals, N_TOTAL, half, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    printf("frame %u %u\n", out[0], out[1]);
    if (out[1] != 0u) {
      static const char* const field[6] = {"u.x", "u.y", "u.z", "v.x", "v.y", "v.z"};
      const float* w = &normals[3u * out[2]];
      printf("first mismatch: run %u normal %u (%.9g %.9g %.9g) %s: select %08x branch %08x\n", half, out[2], w[0], w[1], w[2],
             field[out[3] < 6u ? out[3] : 0u], out[4], out[5]);
      bad = 1;
    }
  }
  {
    uint32_t out[8] = {0};
    CHECK(hipMemset(d_out, 0, sizeof out));
    hipLaunchKernelGGL(pdf_kernel, dim3(1), dim3(PROBE_BLOCK), 0, 0, d_one, d_p, (uint32_t)p.size(), d_q, (uint32_t)q.size(), d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    printf("rcp1 %08x\n", out[7]);
    printf("pdf %u %u\n", out[0], out[1]);
    if (out[7] != 0x3f800000u) bad = 1;
    if (out[1] != 0u) {
      uint32_t pb, qb;
      memcpy(&pb, &p[out[2]], 4);
      memcpy(&qb, &q[out[3]], 4);
      printf("first mismatch: p %08x q %08x %s: without the multiply %08x with it %08x\n", pb, qb, out[4] ? "p < 1e-5" : "0.5 p + q", out[5], out[6]);
      bad = 1;
    }
  }
  hipFree(d_normals);
  hipFree(d_p);
  hipFree(d_q);
  hipFree(d_one);
  hipFree(d_out);
  return bad;
}
