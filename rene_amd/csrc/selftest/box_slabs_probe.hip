// box_slabs_probe.hip -- the two forms of the box item's slab evaluation (../box_slabs.h) against each other on the device it runs on: the dot
// products on the vector pipe (box_slabs_valu) and on the matrix pipe (box_slabs_matrix) must give the same bits in c0, c1, t_in, t_out, and the
// same accept decision and hit parameter out of the shared tail.
//
//   box_slabs_probe RECORDS.npy     the item records of a small scene, a (n, 16) uint32 .npy as rene_scene_small_items hands them out
//                                   (tests/golden/cornell_small_items.npy: Cornell's room with its open face and the two blocks)
//
// One workgroup.  Rays: random ones inside and around the boxes; directions with one or two components of exactly +0 / -0 (parallel to the slabs of
// an axis-aligned box: c1 = +-0) and directions perpendicular to a skew box's axis; origins on a face (c0 = 0 or 1 up to rounding); origins one tmin
// before a face (a hit at tmin); origins with +-0 components.  Two runs: every lane with a ray; and an irregular half of the lanes without one
// (NaN in their registers), the matrix form called with every lane enabled -- as a caller in a kernel has to, hoisted out of its divergent
// branch -- and the vector form inside the divergent branch of the live lanes.
// Prints "compared mismatched" per run and a line for the first mismatch; exits 0 iff nothing mismatched.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../box_slabs.h"

using namespace rene;

constexpr uint32_t PROBE_BLOCK = 256, MAX_RECORDS = 64;
typedef float float16v __attribute__((ext_vector_type(16)));

#define CHECK(x)                                                                          \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                             \
      return 2;                                                                           \
    }                                                                                     \
  } while (0)

// out[0] = comparisons, out[1] = mismatches, out[2..] = the first mismatch: ray, record, field, the two values' bits
__global__ void __launch_bounds__(PROBE_BLOCK) probe_kernel(const float* records, uint32_t n_records, const uint32_t* boxes, uint32_t n_boxes,
                                                             const float* rays, uint32_t n_rays, uint32_t half, uint32_t* out) {
  __shared__ float lds_items[MAX_RECORDS * 16];
  for (uint32_t i = threadIdx.x; i < n_records * 16u; i += PROBE_BLOCK) lds_items[i] = records[i];
  __syncthreads();
  const __attribute__((address_space(3))) float* items = (const __attribute__((address_space(3))) float*)lds_items;
  typedef const __attribute__((address_space(4))) float16v* item_ptr;
  item_ptr base = (item_ptr)(const void*)records;
  const float tmin = 0.001f, first_t = __uint_as_float(__float_as_uint(100000.0f) + 1u);
  uint32_t compared = 0, mismatched = 0;
  for (uint32_t j0 = 0; j0 < n_rays; j0 += PROBE_BLOCK) {  // n_rays is a multiple of the block: every lane makes every pass
    const uint32_t j = j0 + threadIdx.x;
    // the irregular half: a hash of the lane and the pass
    const bool live = !half || (((threadIdx.x * 2654435761u) ^ (j0 * 40503u)) >> 13 & 1u) != 0u;
    const float nan = __uint_as_float(0x7fc00000u);
    const float ox = live ? rays[6 * j] : nan, oy = live ? rays[6 * j + 1] : nan, oz = live ? rays[6 * j + 2] : nan;
    const float dx = live ? rays[6 * j + 3] : nan, dy = live ? rays[6 * j + 4] : nan, dz = live ? rays[6 * j + 5] : nan;
    for (uint32_t b = 0; b < n_boxes; ++b) {
      const uint32_t k = boxes[b];  // wave-uniform
      const float16v q = base[k];
      const uint32_t open_face = __float_as_uint(q[14]);
      // every lane enabled here
      const BoxSlabs m = box_slabs_matrix(items + 16u * k, threadIdx.x, ox, oy, oz, dx, dy, dz);
      float tm = 0.0f;
      const bool hm = box_accept(m, open_face, tmin, first_t, tm);
      if (live) {  // divergent in the second run
        const BoxSlabs v = box_slabs_valu(q, ox, oy, oz, dx, dy, dz);
        float tv = 0.0f;
        const bool hv = box_accept(v, open_face, tmin, first_t, tv);
        const uint32_t got[10] = {__float_as_uint(m.c0[0]), __float_as_uint(m.c0[1]), __float_as_uint(m.c0[2]), __float_as_uint(m.c1[0]),
                                  __float_as_uint(m.c1[1]), __float_as_uint(m.c1[2]), __float_as_uint(m.t_in),  __float_as_uint(m.t_out),
                                  hm ? 1u : 0u,             hm ? __float_as_uint(tm) : 0u};
        const uint32_t want[10] = {__float_as_uint(v.c0[0]), __float_as_uint(v.c0[1]), __float_as_uint(v.c0[2]), __float_as_uint(v.c1[0]),
                                   __float_as_uint(v.c1[1]), __float_as_uint(v.c1[2]), __float_as_uint(v.t_in),  __float_as_uint(v.t_out),
                                   hv ? 1u : 0u,             hv ? __float_as_uint(tv) : 0u};
        for (uint32_t f = 0; f < 10u; ++f) {
          compared++;
          if (got[f] != want[f]) {
            if (atomicAdd(&out[1], 1u) == 0u) {
              out[2] = j; out[3] = k; out[4] = f; out[5] = got[f]; out[6] = want[f];
            }
            mismatched++;
          }
        }
      }
    }
  }
  atomicAdd(&out[0], compared);
  (void)mismatched;
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
static void normalise(float* d) {
  const float l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (l > 0.0f) d[0] /= l, d[1] /= l, d[2] /= l;
}
// the point whose box coordinates are c: solves M o + w = c, M's rows the three x' of record q
static void box_point(const float* q, const double* c, float* o) {
  double m[3][3], r[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) m[i][j] = q[4 * i + j];
    r[i] = c[i] - q[4 * i + 3];
  }
  const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                     m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
  for (int j = 0; j < 3; ++j) {
    double a[3][3];
    memcpy(a, m, sizeof a);
    for (int i = 0; i < 3; ++i) a[i][j] = r[i];
    const double dj = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                      a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    o[j] = (float)(dj / det);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: box_slabs_probe RECORDS.npy\n");
    return 2;
  }
  // a version-1 .npy: 10 bytes, the header's length in bytes 8 and 9, the header, then the words
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::vector<unsigned char> bytes;
  unsigned char buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
  fclose(f);
  if (bytes.size() < 10 || memcmp(bytes.data(), "\x93NUMPY\x01", 7) != 0) {
    fprintf(stderr, "%s: not a version-1 .npy file\n", argv[1]);
    return 2;
  }
  const size_t off = 10u + bytes[8] + 256u * bytes[9];
  if (off > bytes.size() || (bytes.size() - off) % 64u != 0) {
    fprintf(stderr, "%s: not (n, 16) 32-bit words\n", argv[1]);
    return 2;
  }
  const uint32_t n_records = (uint32_t)((bytes.size() - off) / 64u);
  if (n_records == 0 || n_records > MAX_RECORDS) {
    fprintf(stderr, "%s: %u records (1 .. %u)\n", argv[1], n_records, MAX_RECORDS);
    return 2;
  }
  std::vector<float> records(n_records * 16u);
  memcpy(records.data(), bytes.data() + off, records.size() * 4u);
  std::vector<uint32_t> boxes;
  for (uint32_t k = 0; k < n_records; ++k) {
    uint32_t kind;
    memcpy(&kind, &records[16u * k + 12u], 4);
    if (kind == BOX_KIND_BITS) boxes.push_back(k);
  }
  if (boxes.empty()) {
    fprintf(stderr, "%s: no box item\n", argv[1]);
    return 2;
  }

  // ---- the rays ----
  std::vector<float> rays;
  auto push = [&](const float* o, const float* d) {
    for (int i = 0; i < 3; ++i) rays.push_back(o[i]);
    for (int i = 0; i < 3; ++i) rays.push_back(d[i]);
  };
  const float tmin = 0.001f;
  for (uint32_t i = 0; i < 2048; ++i) {  // random: origins in and around the boxes (box coordinates -0.5 .. 1.5 of a random box), any direction
    const float* q = &records[16u * boxes[rnd() % boxes.size()]];
    const double c[3] = {uni(-0.5f, 1.5f), uni(-0.5f, 1.5f), uni(-0.5f, 1.5f)};
    float o[3], d[3] = {uni(-1.f, 1.f), uni(-1.f, 1.f), uni(-1.f, 1.f)};
    box_point(q, c, o);
    normalise(d);
    push(o, d);
  }
  for (uint32_t i = 0; i < 768; ++i) {  // one or two direction components exactly zero, either sign; origin components zeroed likewise now and then
    const float* q = &records[16u * boxes[rnd() % boxes.size()]];
    const double c[3] = {uni(-0.5f, 1.5f), uni(-0.5f, 1.5f), uni(-0.5f, 1.5f)};
    float o[3], d[3] = {uni(-1.f, 1.f), uni(-1.f, 1.f), uni(-1.f, 1.f)};
    box_point(q, c, o);
    const uint32_t m = 1u + rnd() % 6u;  // which components: never all three
    for (int a = 0; a < 3; ++a)
      if (m >> a & 1u) d[a] = (rnd() & 1u) ? 0.0f : -0.0f;
    normalise(d);
    if (i & 1u) o[rnd() % 3u] = (rnd() & 1u) ? 0.0f : -0.0f;
    push(o, d);
  }
  for (uint32_t i = 0; i < 512; ++i) {  // perpendicular to one axis of the box (skew boxes: c1 near zero, of either sign, through a cancellation)
    const float* q = &records[16u * boxes[rnd() % boxes.size()]];
    const float* x = q + 4u * (rnd() % 3u);
    const double c[3] = {uni(-0.5f, 1.5f), uni(-0.5f, 1.5f), uni(-0.5f, 1.5f)};
    float o[3], r[3] = {uni(-1.f, 1.f), uni(-1.f, 1.f), uni(-1.f, 1.f)};
    box_point(q, c, o);
    float d[3] = {x[1] * r[2] - x[2] * r[1], x[2] * r[0] - x[0] * r[2], x[0] * r[1] - x[1] * r[0]};
    normalise(d);
    if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) d[0] = 1.0f;
    push(o, d);
  }
  for (uint32_t i = 0; i < 768; ++i) {  // the origin on a face (i even), or one tmin before it along the ray (i odd): a hit at tmin
    const float* q = &records[16u * boxes[rnd() % boxes.size()]];
    double c[3] = {uni(0.f, 1.f), uni(0.f, 1.f), uni(0.f, 1.f)};
    c[rnd() % 3u] = (rnd() & 1u) ? 1.0 : 0.0;
    float o[3], d[3] = {uni(-1.f, 1.f), uni(-1.f, 1.f), uni(-1.f, 1.f)};
    box_point(q, c, o);
    normalise(d);
    if (i & 1u)
      for (int a = 0; a < 3; ++a) o[a] -= tmin * d[a];
    push(o, d);
  }
  const uint32_t n_rays = (uint32_t)(rays.size() / 6u);
  static_assert((2048 + 768 + 512 + 768) % PROBE_BLOCK == 0, "every lane makes every pass");

  float *d_records = nullptr, *d_rays = nullptr;
  uint32_t *d_boxes = nullptr, *d_out = nullptr;
  CHECK(hipMalloc(&d_records, records.size() * 4u));
  CHECK(hipMalloc(&d_rays, rays.size() * 4u));
  CHECK(hipMalloc(&d_boxes, boxes.size() * 4u));
  CHECK(hipMalloc(&d_out, 8u * 4u));
  CHECK(hipMemcpy(d_records, records.data(), records.size() * 4u, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_rays, rays.data(), rays.size() * 4u, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_boxes, boxes.data(), boxes.size() * 4u, hipMemcpyHostToDevice));
  int bad = 0;
  for (uint32_t half = 0; half < 2u; ++half) {
    uint32_t out[8] = {0};
    CHECK(hipMemset(d_out, 0, sizeof out));
    hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(PROBE_BLOCK), 0, 0, d_records, n_records, d_boxes, (uint32_t)boxes.size(), d_rays, n_rays, half, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out, d_out, sizeof out, hipMemcpyDeviceToHost));
    printf("%u %u\n", out[0], out[1]);
    if (out[1] != 0u) {
      static const char* const field[10] = {"c0.x", "c0.y", "c0.z", "c1.x", "c1.y", "c1.z", "t_in", "t_out", "accept", "t"};
      const float* r = &rays[6u * out[2]];
      printf("first mismatch: run %u ray %u (o %.9g %.9g %.9g d %.9g %.9g %.9g) record %u %s: matrix %08x vector %08x\n", half, out[2], r[0], r[1], r[2],
             r[3], r[4], r[5], out[3], field[out[4] < 10u ? out[4] : 0u], out[5], out[6]);
      bad = 1;
    }
  }
  hipFree(d_records);
  hipFree(d_rays);
  hipFree(d_boxes);
  hipFree(d_out);
  return bad;
}
