// kernels_denoise.hip -- the build-defined denoiser `atrous` (rene_denoise and its kin, include/rene_hip.h): an edge-avoiding a-trous wavelet filter
// (Dammertz et al. 2010; the spatial half of SVGF, Schied et al. 2017) guided by the first-hit normal and albedo layers and by the variance of
// the pixel's mean, which the eight frame chains (device_scene.h, CHAINS) give for nothing: eight independent sub-means per pixel.
//
//   prepare   denoise_prepare_kernel<TILES, PACKED, TRIM>, one thread per owned pixel slot (chain_pass.h maps it to its pixel): reads the pixel's
//             eight radiance records and the resolved guide layers, writes pixel-major records rec[y][x] = {demodulated colour.rgb, variance of
//             the mean of its luminance}, the constant guides g0 = {normal.xyz, albedo.r}, g1 = {albedo.g, albedo.b, 0, 0} (fp32: 16 + 32 bytes
//             per pixel) and the unfiltered variance plane
//               TILES   (rene_denoise_tiles) the constants of the workgroup's 32 x 32 tile -- its own frame count N_t -- come from a table
//                       (kernels.h, DENOISE_SET_FLOATS) and every pixel is marked: g1 = {albedo.g, albedo.b, 1, (float)N_t}, whose .z and .w the
//                       taps load anyway and do not use.  A pixel of an invalid tile (NOISE_SET_NONE) gets zero records, but for
//                       g0 = {the pixel's unfiltered radiance sum, 0}, which finalize hands out
//               PACKED  (rene_denoise_shard_prepare) every store lands in the owned tile's block of a tile-packed buffer (kernels.h, DN_PACKED_*)
//                       instead of at the pixel's index, and a slot outside the image is stored as zero records: the buffer is deterministic
//                       byte for byte.  The tile's origin is an OWNED tile's: the other instantiations run on unsharded contexts only
//               TRIM    (rene_denoise_robust, rene_denoise_tiles_robust) steps 2 and 3 over the chains that kernels_denoise_trim.hip decided to
//                       keep: one 4-byte word per pixel more, trim[y][x] = j | kept << 8.  Where j == 0 every expression is the plain
//                       prepare's -- the same source line -- on the same constants in the same order: such a pixel's records are bit for bit
//                       rene_denoise's (rene_denoise_tiles').  Where j > 0 the pixel's own 1 / n_kept, n_c / n_kept and 1 / (h - 1) take the
//                       places of inv_n, chain_share and inv_km1; they are computed here, with this unit's division
//   pass      atrous_pass_kernel<S, MASKED>, one launch per iteration i (step s = 2^i), one thread per pixel, 25 taps of three 16-byte loads
//             each.  For small steps the workgroup's 32 x 8 tile and a halo of 2 s pixels are staged in LDS (S > 0); the larger steps read their
//             taps through L2 (S == 0: consecutive lanes stay on consecutive records).  Both do the same arithmetic in the same order.
//             MASKED (the records of a TILES prepare) treats an invalid pixel exactly as a pixel outside the image: skipped as a tap -- by
//             control flow, as the border is, so that the sums of a valid pixel see the same operands in the same order -- and not filtered itself
//   finalize  denoise_finalize_kernel<MASKED> remodulates and scales by the frame count: the unit of rene_download.  MASKED: by the pixel's own
//             N_t; an invalid pixel hands out its unfiltered sum
//   mean      RENE_DENOISED_MEAN, on request: col * den of the last call's records
//   place     denoise_shard_place_kernel (rene_denoise_place_shard): one workgroup per packed tile, thread j takes slots j, j + 256, j + 512,
//             j + 768 (consecutive lanes read consecutive 16-byte records) and moves them to the pixel chain_pass.h's slot -> pixel map names.
//             Moves only: the bits arrive as sent
//
// Every kernel's body stays inside its __global__ template and is switched with `if constexpr`: moving the bodies into functions (the launch
// structure then travels by reference) changes the scalar loads and the register allocation of the kernels; this does not.
// A valid pixel's arithmetic is the same text whatever the instantiation: on a context whose tiles all hold the same frames TILES agrees with
// plain bit for bit.  Nothing here writes the accumulation state: chains, image and trim are read only.  No atomics.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "atrous_filter.h"

namespace rene {

struct NoArg {};  // the place of an argument that an instantiation does not take

template <bool TILES, bool PACKED, bool TRIM, class Sets, class Trim>
__global__ void __launch_bounds__(256) denoise_prepare_kernel(const float4* __restrict__ chains, const float4* __restrict__ image, float4* __restrict__ rec,
                                                              float4* __restrict__ guides, float* __restrict__ var_plane, DenoiseLaunch D, Sets T, Trim R) {
  static_assert(std::is_empty_v<Sets> == !TILES && std::is_empty_v<Trim> == !TRIM && (!PACKED || (TILES && !TRIM)), "denoise_prepare<> names the instantiations");
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // owned pixel slot (an unsharded context: tile = slot / 1024)
  if (i >= D.grid.n_slots) return;
  const uint32_t s = (uint32_t)i;
  // (a tile shard: owned tile k is image tile shard_rank + k * shard_count)
  const uint2 o = PACKED ? owned_tile_origin(D.grid, s / TILE_SLOTS) : image_tile_origin(D.grid, s / TILE_SLOTS), d = slot_pixel(s % TILE_SLOTS);
  const uint32_t x = o.x + d.x, y = o.y + d.y;
  // PACKED: rec, guides and var_plane all point at the packed body: owned tile s / 1024's block starts pk records in, the pixel is slot pr of it
  const size_t pk = (size_t)(s / TILE_SLOTS) * DN_PACKED_TILE_F4, pr = s % TILE_SLOTS;
  const auto store = [&](size_t p, const float4& r, const float4& g0, const float4& g1, float v) {
    if constexpr (PACKED) {
      rec[pk + pr] = r;
      guides[pk + DN_PACKED_GUIDES_F4 + 2 * pr] = g0;
      guides[pk + DN_PACKED_GUIDES_F4 + 2 * pr + 1] = g1;
      var_plane[4 * (pk + DN_PACKED_VAR_F4) + pr] = v;
    } else {
      rec[p] = r;
      guides[2 * p] = g0;
      guides[2 * p + 1] = g1;
      var_plane[p] = v;
    }
  };
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (x >= D.grid.width || y >= D.grid.height) {
    if constexpr (PACKED) store(0, zero, zero, zero, 0.0f);  // a slot of a ragged tile: zero records, so that the buffer is the same byte for byte
    return;
  }
  const size_t n4 = (size_t)3 * D.grid.n_slots, p = (size_t)y * D.grid.width + x, np = (size_t)D.grid.width * D.grid.height;
  uint32_t cn[CHAINS] = {};  // TRIM: the n_c behind D.chain_share
  if constexpr (TRIM && !TILES) {
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) cn[g] = R.chain_n[g];
  }
  if constexpr (TILES) {  // the constants of this workgroup's tile: its 256 consecutive slots lie inside one owned tile (workgroup-uniform: scalar loads)
    const uint32_t set = T.tile_set[blockIdx.x / (TILE_SLOTS / 256u)];
    if (set == NOISE_SET_NONE) {  // finite records, and the unfiltered sum where finalize finds it (a move: the image's bits)
      const float4 s0 = image[p];
      store(p, zero, make_float4(s0.x, s0.y, s0.z, 0.0f), zero, 0.0f);
      return;
    }
    const float* k = T.sets + (size_t)set * (TRIM ? DENOISE_ROBUST_SET_FLOATS : DENOISE_SET_FLOATS);
    D.inv_n = k[0];
    D.inv_km1 = k[1];
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) {
      D.chain_share[g] = k[2u + g];
      D.chain_inv[g] = k[2u + CHAINS + g];
      if constexpr (TRIM) cn[g] = __float_as_uint(k[DENOISE_SET_FLOATS + g]);
    }
    D.n_frames = k[NOISE_SET_FLOATS];
  }
  // the constants from here on.  TRIM: a copy, so that all of them are fetched here with a few wide scalar loads, ahead of the chain records --
  // read in place, as the plain prepare reads them, they are fetched one by one inside the per-chain branches, which the kept bits make divergent
  std::conditional_t<TRIM, const DenoiseLaunch, const DenoiseLaunch&> K = D;
  float4 c[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) c[g] = chains[(size_t)g * n4 + i];  // layer 0 of chain g
  uint32_t j = 0, kept = (1u << CHAINS) - 1u;  // nothing trimmed, every chain kept ...
  if constexpr (TRIM) {                        // ... or what denoise_trim_kernel decided
    const uint32_t w = R.trim[p];
    j = w & 0xffu;
    kept = w >> 8;
  }
  // the kept chains' sums in chain order, from C_0 or +0 (everything kept: ((c0 + c1) + c2) + ... like resolve_chains_kernel)
  float sr = (kept & 1u) ? c[0].x : 0.0f, sg = (kept & 1u) ? c[0].y : 0.0f, sb = (kept & 1u) ? c[0].z : 0.0f;
  uint32_t n_kept = (kept & 1u) ? cn[0] : 0u, kk = cn[0] ? 1u : 0u;
#pragma unroll
  for (uint32_t g = 1; g < CHAINS; ++g) {
    if (kept >> g & 1u) {
      sr += c[g].x;
      sg += c[g].y;
      sb += c[g].z;
      n_kept += cn[g];
    }
    kk += cn[g] ? 1u : 0u;
  }
  // the pixel's own constants, which take the places of the launch's (the tile's) where chains are trimmed: 1 / n_kept, 1 / (h - 1)
  const float fk = (float)n_kept, inv_fk = 1.0f / fk, inv_hm1 = 1.0f / (float)(kk - 2u * j - 1u);
  const float4 s1 = image[np + p], s2 = image[2 * np + p];
  const float nx = s1.x * K.inv_n, ny = s1.y * K.inv_n, nz = s1.z * K.inv_n;
  const float ar = s2.x * K.inv_n, ag = s2.y * K.inv_n, ab = s2.z * K.inv_n;
  const float ir = 1.0f / (ar + K.albedo_floor), ig = 1.0f / (ag + K.albedo_floor), ib = 1.0f / (ab + K.albedo_floor);
  const float inv_nk = j ? inv_fk : K.inv_n;
  const float dr = sr * inv_nk * ir, dg = sg * inv_nk * ig, db = sb * inv_nk * ib;
  const float lm = lum3(dr, dg, db);
  float var = 0.0f;
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    if (K.chain_share[g] > 0.0f && (kept >> g & 1u)) {  // chains that have received frames, and are kept
      const float share = j ? (float)cn[g] / fk : K.chain_share[g];
      const float t = lum3(c[g].x * K.chain_inv[g] * ir, c[g].y * K.chain_inv[g] * ig, c[g].z * K.chain_inv[g] * ib) - lm;
      var += share * (t * t);
    }
  }
  var *= j ? inv_hm1 : K.inv_km1;
  // TILES: valid, (float)N_t: where the taps load them with the albedo
  store(p, make_float4(dr, dg, db, var), make_float4(nx, ny, nz, ar), make_float4(ag, ab, TILES ? 1.0f : 0.0f, TILES ? K.n_frames : 0.0f), var);
}

// S > 0: the tile and a halo of 2 S pixels staged in LDS, step S; S == 0: step D.step, every tap from global memory
template <int S, bool MASKED>
__global__ void __launch_bounds__(DN_BLOCK) atrous_pass_kernel(const float4* __restrict__ rec, const float4* __restrict__ guides, float4* __restrict__ out, DenoiseLaunch D) {
  constexpr int HALO = 2 * S, LW = DN_TX + 2 * HALO, LH = DN_TY + 2 * HALO, LN = S ? LW * LH : 1;
  __shared__ float4 t_rec[LN], t_g0[LN], t_g1[LN];
  const int W = (int)D.grid.width, H = (int)D.grid.height;
  // Which tile this workgroup filters.  Workgroups are dealt round-robin over the chip's eight XCDs, each with an L2 of its own: with tiles in
  // launch order the eight neighbours of a tile sit behind eight different L2s and every one of them fetches the halo for itself (measured: a
  // step-8 pass read ten times the records' bytes through the L2s' memory side).  D.tile_columns > 0: XCD k (workgroups k, k + 8, ...) takes the
  // k-th eighth of the tiles in an order that walks super-columns of D.tile_columns tiles, row by row, so that the tiles in flight behind one L2
  // are neighbours.  Only the order changes: no pixel's arithmetic does.
  const uint32_t gx = (D.grid.width + DN_TX - 1) / DN_TX, gy = (D.grid.height + DN_TY - 1) / DN_TY;
  uint32_t bx, by;
  if (D.tile_columns) {
    const uint32_t tile = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);  // (the grid is a multiple of eight workgroups)
    if (tile >= gx * gy) return;
    const uint32_t cw = D.tile_columns, full = gx / cw, per = cw * gy, sc = tile / per;
    if (sc < full) {
      const uint32_t r = tile - sc * per;
      by = r / cw;
      bx = sc * cw + r % cw;
    } else {  // the last, narrower super-column
      const uint32_t wl = gx - full * cw, r = tile - full * per;
      by = r / wl;
      bx = full * cw + r % wl;
    }
  } else {
    if (blockIdx.x >= gx * gy) return;
    by = blockIdx.x / gx;
    bx = blockIdx.x - by * gx;
  }
  const int x0 = (int)bx * DN_TX, y0 = (int)by * DN_TY;
  const int tx = (int)threadIdx.x & (DN_TX - 1), ty = (int)threadIdx.x / DN_TX;
  const int x = x0 + tx, y = y0 + ty;
  if constexpr (S > 0) {
    for (int k = (int)threadIdx.x; k < LN; k += DN_BLOCK) {
      const int ly = k / LW, lx = k - ly * LW, gx = x0 - HALO + lx, gy = y0 - HALO + ly;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {  // (texels outside the image stay unwritten and are never read: their taps are skipped)
        const size_t q = (size_t)gy * W + gx;
        t_rec[k] = rec[q];
        t_g0[k] = guides[2 * q];
        t_g1[k] = guides[2 * q + 1];
      }
    }
    __syncthreads();
  }
  if (x >= W || y >= H) return;
  const int step = S ? S : (int)D.step;
  const int lc = (ty + HALO) * LW + tx + HALO;  // S: the pixel's place in the staged tile
  const size_t p = (size_t)y * W + x;
  Centre c;
  if (S) {
    c.rec = t_rec[lc];
    c.g0 = t_g0[lc];
    c.g1 = t_g1[lc];
  } else {
    c.rec = rec[p];
    c.g0 = guides[2 * p];
    c.g1 = guides[2 * p + 1];
  }
  if (MASKED && !dn_valid(c.g1)) {  // not filtered: its zero record goes on to the next iteration
    out[p] = c.rec;
    return;
  }
  c.lum = lum3(c.rec.x, c.rec.y, c.rec.z);
  {  // 3 x 3 filter (1 2 1) x (1 2 1) / 16 of the variance, taps outside the image skipped and the weights renormalised
    float gv = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        if (MASKED && (dx != 0 || dy != 0) && !dn_valid(S ? t_g1[lc + dy * LW + dx] : guides[2 * ((size_t)qy * W + qx) + 1])) continue;
        const float w = (float)((2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx))) * 0.0625f;
        const float v = S ? t_rec[lc + dy * LW + dx].w : rec[(size_t)qy * W + qx].w;
        gv += w * v;
        gw += w;
      }
    }
    c.sd = D.sigma_l * sqrtf(fmaxf(gv / gw, 0.0f));
  }
  Acc a{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int iy = -2; iy <= 2; ++iy) {
    const int qy = y + iy * step;
    if (qy < 0 || qy >= H) continue;
#pragma unroll
    for (int ix = -2; ix <= 2; ++ix) {
      const int qx = x + ix * step;
      if (qx < 0 || qx >= W) continue;
      const float h = h5(ix) * h5(iy);
      if (S) {
        const int k = lc + iy * S * LW + ix * S;
        if (MASKED && !dn_valid(t_g1[k])) continue;
        tap(c, D, h, t_rec[k], t_g0[k], t_g1[k], a);
      } else {
        const size_t q = (size_t)qy * W + qx;
        if constexpr (MASKED) {
          const float4 q1 = guides[2 * q + 1];  // (the record the tap reads anyway)
          if (!dn_valid(q1)) continue;
          tap(c, D, h, rec[q], guides[2 * q], q1, a);
        } else {
          tap(c, D, h, rec[q], guides[2 * q], guides[2 * q + 1], a);
        }
      }
    }
  }
  const float iw = 1.0f / a.w;  // the centre tap alone weighs 9 / 64
  out[p] = make_float4(a.r * iw, a.g * iw, a.b * iw, a.v * (iw * iw));
}

template <bool MASKED>
__global__ void __launch_bounds__(256) denoise_finalize_kernel(const float4* __restrict__ rec, const float4* __restrict__ guides, float4* __restrict__ out, DenoiseLaunch D) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)D.grid.width * D.grid.height) return;
  const float4 c = rec[p], g0 = guides[2 * p], g1 = guides[2 * p + 1];
  if (MASKED && !dn_valid(g1)) {  // the unfiltered image: prepare left the pixel's sum here
    out[p] = make_float4(g0.x, g0.y, g0.z, 0.0f);
    return;
  }
  const float n = MASKED ? g1.w : D.n_frames;  // (float)N_t
  out[p] = make_float4(c.x * (g0.w + D.albedo_floor) * n, c.y * (g1.x + D.albedo_floor) * n, c.z * (g1.y + D.albedo_floor) * n, 0.0f);
}

__global__ void __launch_bounds__(256) denoise_mean_kernel(const float4* __restrict__ rec, const float4* __restrict__ guides, float4* __restrict__ out, size_t n_px,
                                                           float albedo_floor, uint32_t masked) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_px) return;
  const float4 c = rec[p], g0 = guides[2 * p], g1 = guides[2 * p + 1];
  if (masked && !dn_valid(g1)) {
    out[p] = make_float4(g0.x, g0.y, g0.z, 0.0f);
    return;
  }
  out[p] = make_float4(c.x * (g0.w + albedo_floor), c.y * (g1.x + albedo_floor), c.z * (g1.y + albedo_floor), 0.0f);
}

__global__ void __launch_bounds__(PASS_BLOCK) denoise_shard_place_kernel(const float4* __restrict__ body, float4* __restrict__ rec, float4* __restrict__ guides,
                                                                        float* __restrict__ var_plane, TileGrid G) {
  const uint32_t tile = G.shard_rank + blockIdx.x * G.shard_count;
  const uint32_t tiles_y = (G.height + RENE_TILE_SIZE - 1u) / RENE_TILE_SIZE;
  if (tile >= G.tiles_x * tiles_y) return;  // (the host launches one workgroup per tile the rank owns: never taken)
  const uint2 o = image_tile_origin(G, tile);
  const float4* block = body + (size_t)blockIdx.x * DN_PACKED_TILE_F4;
  const float* block_var = reinterpret_cast<const float*>(block + DN_PACKED_VAR_F4);
#pragma unroll
  for (uint32_t q = 0; q < PASS_PER_THREAD; ++q) {
    const uint32_t r = threadIdx.x + q * PASS_BLOCK;
    const uint2 d = slot_pixel(r);
    const uint32_t x = o.x + d.x, y = o.y + d.y;
    if (x >= G.width || y >= G.height) continue;
    const size_t p = (size_t)y * G.width + x;
    rec[p] = block[r];
    guides[2 * p] = block[DN_PACKED_GUIDES_F4 + 2u * r];
    guides[2 * p + 1] = block[DN_PACKED_GUIDES_F4 + 2u * r + 1u];
    var_plane[p] = block_var[r];
  }
}

// the instantiation that takes these switches: the tile sets and the trim plane are arguments only where they are read
template <bool TILES, bool PACKED, bool TRIM>
constexpr auto denoise_prepare = denoise_prepare_kernel<TILES, PACKED, TRIM, std::conditional_t<TILES, DenoiseTileSets, NoArg>, std::conditional_t<TRIM, DenoiseTrimmed, NoArg>>;

hipError_t launch_denoise_prepare(const float* chains, const float* image, const DenoisePrepare& A, const DenoiseLaunch& D, hipStream_t st) {
  static_assert(TILE_SLOTS % DN_PREPARE_BLOCK == 0, "a prepare workgroup lies inside one tile");
  static_assert(DN_PACKED_TILE_BYTES == 52u * TILE_SLOTS, "52 bytes per slot");
  if (D.grid.n_slots == 0) return hipSuccess;
  const bool tiles = A.sets.tile_set != nullptr, packed = A.body != nullptr, trim = A.trimmed.trim != nullptr;
  if (packed && (!tiles || trim)) return hipErrorInvalidValue;  // (no such kernel)
  float4* const rec = packed ? static_cast<float4*>(A.body) : reinterpret_cast<float4*>(A.rec);
  float4* const guides = packed ? static_cast<float4*>(A.body) : reinterpret_cast<float4*>(A.guides);
  float* const var_plane = packed ? static_cast<float*>(A.body) : A.var_plane;
  const auto go = [&](auto kernel, auto sets, auto trimmed) {
    hipLaunchKernelGGL(kernel, dim3((D.grid.n_slots + DN_PREPARE_BLOCK - 1u) / DN_PREPARE_BLOCK), dim3(DN_PREPARE_BLOCK), 0, st, reinterpret_cast<const float4*>(chains),
                       reinterpret_cast<const float4*>(image), rec, guides, var_plane, D, sets, trimmed);
  };
  if (packed) go(denoise_prepare<true, true, false>, A.sets, NoArg{});
  else if (tiles && trim) go(denoise_prepare<true, false, true>, A.sets, A.trimmed);
  else if (tiles) go(denoise_prepare<true, false, false>, A.sets, NoArg{});
  else if (trim) go(denoise_prepare<false, false, true>, NoArg{}, A.trimmed);
  else go(denoise_prepare<false, false, false>, NoArg{}, NoArg{});
  return hipGetLastError();
}

// steps up to `stage_max` go through the LDS-staged kernel.  The default is RENE_DENOISE_STAGE_MAX (-DRENE_DENOISE_STAGE_MAX=0 builds a library that
// never stages: the A/B of DESIGN.md section 4c); the environment variable of the same name overrides it per call (rene_hip.cpp)
#ifndef RENE_DENOISE_STAGE_MAX
#define RENE_DENOISE_STAGE_MAX 4
#endif
int denoise_stage_max() { return RENE_DENOISE_STAGE_MAX; }

template <bool MASKED>
static auto atrous_pass(uint32_t s) {
  return s == 1 ? atrous_pass_kernel<1, MASKED> : s == 2 ? atrous_pass_kernel<2, MASKED> : s == 4 ? atrous_pass_kernel<4, MASKED> : atrous_pass_kernel<0, MASKED>;
}

hipError_t launch_atrous_pass(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, bool masked, int stage_max, hipStream_t st) {
  const uint32_t tiles = ((D.grid.width + DN_TX - 1) / DN_TX) * ((D.grid.height + DN_TY - 1) / DN_TY);  // (at most 2^21 at 16384 x 16384)
  const uint32_t s = D.step <= (uint32_t)(stage_max < 0 ? 0 : stage_max) ? D.step : 0u;
  hipLaunchKernelGGL(masked ? atrous_pass<true>(s) : atrous_pass<false>(s), dim3((tiles + 7u) & ~7u), dim3(DN_BLOCK), 0, st, reinterpret_cast<const float4*>(rec),
                     reinterpret_cast<const float4*>(guides), reinterpret_cast<float4*>(out), D);
  return hipGetLastError();
}

hipError_t launch_denoise_finalize(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, bool masked, hipStream_t st) {
  const size_t n = (size_t)D.grid.width * D.grid.height;
  hipLaunchKernelGGL(masked ? denoise_finalize_kernel<true> : denoise_finalize_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(rec), reinterpret_cast<const float4*>(guides), reinterpret_cast<float4*>(out), D);
  return hipGetLastError();
}

hipError_t launch_denoise_mean(const float* rec, const float* guides, float* out, uint32_t width, uint32_t height, float albedo_floor, bool masked, hipStream_t st) {
  const size_t n = (size_t)width * height;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(rec),
                     reinterpret_cast<const float4*>(guides), reinterpret_cast<float4*>(out), n, albedo_floor, masked ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_denoise_shard_place(const void* body, uint32_t n_owned, float* rec, float* guides, float* var_plane, const TileGrid& G, hipStream_t st) {
  if (n_owned == 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_shard_place_kernel, dim3(n_owned), dim3(PASS_BLOCK), 0, st, static_cast<const float4*>(body), reinterpret_cast<float4*>(rec),
                     reinterpret_cast<float4*>(guides), var_plane, G);
  return hipGetLastError();
}

}  // namespace rene
