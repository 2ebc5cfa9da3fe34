// atrous_kernels.inc -- the text of the `atrous` denoiser's prepare and pass kernels, written once and compiled twice (like device_code.inc): by
// kernels_denoise.hip with ATROUS_TILES 0 (rene_denoise: one frame count for the whole image) and by kernels_denoise_tiles.hip with ATROUS_TILES 1
// (rene_denoise_tiles: every 32 x 32 tile with the constants of its own frame count N_t, tiles that cannot be estimated masked out).
//
// It is text and not a template because the kernels of kernels_denoise.hip are to stay instruction for instruction what they were: moving their
// bodies into functions (the launch structure then travels by reference) changed the scalar loads and the register allocation of all six; with
// ATROUS_TILES 0 the preprocessor leaves exactly the text those kernels had.
//
//   ATROUS_TILES 1, prepare   takes the constants of the workgroup's tile from a table (kernels.h, DENOISE_SET_FLOATS) and marks every pixel:
//                             guides[2 p + 1] = {albedo.g, albedo.b, 1, (float)N_t}.  A pixel of an invalid tile (NOISE_SET_NONE) gets zero records,
//                             but for guides[2 p] = {the pixel's unfiltered radiance sum, 0}, which finalize hands out
//   ATROUS_TILES 1, pass      treats an invalid pixel exactly as a pixel outside the image: skipped as a tap -- by control flow, as the border is, so
//                             that the sums of a valid pixel see the same operands in the same order -- and not filtered itself
//
// A valid pixel's arithmetic is the same text either way: on a context whose tiles all hold the same frames the two units agree bit for bit.
//
// A third unit, kernels_denoise_shard.hip, compiles the ATROUS_TILES 1 prepare once more with ATROUS_PACKED 1 (rene_denoise_shard_prepare): the same
// text, but every store lands in the owned tile's block of a tile-packed buffer (kernels.h, DN_PACKED_*) instead of at the pixel's index, and a slot
// outside the image is stored as zero records instead of being left out.  Only the four output indices, that one branch and the tile's origin (an OWNED tile's: the two other units run on unsharded
// contexts only, where slot / 1024 is the image tile) are switched; with
// ATROUS_PACKED undefined or 0 the preprocessor leaves the text the two units above had.  The packed unit takes no pass kernel from here.
#ifndef ATROUS_PACKED
#define ATROUS_PACKED 0
#endif
#if ATROUS_PACKED
#define ATROUS_PREPARE_KERNEL denoise_shard_prepare_kernel
#define ATROUS_TILE_ORIGIN owned_tile_origin  // a tile shard: owned tile k is image tile shard_rank + k * shard_count
#define ATROUS_REC_AT (pk + pr)
#define ATROUS_G0_AT (pk + DN_PACKED_GUIDES_F4 + 2 * pr)
#define ATROUS_G1_AT (pk + DN_PACKED_GUIDES_F4 + 2 * pr + 1)
#define ATROUS_VAR_AT (4 * (pk + DN_PACKED_VAR_F4) + pr)
#else
#define ATROUS_TILE_ORIGIN image_tile_origin
#define ATROUS_REC_AT p
#define ATROUS_G0_AT 2 * p
#define ATROUS_G1_AT 2 * p + 1
#define ATROUS_VAR_AT p
#if ATROUS_TILES
#define ATROUS_PREPARE_KERNEL denoise_tiles_prepare_kernel
#define ATROUS_PASS_KERNEL atrous_pass_tiles_kernel
#else
#define ATROUS_PREPARE_KERNEL denoise_prepare_kernel
#define ATROUS_PASS_KERNEL atrous_pass_kernel
#endif
#endif

__global__ void __launch_bounds__(256) ATROUS_PREPARE_KERNEL(const float4* __restrict__ chains, const float4* __restrict__ image, float4* __restrict__ rec,
                                                             float4* __restrict__ guides, float* __restrict__ var_plane, DenoiseLaunch D
#if ATROUS_TILES
                                                             , DenoiseTileSets T
#endif
) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // owned pixel slot (an unsharded context: tile = slot / 1024)
  if (i >= D.grid.n_slots) return;
  const uint32_t s = (uint32_t)i;
  const uint2 o = ATROUS_TILE_ORIGIN(D.grid, s / TILE_SLOTS), d = slot_pixel(s % TILE_SLOTS);
  const uint32_t x = o.x + d.x, y = o.y + d.y;
#if ATROUS_PACKED
  // (rec, guides and var_plane all point at the packed body: owned tile s / 1024's block starts pk records in, the pixel is slot pr of it)
  const size_t pk = (size_t)(s / TILE_SLOTS) * DN_PACKED_TILE_F4, pr = s % TILE_SLOTS;
  if (x >= D.grid.width || y >= D.grid.height) {  // a slot of a ragged tile: zero records, so that the buffer is the same byte for byte
    rec[ATROUS_REC_AT] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    guides[ATROUS_G0_AT] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    guides[ATROUS_G1_AT] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    var_plane[ATROUS_VAR_AT] = 0.0f;
    return;
  }
#else
  if (x >= D.grid.width || y >= D.grid.height) return;
#endif
  const size_t n4 = (size_t)3 * D.grid.n_slots, p = (size_t)y * D.grid.width + x, np = (size_t)D.grid.width * D.grid.height;
#if ATROUS_TILES
  {  // the constants of this workgroup's tile: its 256 consecutive slots lie inside one owned tile (workgroup-uniform: scalar loads)
    const uint32_t set = T.tile_set[blockIdx.x / (TILE_SLOTS / 256u)];
    if (set == NOISE_SET_NONE) {  // finite records, and the unfiltered sum where finalize finds it (a move: the image's bits)
      const float4 s0 = image[p];
      rec[ATROUS_REC_AT] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      guides[ATROUS_G0_AT] = make_float4(s0.x, s0.y, s0.z, 0.0f);
      guides[ATROUS_G1_AT] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      var_plane[ATROUS_VAR_AT] = 0.0f;
      return;
    }
    const float* k = T.sets + (size_t)set * DENOISE_SET_FLOATS;
    D.inv_n = k[0];
    D.inv_km1 = k[1];
#pragma unroll
    for (uint32_t g = 0; g < CHAINS; ++g) {
      D.chain_share[g] = k[2u + g];
      D.chain_inv[g] = k[2u + CHAINS + g];
    }
    D.n_frames = k[NOISE_SET_FLOATS];
  }
#endif
  float4 c[CHAINS];
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) c[g] = chains[(size_t)g * n4 + i];  // layer 0 of chain g
  float sr = c[0].x, sg = c[0].y, sb = c[0].z;  // ((c0 + c1) + c2) + ... like resolve_chains_kernel
#pragma unroll
  for (uint32_t g = 1; g < CHAINS; ++g) {
    sr += c[g].x;
    sg += c[g].y;
    sb += c[g].z;
  }
  const float4 s1 = image[np + p], s2 = image[2 * np + p];
  const float nx = s1.x * D.inv_n, ny = s1.y * D.inv_n, nz = s1.z * D.inv_n;
  const float ar = s2.x * D.inv_n, ag = s2.y * D.inv_n, ab = s2.z * D.inv_n;
  const float ir = 1.0f / (ar + D.albedo_floor), ig = 1.0f / (ag + D.albedo_floor), ib = 1.0f / (ab + D.albedo_floor);
  const float dr = sr * D.inv_n * ir, dg = sg * D.inv_n * ig, db = sb * D.inv_n * ib;
  const float lm = lum3(dr, dg, db);
  float var = 0.0f;
#pragma unroll
  for (uint32_t g = 0; g < CHAINS; ++g) {
    if (D.chain_share[g] > 0.0f) {  // chains that have received frames
      const float t = lum3(c[g].x * D.chain_inv[g] * ir, c[g].y * D.chain_inv[g] * ig, c[g].z * D.chain_inv[g] * ib) - lm;
      var += D.chain_share[g] * (t * t);
    }
  }
  var *= D.inv_km1;
  rec[ATROUS_REC_AT] = make_float4(dr, dg, db, var);
  guides[ATROUS_G0_AT] = make_float4(nx, ny, nz, ar);
#if ATROUS_TILES
  guides[ATROUS_G1_AT] = make_float4(ag, ab, 1.0f, D.n_frames);  // valid, (float)N_t: where the taps load them with the albedo
#else
  guides[ATROUS_G1_AT] = make_float4(ag, ab, 0.0f, 0.0f);
#endif
  var_plane[ATROUS_VAR_AT] = var;
}

#if !ATROUS_PACKED
// S > 0: the tile and a halo of 2 S pixels staged in LDS, step S; S == 0: step D.step, every tap from global memory
template <int S>
__global__ void __launch_bounds__(DN_BLOCK) ATROUS_PASS_KERNEL(const float4* __restrict__ rec, const float4* __restrict__ guides, float4* __restrict__ out, DenoiseLaunch D) {
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
#if ATROUS_TILES
  if (!dn_valid(c.g1)) {  // not filtered: its zero record goes on to the next iteration
    out[p] = c.rec;
    return;
  }
#endif
  c.lum = lum3(c.rec.x, c.rec.y, c.rec.z);
  {  // 3 x 3 filter (1 2 1) x (1 2 1) / 16 of the variance, taps outside the image skipped and the weights renormalised
    float gv = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
#if ATROUS_TILES
        if ((dx != 0 || dy != 0) && !dn_valid(S ? t_g1[lc + dy * LW + dx] : guides[2 * ((size_t)qy * W + qx) + 1])) continue;
#endif
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
#if ATROUS_TILES
        if (!dn_valid(t_g1[k])) continue;
#endif
        tap(c, D, h, t_rec[k], t_g0[k], t_g1[k], a);
      } else {
        const size_t q = (size_t)qy * W + qx;
#if ATROUS_TILES
        const float4 q1 = guides[2 * q + 1];  // (the record the tap reads anyway)
        if (!dn_valid(q1)) continue;
        tap(c, D, h, rec[q], guides[2 * q], q1, a);
#else
        tap(c, D, h, rec[q], guides[2 * q], guides[2 * q + 1], a);
#endif
      }
    }
  }
  const float iw = 1.0f / a.w;  // the centre tap alone weighs 9 / 64
  out[p] = make_float4(a.r * iw, a.g * iw, a.b * iw, a.v * (iw * iw));
}
#undef ATROUS_PASS_KERNEL
#endif

#undef ATROUS_PREPARE_KERNEL
#undef ATROUS_TILE_ORIGIN
#undef ATROUS_REC_AT
#undef ATROUS_G0_AT
#undef ATROUS_G1_AT
#undef ATROUS_VAR_AT
#undef ATROUS_PACKED
