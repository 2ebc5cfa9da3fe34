// kernels.h -- host-visible launch wrappers of kernels.hip
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../../include/rene_hip.h"
#include "device_scene.h"
#include "kernel_select.h"

namespace rene {

constexpr uint32_t RENE_FLAG_INTERNAL_TEST_DROP = 1u << 29;  // RenderParams.flags, set by rene_render under RENE_TEST_DROP=<launch>: some items of that
                                                             // launch are dropped as if their hand-off had timed out (tests of the replay)
// tests: under RENE_TEST_KERNEL_LOG=<path> (read at every launch, like RENE_NO_LDS_TABLES) each render launch appends the mangled name of the
// kernel it launches to <path>, one line per launch, in the form of the `Function Name:` entries of <unit>.res (tests/kernel_matrix.py
// restates the selection; the log checks that restatement against it).  Called by launch_render (rene_hip.cpp).
void log_render_launch(const void* kernel, hipStream_t st);

struct LaunchConfig {
  uint32_t features = 0;     // FEAT_* of the scene
  uint32_t stack_depth = 16; // LDS traversal stack entries per lane
  uint32_t grid = 0;         // workgroups of the persistent render launch (upper bound)
  uint32_t cus = 0;          // compute units of the device
  uint32_t wave_stack = 0;   // wavefront integrator: LDS traversal stack entries per lane (exact tree depth)
  uint32_t n_insts = 0;      // instances of the scene (the restart kernels keep a small table of them in LDS)
};

// workgroups of the calling thread's most recent persistent render launch after fit_grid's clamp (rene_hip.cpp)
extern thread_local uint32_t g_launched_blocks;
hipError_t launch_render(const LaunchConfig& cfg, const SceneView& S, const RenderParams& P, hipStream_t st);
// what launch_render launches for this scene under these RENE_FLAG_* (kernel_select.h; RENE_NO_LDS_TABLES is read here, at every call), and the
// instantiation of a choice in the unit that holds its family -- kernels_bvh.hip: path integrator, BVH; kernels_vol.hip: volpath -- or null
using RenderKernel = void (*)(SceneView, RenderParams);
int render_block_size();
inline KernelChoice select_kernel(const LaunchConfig& cfg, const SceneView& S, uint32_t flags) {
  return select_kernel(SelectInputs{cfg.features, flags, S.main.n_nodes, cfg.stack_depth, cfg.n_insts, S.lights_len, S.small_bytes, (uint32_t)render_block_size(),
                                    std::getenv("RENE_NO_LDS_TABLES") != nullptr});
}
RenderKernel bvh_render_kernel(const KernelChoice& k);
RenderKernel vol_render_kernel(const KernelChoice& k);
// stage-separated wavefront integrator (wavefront.inc, kernels_wave.hip): path state in HBM, SoA
struct WaveState {
  float4* ro;        // xyz ray origin
  float4* rd;        // xyz ray direction
  float4* color;     // rgb throughput; w = BSDF pdf awaiting the emitter-pdf ray
  uint4* ctl;        // x rng state, y frame-wide rng state, z depth, w next frame of this slot
  float4* hit;       // t, u, v, bits(slot)
  float4* sh_wi;     // [max_lights][n_slots] shadow ray direction (xyz)
  float4* sh_c;      // [max_lights][n_slots] contribution if unoccluded (rgb)
  uint32_t* status;  // WS_* bits
  uint32_t* n_done;  // slots that have finished all their frames
  uint32_t* trace_counter;  // [2] next ray id of the closest-hit / secondary traversal pass
  unsigned long long* wave_sums;  // [waves][8] per-wave counter rows (folded into the context's counters at the end)
  uint32_t n_slots;
  uint32_t max_lights;
  uint32_t fp16_payload;  // RENE_FLAG_FP16_PAYLOAD: direction and throughput of a slot as six halves in ONE float4 (Q.rd), Q.color unused
  uint32_t pad_;
};
hipError_t launch_wave_init(const WaveState& Q, hipStream_t st);
hipError_t launch_wave_finish(const RenderParams& P, const WaveState& Q, hipStream_t st);
hipError_t launch_wave_rounds(const LaunchConfig& cfg, const SceneView& S, const RenderParams& P, const WaveState& Q,
                              uint32_t rounds, hipStream_t st);
hipError_t launch_trace(const LaunchConfig& cfg, const SceneView& S, int which, uint32_t n, const float* o,
                        const float* d, float tmin, float tmax, rene_hit* out, hipStream_t st);
hipError_t launch_bsdf_eval(const SceneView& S, uint32_t material, int inst_index, uint32_t n, const float* nrm3, const float* uv,
                            const float* wo3, const float* wi3, const uint32_t* seeds, float* out, hipStream_t st);
hipError_t launch_medium_eval(const SceneView& S, uint32_t medium, uint32_t n, const float* rd3, const float* t_max,
                              const float* wo3, const float* wi3, const uint32_t* seeds, float* out, hipStream_t st);
hipError_t launch_transmittance(const LaunchConfig& cfg, const SceneView& S, bool emit, uint32_t medium, uint32_t n, const float* o, const float* d,
                                float* out4, hipStream_t st);
hipError_t launch_emitter_pdf(const LaunchConfig& cfg, const SceneView& S, uint32_t n, const float* o, const float* d, float* out, hipStream_t st);
// FEAT_SMALL contexts only (the LDS image): the item loop + emitter_pdf_lds, and emit_sample / emit_sample_lds per seed
hipError_t launch_emitter_pdf_lds(const SceneView& S, bool normalised, uint32_t n, const float* o, const float* d, float* out, hipStream_t st);
hipError_t launch_emit_sample(const SceneView& S, bool lds, uint32_t n, const uint32_t* seeds, float* out8, hipStream_t st);
hipError_t launch_pcg_probe(uint32_t seed, uint32_t n, uint32_t* out, hipStream_t st);
// the frame-wide sample stream as a per-launch table (device_scene.h, FRAME_STREAM_*): where the kernel launch_render picks reads
// RenderParams::frame_stream (KernelChoice::reads_frame_stream) rene_render provides [n_frames][FRAME_STREAM_STRIDE][4] floats and launch_render
// fills them on the stream before it launches; the fill on its own (rene_frame_stream_probe)
hipError_t launch_frame_stream_fill(const SceneView& S, uint32_t seed_state0, uint32_t first_frame, uint32_t frame_stride, uint32_t n_frames,
                                    float* table, hipStream_t st);
// tile-sharded exchange: the 32x32 tiles with index % shard_count == shard_rank of a [3][H][W][4] image <-> a packed
// buffer [owned tile][layer][32][32][4] (out-of-image texels of edge tiles are zero / skipped)
hipError_t launch_pack_tiles(const float* fb, float* packed, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t n_tiles,
                             uint32_t shard_rank, uint32_t shard_count, bool unpack, hipStream_t st);
// rene_trace_queue (probe: the J1 gate): a traversal-only persistent pass over a queue-ordered SoA ray buffer
struct TraceQueue {
  const float* o_tmax;      // [n][4] origin, tmax
  const uint32_t* d_flags;  // [n][2] direction as three halves + flags in the fourth (bit 0: any-hit, bit 1: emitter-only structure) -- or,
                            // fp32 payload, [n][4] direction as three floats + flags
  float* hits;              // [n][4] t (-1: miss), u, v, bits(slot)
  uint32_t* counter;        // next ray of the queue (zeroed by the host)
  uint32_t n;
  uint32_t refill_min;      // dead lanes a wave gathers before it fetches rays for them (64: only when the whole wave is done)
  uint32_t leaf_min;        // lanes at a leaf before the leaf step runs
  uint32_t fp16;            // direction payload: 1 = three halves (8 bytes), 0 = three floats (16 bytes)
  uint32_t stack_entries;
  uint32_t passes;          // the queue is traversed this many times over in one launch (>= 1)
};
// rene_trace_queue (probe, kernels_gate.hip): a traversal-only persistent pass over a queue-ordered ray buffer; step_counters (optional): 5 x u64
hipError_t launch_trace_queue(const LaunchConfig& cfg, const SceneView& S, const TraceQueue& Q, uint32_t blocks_per_cu, unsigned long long* step_counters, hipStream_t st);
// frame chains: the owned tiles of out[3][H][W][4] = the CHAINS [3][n_slots][4] blocks of `chains` added in chain order (alpha 0); the chains are left as they are
hipError_t launch_resolve_chains(const float* chains, float* out, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t n_slots, uint32_t shard_rank,
                                 uint32_t shard_count, hipStream_t st);
// the passes over the frame chains (chain_pass.h): the geometry every one of them is launched with, and the chain counts two of them take
struct TileGrid {
  uint32_t width, height, tiles_x, n_slots;
  uint32_t shard_rank, shard_count;  // owned tile k is image tile shard_rank + k * shard_count (0, 1: every tile)
};
struct ChainCounts {
  uint32_t chain_n[CHAINS];  // n_c, the frames every chain has received
  // owned tiles that differ in their frame counts (adaptive sampling): [n_sets][CHAINS] chain counts and the set of every owned tile; both null: chain_n holds for every tile
  const uint32_t* sets;
  const uint32_t* tile_set;
};
// the `atrous` denoiser (kernels_denoise.hip, rene_denoise and its kin): what its prepare, pass and finalize kernels are launched with
struct DenoiseLaunch {
  TileGrid grid;                 // (an unsharded context: 0, 1)
  uint32_t step;                 // the pass's tap spacing, 2^iteration
  uint32_t tile_columns;         // order of the passes' 32 x 8 tiles over the workgroups: 0 = row-major; n = an eighth of the tiles per XCD, in super-columns n tiles wide
  float n_frames, inv_n;         // N = frames accumulated, 1 / N
  float inv_km1;                 // 1 / (k - 1), k = chains that have received frames
  float chain_share[CHAINS];     // n_c / N (0: the chain has no frames)
  float chain_inv[CHAINS];       // 1 / n_c
  float sigma_l, inv_sigma_n2, inv_sigma_a2, albedo_floor, relative_floor;
};
// the noise estimate (kernels_noise.hip, rene_estimate_noise): what its kernel is launched with
struct NoiseLaunch {
  TileGrid grid;
  float inv_n;                       // 1 / N, N = frames accumulated
  float inv_km1;                     // 1 / (k - 1), k = chains that have received frames
  float chain_share[CHAINS];         // n_c / N (0: the chain has no frames)
  float chain_inv[CHAINS];           // 1 / n_c
  // owned tiles that differ in their frame counts (adaptive sampling): [n_sets][NOISE_SET_FLOATS] sets of the four constants above, in that order, and
  // the set of every owned tile (NOISE_SET_NONE: not estimated, a zero record); both null: the constants above hold for every tile
  const float* sets;
  const uint32_t* tile_set;
};
constexpr uint32_t NOISE_SET_FLOATS = 2u + 2u * CHAINS, NOISE_SET_NONE = 0xffffffffu;
// the denoiser tile by tile (rene_denoise_tiles): the constants of every distinct N_t as a noise set followed by (float)N_t, and the set of every
// owned tile (NOISE_SET_NONE: an invalid tile, masked out of the filter) -- always a table, one set on an even context.  Both null: the constants of
// the DenoiseLaunch hold for every tile (rene_denoise)
constexpr uint32_t DENOISE_SET_FLOATS = NOISE_SET_FLOATS + 1u;
struct DenoiseTileSets {
  const float* sets;
  const uint32_t* tile_set;
};
// the trimmed prepare (rene_denoise_robust, rene_denoise_tiles_robust): steps R1 - R4 in a unit of their own, built with the flags of the robust
// resolve (kernels_denoise_trim.hip), and a prepare that reads what they decided, built with the denoiser's flags (kernels_denoise.hip).
// Between the two: one word per pixel of the image, trim [H][W] = j | kept << 8 (bit g of kept: chain g is kept; a pixel of an invalid tile: 0).
// The tile-by-tile table grows by the chain counts themselves: a DENOISE_SET_FLOATS set followed by the bits of the CHAINS n_c (uint32).
constexpr uint32_t DENOISE_ROBUST_SET_FLOATS = DENOISE_SET_FLOATS + CHAINS;
struct DenoiseTrimLaunch {
  TileGrid grid;
  uint32_t max_trim;
  float gain;
  uint32_t chain_n[CHAINS];  // n_c of the whole image; tile_set != null: every owned tile's from its set
  const float* sets;         // [n_sets][DENOISE_ROBUST_SET_FLOATS]
  const uint32_t* tile_set;  // NOISE_SET_NONE: an invalid tile, j = 0
};
hipError_t launch_denoise_trim(const float* chains, uint32_t* trim, const DenoiseTrimLaunch& L, hipStream_t st);
struct DenoiseTrimmed {
  const uint32_t* trim;      // null: the plain prepare
  uint32_t chain_n[CHAINS];  // n_c of the whole image (with tile sets: every tile's from its DENOISE_ROBUST_SET_FLOATS set)
};
// the denoiser on tile shards (rene_denoise_shard_prepare / rene_denoise_place_shard): the records of the tile-by-tile prepare, tile-packed.  The
// body of a packed buffer holds, for every owned tile k in owned order, one block of DN_PACKED_TILE_F4 16-byte records:
// rec [1024] (slot order), guides [1024][2], var [1024] floats -- 52 bytes per slot, every part 16-byte aligned.
constexpr uint32_t DN_PACKED_GUIDES_F4 = TILE_SLOTS, DN_PACKED_VAR_F4 = 3u * TILE_SLOTS, DN_PACKED_TILE_F4 = DN_PACKED_VAR_F4 + TILE_SLOTS / 4u;
constexpr size_t DN_PACKED_TILE_BYTES = (size_t)DN_PACKED_TILE_F4 * 16u;
// what varies between the prepares
struct DenoisePrepare {
  float *rec, *guides, *var_plane;  // pixel-major rec [H][W][4] (demodulated colour, variance of the mean), guides [H][W][2][4], var_plane [H][W] -- or
  void* body;                       // (with sets, untrimmed) a packed body of n_slots / 1024 blocks, the owned slots of D.grid; slots outside the image: zero records
  DenoiseTileSets sets;             // not null: the second guide carries {valid, (float)N_t} in .z and .w; D's n_frames, inv_n, inv_km1, chain_share, chain_inv are not read
  DenoiseTrimmed trimmed;           // trim not null: steps 2 and 3 over the chains `trim` keeps; where j == 0 the same records bit for bit
};
// chains [CHAINS][3][n_slots][4] + the resolved image [3][H][W][4] -> the records of A
hipError_t launch_denoise_prepare(const float* chains, const float* image, const DenoisePrepare& A, const DenoiseLaunch& D, hipStream_t st);
// one a-trous iteration rec -> out (step D.step; steps up to stage_max through the LDS-staged kernel, 1 / 2 / 4 exist); masked: the records of a prepare with sets
hipError_t launch_atrous_pass(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, bool masked, int stage_max, hipStream_t st);
hipError_t launch_denoise_finalize(const float* rec, const float* guides, float* out, const DenoiseLaunch& D, bool masked, hipStream_t st);
int denoise_stage_max();
// RENE_DENOISED_MEAN: out [H][W][4] = col * den of the filtered records; masked: an invalid pixel's unfiltered SUM, which the host divides by its tile's N_t
hipError_t launch_denoise_mean(const float* rec, const float* guides, float* out, uint32_t width, uint32_t height, float albedo_floor, bool masked, hipStream_t st);
// the n_owned blocks of `body` -- the tiles shard_rank + k * shard_count of G -- scattered into pixel-major rec [H][W][4], guides [H][W][2][4] and
// var_plane [H][W] of the whole image (G.n_slots is not read); slots outside the image are skipped
hipError_t launch_denoise_shard_place(const void* body, uint32_t n_owned, float* rec, float* guides, float* var_plane, const TileGrid& G, hipStream_t st);
// chains [CHAINS][3][n_slots][4] -> tiles [n_slots / 1024][4]: per owned tile {sum of the variance of the mean, sum of the luminance, bits(pixels inside the image), 0}
hipError_t launch_noise_tiles(const float* chains, float* tiles, const NoiseLaunch& L, hipStream_t st);
// rene_download_mean (kernels_mean.hip): out[H][W][4] = layer [H][W][4] of the resolved image, every texel divided by the frame count of its 32 x 32
// tile (tile_frames [tiles_y * tiles_x] on the image's full grid; 0 frames: 0) -- an IEEE fp32 division
hipError_t launch_tile_mean(const float* layer, float* out, const uint32_t* tile_frames, uint32_t width, uint32_t height, uint32_t tiles_x, hipStream_t st);
// the firefly-robust resolve (kernels_robust.hip, rene_resolve_robust): what its kernel is launched with
struct RobustLaunch {
  TileGrid grid;
  uint32_t max_trim;
  float gain;
  ChainCounts counts;
};
// chains [CHAINS][3][n_slots][4] -> out [H][W][4]: per owned pixel inside the image {robust mean rgb, (float)j}; tiles [n_slots / 1024][4]: per owned tile
// {sum of lum(plain mean), sum of lum(robust mean), bits(pixels inside the image), bits(pixels with j > 0)}
hipError_t launch_robust_tiles(const float* chains, float* out, float* tiles, const RobustLaunch& L, hipStream_t st);
// the denoiser hand-off (kernels_features.hip, rene_export_features): what its kernel is launched with
struct FeatureLaunch {
  TileGrid grid;
  uint32_t features, channels;  // RENE_FEATURE_* mask and the channels it selects (rene_feature_channels)
  ChainCounts counts;
};
// chains [CHAINS][3][n_slots][4] + the resolved image [3][H][W][4] -> dst, a tightly packed [C][H][W] (RENE_FEATURES_CHW) or [H][W][C] tensor of fp32 or
// fp16 elements (RENE_FEATURES_F32 / _F16): the channels of L.features in bit order, for the owned pixels inside the image; nothing else is written
hipError_t launch_features(const float* chains, const float* image, void* dst, int format, int layout, const FeatureLaunch& L, hipStream_t st);
// the output transform (kernels_output.hip, rene_output_8bit): what its kernel is launched with
struct OutputLaunch {
  const float* layer;            // [H][W][4] sums (or means, with a divisor of 1)
  void* dst;                     // [H][W][3] or [H][W][4] bytes, 4-byte aligned
  const uint32_t* tile_frames;   // [n_tiles] the divisor of every tile on the image's full grid (0: the tile's pixels are 0)
  const float* thresholds;       // RENE_OUTPUT_SRGB: rene_output_thresholds' 255 floats on the device
  uint32_t width, height, tiles_x, n_tiles;
  uint32_t shard_rank, shard_count;  // only the pixels of the tiles with index % shard_count == shard_rank are written (0, 1: every tile)
  uint32_t shard_inv;                // floor(2^32 / shard_count) where shard_count > 1: the kernel's modulus by multiplication
};
// layer -> dst: transform RENE_OUTPUT_SRGB / _AOV / _AOV_NORMAL of every pixel's mean, format RENE_OUTPUT_RGB8 / _RGBA8 (alpha 255)
hipError_t launch_output(const OutputLaunch& L, int transform, int format, hipStream_t st);
// rene_output_probe: out[i] = the byte of v[i] by the kernel's own per-channel function (device pointers)
hipError_t launch_output_probe(int transform, size_t n, const float* v, uint8_t* out, const float* thresholds, hipStream_t st);
// the tone-mapped output transform (kernels_tonemap.hip, rene_output_tonemapped): the output kernel's launch (sRGB: `thresholds` is set) and the
// operator's two numbers
struct TonemapLaunch {
  OutputLaunch out;
  float scale;  // the exposure's factor
  float w2;     // RENE_TONEMAP_REINHARD: white * white, rounded to fp32 on the host
};
// op RENE_TONEMAP_CLAMP / _REINHARD / _ACES, format RENE_OUTPUT_RGB8 / _RGBA8
hipError_t launch_tonemap(const TonemapLaunch& L, int op, int format, hipStream_t st);
// rene_tonemap_probe: out[3 i ..] = the bytes of the mean rgb[3 i ..] by the kernel's own per-pixel function (device pointers)
hipError_t launch_tonemap_probe(int op, float scale, float w2, size_t n, const float* rgb, uint8_t* out, const float* thresholds, hipStream_t st);
// the luminance histogram (kernels_luminance.hip, rene_luminance_histogram)
constexpr uint32_t LUM_BINS = 256, LUM_ROW = LUM_BINS + 1, LUM_BLOCK = 256;
struct LuminanceLaunch {
  const float* layer;           // [H][W][4] sums (or means, with a divisor of 1)
  const uint32_t* tile_frames;  // [n_tiles] the divisor of every tile on the image's full grid (0: the tile's pixels are 0, and dark)
  uint32_t* rows;               // [groups][LUM_ROW] scratch: every workgroup's 256 counts and its dark count
  uint32_t* out;                // [LUM_ROW] the sum of the rows
  uint32_t width, height, tiles_x, n_tiles;
  uint32_t shard_rank, shard_count, shard_inv;  // as in OutputLaunch
  uint32_t groups;                              // workgroups of the counting launch, sized to the chip; any number >= 1 gives the same counts
};
hipError_t launch_luminance(const LuminanceLaunch& L, hipStream_t st);
// the checkpoint (kernels_state.hip, rene_save_state / rene_restore_state): one chunk of owned tiles between the chains and a chunk buffer that holds
// the state format's payload, STATE_TILE_DWORDS dwords per tile -- [CHAINS][3][32 dy][32 dx][3], row-major, without the version words
constexpr uint32_t STATE_TILE_DWORDS = RENE_STATE_TILE_BYTES / 4u;
static_assert(STATE_TILE_DWORDS == CHAINS * 3u * TILE_SLOTS * 3u, "the payload of a tile: every record's three floats");
struct StateLaunch {
  TileGrid grid;
  uint32_t first_owned, n_tiles;  // the chunk: owned tiles first_owned .. first_owned + n_tiles - 1; tile i of the chunk is block i of the chunk buffer
};
// pack: chains -> chunk; unpack: chunk -> chains (records with version 0, zero outside the image); both: sums [owned tile] = {c0, c1} of the payload
hipError_t launch_state(float* chains, void* chunk, void* sums, const StateLaunch& L, bool unpack, hipStream_t st);
// the geometry pass (kernels_gbuffer.hip, rene_gbuffer / rene_primary_hits): what its kernels are launched with
struct GbufferLaunch {
  TileGrid grid;
  const uint32_t* seeds;  // [n_frames] the frames' seeds on the device (rene_frame_seeds)
  uint32_t n_frames;
  uint32_t id_source;     // RENE_GBUFFER_ID_*
  void* dst;              // rene_gbuffer_pixel [H][W], or (samples) rene_primary_hit [n_frames][H][W]; 16-byte aligned, zeroed by the host
};
// one lane per owned pixel slot; `samples`: the per-sample probe instead of the records
hipError_t launch_gbuffer(const LaunchConfig& cfg, const SceneView& S, const GbufferLaunch& L, bool samples, hipStream_t st);
// the occlusion pass (kernels_occlusion.hip, rene_occlusion / rene_occlusion_samples): what its kernels are launched with
struct OcclusionLaunch {
  TileGrid grid;
  const uint32_t* seeds;  // [n_frames] the frames' seeds on the device (rene_frame_seeds)
  uint32_t n_frames;
  uint32_t rays;          // occlusion rays per hitting sample, 1 .. RENE_OCCLUSION_MAX_RAYS
  float radius;           // their tmax
  void* dst;              // rene_occlusion_pixel [H][W], or (samples) rene_occlusion_sample [n_frames][rays][H][W]; 16-byte aligned, zeroed by the host
};
// one lane per owned pixel slot; `samples`: the per-sample probe instead of the records
hipError_t launch_occlusion(const LaunchConfig& cfg, const SceneView& S, const OcclusionLaunch& L, bool samples, hipStream_t st);
// the direct-light pass (kernels_direct.hip, rene_direct / rene_direct_samples): what its kernels are launched with
struct DirectLaunch {
  TileGrid grid;
  const uint32_t* seeds;  // [n_frames] the frames' seeds on the device (rene_frame_seeds)
  uint32_t n_frames;
  uint32_t background;    // the scene has a background that is not black (FEAT_BACKGROUND): a miss adds its colour
  void* dst;              // rene_direct_pixel [H][W], or (samples) rene_direct_sample [n_frames][H][W]; 16-byte aligned, zeroed by the host
};
// one lane per owned pixel slot; `samples`: the per-sample probe instead of the records
hipError_t launch_direct(const LaunchConfig& cfg, const SceneView& S, const DirectLaunch& L, bool samples, hipStream_t st);
// the bounce pass (kernels_bounces.hip, rene_bounces / rene_bounces_samples): what its kernels are launched with
struct BouncesLaunch {
  TileGrid grid;
  const uint32_t* seeds;  // [n_frames] the frames' seeds on the device (rene_frame_seeds)
  uint32_t n_frames;
  uint32_t background;    // the scene has a background that is not black (FEAT_BACKGROUND): a miss adds its colour
  uint32_t max_depth;     // the cap on a path's iterations, 1 .. RENE_BOUNCES_MAX_DEPTH
  void* dst;              // rene_bounces_pixel [H][W], or (samples) rene_bounces_sample [n_frames][H][W]; 16-byte aligned, zeroed by the host
};
// one lane per owned pixel slot; `samples`: the per-sample probe instead of the records
hipError_t launch_bounces(const LaunchConfig& cfg, const SceneView& S, const BouncesLaunch& L, bool samples, hipStream_t st);
// the light-group pass (kernels_lights.hip, rene_lights / rene_lights_samples): what its kernels are launched with
struct LightsLaunch {
  TileGrid grid;
  const uint32_t* seeds;  // [n_frames] the frames' seeds on the device (rene_frame_seeds)
  uint32_t n_frames;
  uint32_t background;    // the scene has a background that is not black (FEAT_BACKGROUND): a miss adds its colour
  const uint8_t* instance_group;  // [instances of the scene] on the device, every entry below RENE_LIGHTS_GROUPS: the group of an instance's own emission
  const uint8_t* distant_group;   // [S.lights_len] likewise: the group of a distant light
  uint32_t background_group;      // the group of the miss add, below RENE_LIGHTS_GROUPS
  void* dst;              // rene_lights_pixel [H][W], or (samples) rene_lights_sample [n_frames][H][W]; 16-byte aligned, zeroed by the host
};
// one lane per owned pixel slot; `samples`: the per-sample probe instead of the records
hipError_t launch_lights(const LaunchConfig& cfg, const SceneView& S, const LightsLaunch& L, bool samples, hipStream_t st);
// the multi-channel OpenEXR body (kernels_exr.hip, rene_output_exr): what its kernel is launched with.  A source that no chosen layer reads may be null.
struct ExrLaunch {
  const float* beauty;            // [H][W][4] sums (or means, with divisors of 1): R G B
  const float* albedo;            // [H][W][4] the resolved image's layer 2
  const float* normal;            // [H][W][4] the resolved image's layer 1
  const float* denoised;          // [H][W][4] RENE_DENOISED_MEAN as launch_denoise_mean leaves it
  const uint32_t* beauty_frames;  // [n_tiles] the divisor of every tile on the image's full grid for `beauty` (0: the tile's pixels are 0)
  const uint32_t* image_frames;   // ... for `albedo` and `normal`: N_t
  const uint32_t* denoised_frames;  // ... for `denoised`
  const rene_gbuffer_pixel* records;  // [H][W] the geometry pass's records
  void* dst;                      // the body, height x (8 + width x bytes_per_pixel) bytes, 4-byte aligned
  uint32_t width, height, tiles_x, n_tiles;
  uint32_t shard_rank, shard_count;  // only the bytes of the pixels of the tiles with index % shard_count == shard_rank are written (0, 1: every tile)
  uint32_t shard_inv;                // as in OutputLaunch
  uint32_t layers;                   // RENE_EXR_* mask
  uint32_t bytes_per_pixel;          // of that mask (rene_exr_layout)
};
hipError_t launch_exr(const ExrLaunch& L, hipStream_t st);
// the ZIPS chunks of a compressed OpenEXR file (kernels_exr_zips.hip, rene_exr_compress): an uncompressed body in, the file's tail out
struct ZipsLaunch {
  const uint8_t* body;          // height chunks of 8 + row_bytes bytes, 4-byte aligned
  uint8_t* tail;                // the offset table (height uint64), then the chunks back to back; 8-byte aligned, 8 * height + the body's bytes at least
  uint32_t* sizes;              // [height] scratch: every chunk's size (row_bytes: stored raw)
  unsigned long long* written;  // the tail's length in bytes
  unsigned long long attr_bytes;  // what the table's offsets count in front of the tail
  uint32_t height, row_bytes;   // row_bytes: width x bytes per pixel, even, at most 16384 x 66
};
hipError_t launch_exr_zips_size(const ZipsLaunch& L, hipStream_t st);
hipError_t launch_exr_zips_scan(const ZipsLaunch& L, hipStream_t st);    // (after the size kernel, on its stream)
hipError_t launch_exr_zips_encode(const ZipsLaunch& L, hipStream_t st);  // (after the scan)
// the body of a Cryptomatte file (kernels_cryptomatte.hip, rene_output_cryptomatte): up to three layers' geometry records and name-hash tables in,
// the scan-line chunks of an uncompressed file of 8 FLOAT channels per layer out
constexpr uint32_t CRYPTOMATTE_LAYERS = RENE_CRYPTOMATTE_MAX_LAYERS;
struct CryptomatteLaunch {
  const rene_gbuffer_pixel* records[CRYPTOMATTE_LAYERS];  // [H][W] per layer
  const uint32_t* hashes[CRYPTOMATTE_LAYERS];             // [n_names[l]] rene_cryptomatte_hash of the name of id i
  uint32_t n_names[CRYPTOMATTE_LAYERS];
  // where a layer's channels lie in the chunk, as the index of the channel row (the rows are in the order of the channel names' bytes):
  // [l][0 .. 3] the level 00's A B G R, [l][4 .. 7] the level 01's
  uint8_t row_index[CRYPTOMATTE_LAYERS][8];
  void* dst;                         // the body, height x (8 + width x 32 x n_layers) bytes, 4-byte aligned
  uint32_t width, height, tiles_x;
  uint32_t shard_rank, shard_count;  // as in ExrLaunch
  uint32_t shard_inv;
  uint32_t n_layers;                 // 1 .. CRYPTOMATTE_LAYERS
};
hipError_t launch_cryptomatte(const CryptomatteLaunch& L, hipStream_t st);
// the body of a pass-layer file (kernels_exr_passes.hip, rene_output_exr_passes): the records of the occlusion, direct-light, bounce and light-group
// passes and the radiance sums in, the scan-line chunks of an uncompressed file of HALF channels out.  A source that no chosen layer reads may be null.
struct ExrPassesLaunch {
  const rene_occlusion_pixel* occlusion;  // [H][W]: AO, BENT
  const rene_direct_pixel* direct;        // [H][W]: DIRECT, INDIRECT
  const rene_bounces_pixel* bounces;      // [H][W]: BOUNCES, LENGTH
  const rene_lights_pixel* lights;        // [H][W]: LIGHTS
  const float* beauty;                    // [H][W][4] the radiance layer's sums: INDIRECT
  void* dst;                              // the body, height x (8 + width x bytes_per_pixel) bytes, 4-byte aligned
  uint32_t width, height, tiles_x;
  uint32_t shard_rank, shard_count;       // as in ExrLaunch
  uint32_t shard_inv;
  uint32_t layers;                        // RENE_EXRP_* mask
  uint32_t groups;                        // the light groups LIGHTS writes, a non-empty mask of 8 bits (0 without LIGHTS)
  uint32_t bytes_per_pixel;               // of the two masks (rene_exr_passes_layout), 2 .. 130
};
hipError_t launch_exr_passes(const ExrPassesLaunch& L, hipStream_t st);

}  // namespace rene
