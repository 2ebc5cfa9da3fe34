// rene_cli.cpp -- `rene-hip`: rene's command line (rene/src/main.rs:47-207, 1613-1687) over the C ABI.
//
//   rene-hip <scene.pbrt> [--aov-normal PATH] [--aov-albedo PATH] [--denoiser none|optix|oidn|atrous]
//            [--dump-module PATH]                       <- the reference's five options (main.rs:54-71)
//            [--spp N] [--seed S] [--width W] [--height H] [--gpus G] [--batch B] [--out PATH] [--frame-groups]
//            [--target-noise T] [--noise-map PATH] [--adaptive] [--dilate D] [--sample-map PATH]
//            [--robust] [--robust-gain G] [--robust-max-trim M] [--trim-map PATH] [--features PREFIX]
//            [--reject-fireflies] [--reject-gain G] [--reject-max-trim M]
//            [--tonemap clamp|reinhard|aces] [--exposure EV|auto] [--white W]
//            [--checkpoint FILE] [--resume FILE]
//            [--gbuffer PREFIX] [--gbuffer-frames N] [--gbuffer-id instance|material|primitive]
//            [--exr PATH] [--exr-layers beauty,albedo,normal,denoised,alpha,depth,position,ids] [--exr-compression none|zips]
//            [--cryptomatte PATH] [--cryptomatte-layers object,material] [--cryptomatte-frames N]
//            [--exr-passes PATH] [--exr-pass-layers ao,bent,direct,indirect,bounces,length,lights] [--exr-light-names N0,N1,...]
//            [--ao PREFIX] [--ao-radius R] [--ao-rays K] [--ao-frames N]
//            [--direct PREFIX] [--direct-frames N]
//            [--bounces PREFIX] [--bounces-frames N] [--bounces-max-depth D]
//            [--lights PREFIX] [--lights-frames N] [--lights-mix W0,W1,...]
//
// The reference hard-codes 5000 samples in batches of 100 (main.rs:80-81); --spp / --batch default
// to those.  Output name = Film "filename" (+ ".png" when it ends in ".exr", main.rs:1651-1656).
// --gpus G renders on G devices from this one process: one context per device, 32x32 tiles dealt
// round-robin, the per-device images summed on the host (each pixel has exactly one owner).
// --denoiser atrous (build-defined; optix / oidn are accepted and ignored as in a reference build without them): the radiance written
// is the device's a-trous filter of the job (rene_denoise, include/rene_hip.h); one GPU only -- a gathered image has no frame chains.
// --target-noise T (build-defined): render until the image's noise figure (rene_estimate_noise, include/rene_hip.h) is at most T; --spp becomes
// the cap and --batch, rounded up to a multiple of 8, the first batch.  After every batch the noise is estimated; the next batch is half of
// what the 1 / sqrt(N) law says is missing (one render's prediction scatters), at least --batch, a multiple of 8.  The image is bit for bit
// that of a fixed --spp N run for the N it stopped at.  With --gpus G every tile shard is estimated and the estimates are combined.
// --noise-map PATH: an 8-bit grey PNG of one pixel per 32 x 32 tile, 255 min(1, tile noise / scale), scale = T or else the worst tile's noise.
// --adaptive (build-defined, with --target-noise T): the target is met per 32 x 32 TILE, and a tile that has met it stops rendering
// (rene_set_active_tiles, include/rene_hip.h).  After every batch the tile figures pick the tiles that go on (rene_noise_select_tiles: above T, or
// within --dilate D tiles, default 1, of one that is); the quietest of them sets the next batch by the schedule above.  The image written is the
// mean, every pixel over its own tile's frames (rene_download_mean).  One GPU, no --denoiser atrous (the filter takes one frame count).
// --sample-map PATH: an 8-bit grey PNG of one pixel per tile, 255 N_t / max N_t -- where the job's frames went.
// --robust (build-defined): the radiance written is the firefly-robust mean (rene_resolve_robust, include/rene_hip.h: a trimmed mean over the eight
// frame chains; biased dark, which the INFO line it prints quantifies as the energy kept), with --robust-gain G (default 1) and --robust-max-trim M
// (0 .. 3, default 3).  Works with --target-noise and --adaptive (the noise figures still describe the plain mean) and with --gpus G: every tile shard
// is resolved before the exchange, the shards' tiles meet on the host and their summaries are combined.  Not with --denoiser atrous: the filter
// reads the chains, not this image.  --trim-map PATH (implies the resolve): an 8-bit grey PNG of the image's size, 85 j per pixel.
// --reject-fireflies (build-defined, with --denoiser atrous or atrous-tiles): the filter is prepared from the chains that do not stand out
// (rene_denoise_robust / rene_denoise_tiles_robust, include/rene_hip.h), for scenes whose noise is fireflies; --reject-gain G (default 0.35, the
// filter's own) and --reject-max-trim M (0 .. 3, default 3).  The INFO line gives the share of pixels that left chains out.
// Not with --gpus G: the library denoises tile shards with the plain filter only (rene_denoise_shard_prepare .. rene_denoise_placed), and this
// command line does not drive those calls yet.
// --features PREFIX (build-defined): the denoiser hand-off as files (rene_export_features, include/rene_hip.h) -- after the job PREFIX.color.pfm,
// .albedo.pfm, .normal.pfm, .half_a.pfm and .half_b.pfm (`PF`, three channels) and PREFIX.variance.pfm and .frames.pfm (`Pf`, one), all of them
// MEANS in fp32, little-endian (scale -1), bottom row first: what `oidnDenoise --hdr / --alb / --nrm` takes.  Works with --target-noise, --adaptive
// (every pixel over its own tile's frames; .frames.pfm is the sample map per pixel) and --robust (the features describe the plain mean).  One GPU:
// exporting the shards before the gather is not offered.
// --tonemap OP, --exposure EV|auto, --white W (build-defined): the radiance written by --out goes through an exposure factor and a tone curve
// ahead of its sRGB byte (rene_output_tonemapped, include/rene_hip.h) -- clamp (the default: exposure only), reinhard (extended, on the luminance,
// white point W, default 4) or aces (Narkowicz's fit).  EV is rounded to eighth-stops; `auto` takes it from the image's luminance histogram
// (rene_luminance_histogram, rene_auto_exposure_e8) and prints it on an INFO line.  The AOV files are not tone-mapped.  On one GPU the device
// does it; under RENE_HOST_OUTPUT=1 and with --gpus G the host functions rene_tonemap_rgb8 / rene_luminance_histogram_host do, to the same bytes.
// Without these options the image is what it always was.
// --checkpoint FILE, --resume FILE (build-defined): the job's state -- its frame chains and bookkeeping, rene_save_state_file / rene_restore_state_files,
// include/rene_hip.h -- is written to FILE after every batch and at the end (to FILE.tmp, then renamed: FILE is whole or absent); --resume FILE
// restores it into the fresh context and renders the frames that are missing up to --spp.  The frames are bit for bit the ones the job would have
// rendered had it gone on, so for a job of a fixed sample count the image is that of the uninterrupted job whatever the two --spp were:
// `--spp 8 --checkpoint f` then `--spp 16 --resume f` writes the bytes of `--spp 16`.  The scene, --seed, --width and --height must be those of
// the job that was saved.  Works with --batch, --target-noise and --adaptive -- the active tiles and every tile's frame count come from the file.
// Under --target-noise / --adaptive the image also depends on WHEN the job looked at its noise, which the state does not record: a job that was
// killed and is resumed with the SAME --spp, --batch and target repeats the estimate (and the tiles' selection, idempotent on the saved set) its
// last checkpoint followed and goes on through the batches the uninterrupted job would have rendered -- the same bytes.  A job that ended at its
// own, smaller --spp cut its last batch short there; resumed with a larger --spp it is judged at that frame count, where the uninterrupted job
// would not have looked: a valid job of the same target, but not the same bytes unless no tile changes state there (a job resumed inside its
// first batch completes that batch before any tile is judged, so nothing differs then).  Works with every output and denoiser option.  One GPU: a state restores on any tile-shard layout through the library, which this command line does not drive.
// --gbuffer PREFIX (build-defined): the geometry pass as files (rene_gbuffer, include/rene_hip.h) -- after the job PREFIX.depth.pfm (`Pf`, the mean
// depth of the hitting samples, 0 where nothing hit), PREFIX.coverage.pfm (`Pf`, hits / n), PREFIX.position.pfm (`PF`, the mean world position, 0
// where nothing hit) and PREFIX.id.png, over the primary rays of frames 0 .. N - 1, N = --gbuffer-frames (default min(--spp, 16)); the ids are
// the instances, or with --gbuffer-id the materials or the primitives.  One GPU: with --gpus G the shards' records would have to be merged
// (rene_gbuffer on every shard, api.gbuffer_merge), which this command line does not drive.
// --exr PATH (build-defined): after the job, the layers of --exr-layers (default beauty,albedo,normal) as ONE scan-line OpenEXR file, uncompressed,
// HALF / FLOAT / UINT channels (rene_write_exr, include/rene_hip.h): beauty (R G B: the job's mean radiance, with --robust the robust mean), albedo,
// normal, denoised (the filtered mean; needs --denoiser atrous or atrous-tiles), and from the geometry pass alpha (A), depth (Z), position (P.X .Y .Z)
// and ids (id0 .. id3, cov0 .. cov3) -- the pass runs over the frames --gbuffer would take (--gbuffer-frames, --gbuffer-id).  The file's body is packed
// on the device and only its bytes come back.  --exr-compression zips (default none): every scan line deflated on the device into a ZIPS chunk
// (rene_write_exr_compressed), a smaller file that every reader inflates.  One GPU.  --out x.exr is not this option: it keeps the reference's INFO line and its PNG.
// --cryptomatte PATH (build-defined): after the job, the id mattes BY NAME as a Cryptomatte OpenEXR file (rene_write_cryptomatte, include/rene_hip.h),
// the format Nuke, Fusion, Blender and Natron read: the layers of --cryptomatte-layers (default object,material: CryptoObject over the instances,
// CryptoMaterial over the materials), named as the scene names them (ObjectInstance and MakeNamedMaterial names, else object_<i> / material_<i>),
// from the geometry pass over frames 0 .. N - 1, N = --cryptomatte-frames (default min(--spp, 16)).  --exr-compression applies to this file too.
// One GPU.  The pass runs once per layer; the second layer's records live in a second context of the same scene and seed, which exists for that
// call alone (this program holds no device memory of its own).
// --exr-passes PATH (build-defined): after the job, the pass layers as ONE OpenEXR file of HALF channels (rene_write_exr_passes, include/rene_hip.h):
// ao, bent.*, depth0.* .. depth9.*, direct.*, indirect.*, light0.* .. light7.* and pathlength, of the layers of --exr-pass-layers (default: those
// whose passes the command line asks for with --ao, --direct, --bounces and --lights; without any of them, all).  The passes the layers need run
// over the job's own frames -- a uniform job's 0 .. spp - 1 -- with --ao-radius, --ao-rays, --bounces-max-depth and the library's light grouping,
// into the library's buffers, behind the .pfm files of those options.  --exr-light-names N0,N1,... names the light groups in the file's
// rene/lightGroups attribute (an empty entry: no name).  --exr-compression applies to this file too.  One GPU; `indirect` is beauty - direct over
// the same samples, which an --adaptive job's tiles do not have: refused.
// --ao PREFIX (build-defined): the occlusion pass as files (rene_occlusion, include/rene_hip.h) -- after the job PREFIX.ao.pfm (`Pf`, 1 - occluded /
// rays, 1 where no ray was cast), PREFIX.bent.pfm (`PF`, the normalised sum of the unoccluded directions, 0 where there is none) and PREFIX.ao.png
// (grey, floor(255 ao + 0.5)), over the primary rays of frames 0 .. N - 1, N = --ao-frames (default min(--spp, 16)), with --ao-rays K rays per
// hitting sample (1 .. 64, default 1) that end after --ao-radius R world units (default 1).  One GPU, like --gbuffer: through the library,
// rene_occlusion on every tile shard and api.occlusion_merge join the shards' records.
// --direct PREFIX (build-defined): the direct-light pass as files (rene_direct, include/rene_hip.h) -- after the job PREFIX.direct.pfm (`PF`, the
// direct light per sample, (seen + distant + sampled) / N) and PREFIX.direct.png (its sRGB bytes), over frames 0 .. N - 1, N = --direct-frames
// (default --spp, at most 65536).  Where the pass covers exactly the job's frames and the job is uniform -- one GPU, not --adaptive, not --resume --
// also PREFIX.indirect.pfm, (beauty sum - direct sum) / N: the indirect light of the same samples.  Otherwise an INFO line says why it is left out.
// --bounces PREFIX (build-defined): the bounce pass as files (rene_bounces, include/rene_hip.h) -- after the job PREFIX.depth0.pfm .. PREFIX.depth9.pfm
// (`PF`, what iteration d of the path loop added per sample, bucket[d].sum / N; depth9: every iteration from 9 on), PREFIX.length.pfm (`Pf`, the mean
// path length, length_sum / N) and PREFIX.length.png (grey: floor(255 length / the image's largest mean length + 0.5), black where that is 0), over
// frames 0 .. N - 1, N = --bounces-frames (default --spp, at most 65536).  --bounces-max-depth D (1 .. 50; default 0: rene's own 50) caps the paths
// of the PASS -- the job's own image is rene's, uncapped -- so depthD .. depth9 are black.  One GPU, like --direct.
// --lights PREFIX (build-defined): the light-group pass as files (rene_lights, include/rene_hip.h) under the library's own grouping
// (rene_lights_default_groups) -- after the job PREFIX.group<k>.pfm for the groups in use (`PF`, what the sources of group k added per sample,
// group[k].sum / N) and PREFIX.groups.txt, one line per group naming its sources ("group 1: distant 0", "group 2: instance 7"), over frames
// 0 .. N - 1, N = --lights-frames (default --spp, at most 65536).  --lights-mix W0,W1,... (at most eight factors; the groups behind the last
// one keep 1) also writes the relit mean image PREFIX.mix.pfm, (((W0 g0) + (W1 g1)) + ...) / N in fp32 (api.lights_mix), and PREFIX.mix.png (its
// sRGB bytes).  One GPU, like --direct.
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/rene_hip.h"

namespace {

// ---- minimal PNG writer: 8-bit RGB, zlib "stored" blocks (no compression library needed) -----------
uint32_t crc_table[256];
void crc_init() {
  for (uint32_t n = 0; n < 256; ++n) {
    uint32_t c = n;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
    crc_table[n] = c;
  }
}
uint32_t crc32(const uint8_t* p, size_t n, uint32_t c = 0xffffffffu) {
  for (size_t i = 0; i < n; ++i) c = crc_table[(c ^ p[i]) & 0xff] ^ (c >> 8);
  return c;
}
void be32(std::vector<uint8_t>& v, uint32_t x) {
  for (int s = 24; s >= 0; s -= 8) v.push_back((uint8_t)(x >> s));
}
void chunk(std::vector<uint8_t>& out, const char* type, const std::vector<uint8_t>& data) {
  be32(out, (uint32_t)data.size());
  std::vector<uint8_t> td(type, type + 4);
  td.insert(td.end(), data.begin(), data.end());
  out.insert(out.end(), td.begin(), td.end());
  be32(out, crc32(td.data(), td.size()) ^ 0xffffffffu);
}
// ch = 3: 8-bit RGB; ch = 1: 8-bit grey
bool write_png(const std::string& path, const uint8_t* rgb, uint32_t w, uint32_t h, uint32_t ch = 3) {
  crc_init();
  std::vector<uint8_t> raw;
  raw.reserve((size_t)h * (ch * w + 1));
  for (uint32_t y = 0; y < h; ++y) {
    raw.push_back(0);  // filter: none
    raw.insert(raw.end(), rgb + (size_t)y * w * ch, rgb + (size_t)(y + 1) * w * ch);
  }
  std::vector<uint8_t> z = {0x78, 0x01};
  size_t pos = 0;
  uint32_t a = 1, b = 0;
  for (uint8_t c : raw) {
    a = (a + c) % 65521u;
    b = (b + a) % 65521u;
  }
  while (pos < raw.size() || raw.empty()) {
    size_t n = std::min<size_t>(65535, raw.size() - pos);
    z.push_back(pos + n == raw.size() ? 1 : 0);
    z.push_back((uint8_t)(n & 0xff));
    z.push_back((uint8_t)(n >> 8));
    z.push_back((uint8_t)(~n & 0xff));
    z.push_back((uint8_t)((~n >> 8) & 0xff));
    z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
    pos += n;
    if (raw.empty()) break;
  }
  be32(z, (b << 16) | a);
  std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  std::vector<uint8_t> ihdr;
  be32(ihdr, w);
  be32(ihdr, h);
  const uint8_t tail[5] = {8, (uint8_t)(ch == 1 ? 0 : 2), 0, 0, 0};
  ihdr.insert(ihdr.end(), tail, tail + 5);
  chunk(out, "IHDR", ihdr);
  chunk(out, "IDAT", z);
  chunk(out, "IEND", {});
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
  std::fclose(f);
  return ok;
}

// PFM: "PF" (three channels, interleaved) or "Pf" (one), width and height, a negative scale for little-endian floats, then the rows BOTTOM FIRST.
// planes: `ch` planes of [h][w] floats, rows top first (a [C][H][W] feature tensor's).
bool write_pfm(const std::string& path, const float* planes, uint32_t w, uint32_t h, uint32_t ch) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  std::fprintf(f, "%s\n%u %u\n-1.0\n", ch == 3 ? "PF" : "Pf", w, h);
  std::vector<float> row((size_t)w * ch);
  bool ok = true;
  for (uint32_t y = h; y-- > 0 && ok;) {
    for (uint32_t x = 0; x < w; ++x)
      for (uint32_t c = 0; c < ch; ++c) row[(size_t)x * ch + c] = planes[((size_t)c * h + y) * w + x];
    ok = std::fwrite(row.data(), sizeof(float), row.size(), f) == row.size();
  }
  return std::fclose(f) == 0 && ok;
}

int die(const char* what) {
  std::fprintf(stderr, "\nrene-hip: %s: %s\n", what, rene_last_error());
  return 1;
}

void usage() {
  std::fprintf(stderr,
               "usage: rene-hip <pbrt file> [--aov-normal PATH] [--aov-albedo PATH] [--denoiser none|optix|oidn|atrous|atrous-tiles]\n"
               "                [--dump-module PATH] [--spp N] [--seed S] [--width W] [--height H] [--gpus G]\n"
               "                [--batch B] [--out PATH] [--frame-groups] [--target-noise T] [--noise-map PATH]\n"
               "                [--adaptive] [--dilate D] [--sample-map PATH] [--robust] [--robust-gain G]\n"
               "                [--robust-max-trim M] [--trim-map PATH] [--features PREFIX]\n"
               "                [--reject-fireflies] [--reject-gain G] [--reject-max-trim M]\n"
               "                [--tonemap clamp|reinhard|aces] [--exposure EV|auto] [--white W]\n"
               "                [--checkpoint FILE] [--resume FILE]\n"
               "                [--gbuffer PREFIX] [--gbuffer-frames N] [--gbuffer-id instance|material|primitive]\n"
               "                [--exr PATH] [--exr-layers beauty,albedo,normal,denoised,alpha,depth,position,ids] [--exr-compression none|zips]\n"
               "                [--cryptomatte PATH] [--cryptomatte-layers object,material] [--cryptomatte-frames N]\n"
               "                [--exr-passes PATH] [--exr-pass-layers ao,bent,direct,indirect,bounces,length,lights] [--exr-light-names N0,N1,...]\n"
               "                [--ao PREFIX] [--ao-radius R] [--ao-rays K] [--ao-frames N]\n"
               "                [--direct PREFIX] [--direct-frames N]\n"
               "                [--bounces PREFIX] [--bounces-frames N] [--bounces-max-depth D]\n"
               "                [--lights PREFIX] [--lights-frames N] [--lights-mix W0,W1,...]\n"
               "  --checkpoint FILE  write the job's state to FILE after every batch and at the end (one GPU)\n"
               "  --resume FILE      restore a state written by --checkpoint and render the frames missing up to --spp (same scene, seed and size)\n"
               "  --reject-fireflies  with --denoiser atrous|atrous-tiles, one GPU: prepare the filter from the frame chains that do not stand out\n"
               "  --denoiser atrous-tiles  the atrous filter tile by tile: also for an --adaptive job, whose tiles differ in their frame counts\n"
               "  --features PREFIX  after the job, write the denoiser hand-off (means, fp32 PFM, bottom row first):\n"
               "                     PREFIX.{color,albedo,normal,half_a,half_b}.pfm (PF) and PREFIX.{variance,frames}.pfm (Pf)\n"
               "  --gbuffer PREFIX   after the job, write the geometry pass over the primary rays of frames 0 .. N - 1 (one GPU):\n"
               "                     PREFIX.{depth,coverage}.pfm (Pf), PREFIX.position.pfm (PF) and PREFIX.id.png, the id mattes in false colours\n"
               "  --gbuffer-frames N  the frames of the pass (default min(--spp, 16)); --gbuffer-id: what an id is (default instance)\n"
               "  --exr PATH         after the job, write the layers of --exr-layers (default beauty,albedo,normal) as one multi-channel OpenEXR (one GPU);\n"
               "                     denoised needs --denoiser atrous|atrous-tiles; alpha, depth, position and ids run the geometry pass;\n"
               "                     beauty (R G B) is the job's mean radiance, with --robust the robust mean that --out shows\n"
               "  --exr-compression none|zips  zips: deflate every scan line of --exr's file on the device (ZIPS chunks); default none\n"
               "  --cryptomatte PATH  after the job, write the id mattes by name as a Cryptomatte OpenEXR (one GPU): --cryptomatte-layers object,material\n"
               "                     (default both), over frames 0 .. N - 1 of --cryptomatte-frames (default min(--spp, 16)); honours --exr-compression\n"
               "  --exr-passes PATH  after the job, write the pass layers as one OpenEXR file of HALF channels (one GPU): ao, bent, depth0 .. depth9, direct,\n"
               "                     indirect, light0 .. light7, pathlength -- the layers of --exr-pass-layers (default: those of --ao, --direct, --bounces and\n"
               "                     --lights where given, else all), their passes run over the job's own frames; --exr-light-names N0,N1,... names the light\n"
               "                     groups in the rene/lightGroups attribute; honours --ao-radius, --ao-rays, --bounces-max-depth and --exr-compression\n"
               "  --ao PREFIX        after the job, write the occlusion pass over the primary rays of frames 0 .. N - 1 (one GPU):\n"
               "                     PREFIX.ao.pfm (Pf), PREFIX.bent.pfm (PF, the bent normal) and PREFIX.ao.png (grey)\n"
               "  --ao-radius R      where the occlusion rays end, in world units (default 1); --ao-rays K: rays per hitting sample (1 .. 64, default 1);\n"
               "                     --ao-frames N: the frames of the pass (default min(--spp, 16))\n"
               "  --direct PREFIX    after the job, write the direct-light pass over frames 0 .. N - 1 (one GPU): PREFIX.direct.pfm (PF, per sample),\n"
               "                     PREFIX.direct.png and, where the pass covers exactly the frames of a uniform job, PREFIX.indirect.pfm (beauty - direct)\n"
               "  --direct-frames N  the frames of the pass (default --spp, at most 65536)\n"
               "  --bounces PREFIX   after the job, write the bounce pass over frames 0 .. N - 1 (one GPU): PREFIX.depth0.pfm .. PREFIX.depth9.pfm (PF, what\n"
               "                     iteration d of the path loop added per sample; depth9: every iteration from 9 on), PREFIX.length.pfm (Pf, the mean\n"
               "                     path length) and PREFIX.length.png (grey, scaled to the image's largest)\n"
               "  --bounces-frames N  the frames of the pass (default --spp, at most 65536); --bounces-max-depth D: cap the pass's paths at D\n"
               "                     iterations (1 .. 50; default 0: 50)\n"
               "  --lights PREFIX    after the job, write the light-group pass over frames 0 .. N - 1 (one GPU) under the library's grouping -- the\n"
               "                     background, every distant light, every emitting instance -- PREFIX.group<k>.pfm (PF, what group k's sources added\n"
               "                     per sample) for the groups in use and PREFIX.groups.txt (one line per group naming its sources)\n"
               "  --lights-frames N  the frames of the pass (default --spp, at most 65536); --lights-mix W0,W1,...: also PREFIX.mix.pfm and\n"
               "                     PREFIX.mix.png, the mean image with group k's light scaled by Wk (at most eight factors; the rest keep 1)\n");
}

// The false colour of an id in PREFIX.id.png: h = id * 0x9E3779B1; h ^= h >> 15; h *= 0x85EBCA6B; h ^= h >> 13 (uint32 arithmetic), channel c =
// 64 + 3 * ((h >> 8 c) & 255) / 4 -- 64 .. 255, so no id is black.  A pixel is the sum over its slots of colour * count / n, rounded to nearest:
// the background stays black and the edges are anti-aliased by the counts.
void id_colour(uint32_t id, float rgb[3]) {
  uint32_t h = id * 0x9E3779B1u;
  h ^= h >> 15;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  for (int c = 0; c < 3; ++c) rgb[c] = (float)(64u + 3u * ((h >> (8 * c)) & 255u) / 4u);
}

// What --gbuffer, --ao, --direct, --bounces and --lights refuse in the same words: more than one GPU (every shard holds the records of its tiles only), and a frame count
// above the pass's limit (max_frames 0: the option words that refusal itself).  `opt` names the option, `pass` the library's call.  true: refused
bool pass_option_refused(const char* opt, const char* pass, uint32_t gpus, uint32_t frames, uint32_t max_frames) {
  if (gpus > 1) {
    std::fprintf(stderr, "rene-hip: --%s cannot be combined with --gpus %u: the files are written from one unsharded context -- through the library, "
                         "rene_%s on every tile shard and api.%s_merge join the shards' records\n", opt, gpus, pass, pass);
    return true;
  }
  if (max_frames && frames > max_frames) {
    std::fprintf(stderr, "rene-hip: --%s-frames must be 1 .. %u\n", opt, max_frames);
    return true;
  }
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  auto t_start = std::chrono::steady_clock::now();
  std::string pbrt_path, aov_normal, aov_albedo, denoiser = "none", dump_module, out_override;
  uint32_t spp = 5000, batch = 100, seed = RENE_DEFAULT_SEED, width = 0, height = 0, gpus = 1;
  std::string noise_map, sample_map;
  bool adaptive = false;      // --adaptive: tiles that have met --target-noise stop rendering
  uint32_t dilate = 1;
  double target_noise = 0.0;  // --target-noise: 0 = render --spp frames
  bool have_target = false;
  bool robust = false;        // --robust: the image written is rene_resolve_robust's
  std::string trim_map;
  std::string features_prefix;  // --features: the feature tensor as PFM files
  rene_robust_params robust_params;
  rene_robust_params_default(&robust_params);
  bool reject = false;  // --reject-fireflies: the filter is rene_denoise_robust / rene_denoise_tiles_robust
  bool tonemapped = false, auto_exposure = false;  // --tonemap / --exposure / --white: --out goes through rene_output_tonemapped's arithmetic
  std::string tonemap = "clamp";
  double exposure_ev = 0.0;
  float white = 4.0f;
  rene_robust_params reject_params;
  rene_denoise_robust_params_default(&reject_params);
  std::string checkpoint_path, resume_path;  // --checkpoint / --resume: the job's state as a file
  std::string gbuffer_prefix, gbuffer_id = "instance";  // --gbuffer: the geometry pass as files
  uint32_t gbuffer_frames = 0;                          // (0: min(spp, 16))
  std::string exr_compression_name;                     // --exr-compression: none (default) or zips
  std::string exr_path, exr_layer_names;                // --exr: the job's layers as one OpenEXR file
  std::string cryptomatte_path, cryptomatte_layer_names = "object,material";  // --cryptomatte: the id mattes by name
  uint32_t cryptomatte_frames = 0;                      // (0: min(spp, 16))
  std::string exr_passes_path, exr_pass_layer_names, exr_light_names;  // --exr-passes: the pass layers as one OpenEXR file
  bool have_light_names = false;
  std::string ao_prefix;                                // --ao: the occlusion pass as files
  rene_occlusion_params ao_params;
  rene_occlusion_params_default(&ao_params);
  uint32_t ao_frames = 0;                               // (0: min(spp, 16))
  std::string direct_prefix;                            // --direct: the direct-light pass as files
  uint32_t direct_frames = 0;                           // (0: min(spp, 65536))
  std::string bounces_prefix;                           // --bounces: the bounce pass as files
  uint32_t bounces_frames = 0, bounces_max_depth = 0;   // (0: min(spp, 65536); 0: rene's own 50)
  std::string lights_prefix, lights_mix;                // --lights: the light-group pass as files; --lights-mix: the factors as given
  uint32_t lights_frames = 0;                           // (0: min(spp, 65536))
  float lights_weights[RENE_LIGHTS_GROUPS];
  bool frame_groups = false;  // --frame-groups (round 3's opt-in): accepted and ignored, every context renders eight frame chains per pixel (ABI v5)
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto val = [&](const char* name) -> const char* {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "rene-hip: %s needs a value\n", name);
        std::exit(2);
      }
      return argv[++i];
    };
    if (a == "--aov-normal") aov_normal = val("--aov-normal");
    else if (a == "--aov-albedo") aov_albedo = val("--aov-albedo");
    else if (a == "--denoiser") denoiser = val("--denoiser");
    else if (a == "--dump-module") dump_module = val("--dump-module");
    else if (a == "--spp") spp = (uint32_t)std::strtoul(val("--spp"), nullptr, 0);
    else if (a == "--batch") batch = (uint32_t)std::strtoul(val("--batch"), nullptr, 0);
    else if (a == "--seed") seed = (uint32_t)std::strtoul(val("--seed"), nullptr, 0);
    else if (a == "--width") width = (uint32_t)std::strtoul(val("--width"), nullptr, 0);
    else if (a == "--height") height = (uint32_t)std::strtoul(val("--height"), nullptr, 0);
    else if (a == "--gpus") gpus = (uint32_t)std::strtoul(val("--gpus"), nullptr, 0);
    else if (a == "--out") out_override = val("--out");
    else if (a == "--frame-groups") frame_groups = true;
    else if (a == "--target-noise") { target_noise = std::strtod(val("--target-noise"), nullptr); have_target = true; }
    else if (a == "--noise-map") noise_map = val("--noise-map");
    else if (a == "--adaptive") adaptive = true;
    else if (a == "--dilate") dilate = (uint32_t)std::strtoul(val("--dilate"), nullptr, 0);
    else if (a == "--sample-map") sample_map = val("--sample-map");
    else if (a == "--robust") robust = true;
    else if (a == "--robust-gain") robust_params.gain = std::strtof(val("--robust-gain"), nullptr);
    else if (a == "--robust-max-trim") robust_params.max_trim = (uint32_t)std::strtoul(val("--robust-max-trim"), nullptr, 0);
    else if (a == "--trim-map") trim_map = val("--trim-map");
    else if (a == "--reject-fireflies") reject = true;
    else if (a == "--reject-gain") { reject_params.gain = std::strtof(val("--reject-gain"), nullptr); reject = true; }
    else if (a == "--reject-max-trim") { reject_params.max_trim = (uint32_t)std::strtoul(val("--reject-max-trim"), nullptr, 0); reject = true; }
    else if (a == "--features") features_prefix = val("--features");
    else if (a == "--tonemap") { tonemap = val("--tonemap"); tonemapped = true; }
    else if (a == "--exposure") {
      const std::string e = val("--exposure");
      auto_exposure = e == "auto";
      if (!auto_exposure) exposure_ev = std::strtod(e.c_str(), nullptr);
      tonemapped = true;
    }
    else if (a == "--checkpoint") checkpoint_path = val("--checkpoint");
    else if (a == "--resume") resume_path = val("--resume");
    else if (a == "--gbuffer") gbuffer_prefix = val("--gbuffer");
    else if (a == "--gbuffer-frames") gbuffer_frames = (uint32_t)std::strtoul(val("--gbuffer-frames"), nullptr, 0);
    else if (a == "--gbuffer-id") gbuffer_id = val("--gbuffer-id");
    else if (a == "--exr") exr_path = val("--exr");
    else if (a == "--exr-layers") exr_layer_names = val("--exr-layers");
    else if (a == "--exr-compression") exr_compression_name = val("--exr-compression");
    else if (a == "--cryptomatte") cryptomatte_path = val("--cryptomatte");
    else if (a == "--cryptomatte-layers") cryptomatte_layer_names = val("--cryptomatte-layers");
    else if (a == "--cryptomatte-frames") cryptomatte_frames = (uint32_t)std::strtoul(val("--cryptomatte-frames"), nullptr, 0);
    else if (a == "--exr-passes") exr_passes_path = val("--exr-passes");
    else if (a == "--exr-pass-layers") exr_pass_layer_names = val("--exr-pass-layers");
    else if (a == "--exr-light-names") { exr_light_names = val("--exr-light-names"); have_light_names = true; }
    else if (a == "--ao") ao_prefix = val("--ao");
    else if (a == "--ao-radius") ao_params.radius = std::strtof(val("--ao-radius"), nullptr);
    else if (a == "--ao-rays") ao_params.rays = (uint32_t)std::strtoul(val("--ao-rays"), nullptr, 0);
    else if (a == "--ao-frames") ao_frames = (uint32_t)std::strtoul(val("--ao-frames"), nullptr, 0);
    else if (a == "--direct") direct_prefix = val("--direct");
    else if (a == "--direct-frames") direct_frames = (uint32_t)std::strtoul(val("--direct-frames"), nullptr, 0);
    else if (a == "--bounces") bounces_prefix = val("--bounces");
    else if (a == "--bounces-frames") bounces_frames = (uint32_t)std::strtoul(val("--bounces-frames"), nullptr, 0);
    else if (a == "--bounces-max-depth") bounces_max_depth = (uint32_t)std::strtoul(val("--bounces-max-depth"), nullptr, 0);
    else if (a == "--lights") lights_prefix = val("--lights");
    else if (a == "--lights-frames") lights_frames = (uint32_t)std::strtoul(val("--lights-frames"), nullptr, 0);
    else if (a == "--lights-mix") lights_mix = val("--lights-mix");
    else if (a == "--white") { white = std::strtof(val("--white"), nullptr); tonemapped = true; }
    else if (a == "-h" || a == "--help") { usage(); return 0; }
    else if (!a.empty() && a[0] == '-') { std::fprintf(stderr, "rene-hip: unknown option %s\n", a.c_str()); usage(); return 2; }
    else pbrt_path = a;
  }
  if (denoiser != "none" && denoiser != "optix" && denoiser != "oidn" && denoiser != "atrous" && denoiser != "atrous-tiles") {
    std::fprintf(stderr, "rene-hip: invalid --denoiser %s\n", denoiser.c_str());
    return 2;
  }
  const bool atrous_tiles = denoiser == "atrous-tiles";  // rene_denoise_tiles: every tile with its own frame count
  const bool atrous = denoiser == "atrous" || atrous_tiles;
  if (reject && atrous && gpus > 1) {  // the trimmed prepare's trim plane is not part of the records tile shards hand over
    std::fprintf(stderr, "rene-hip: --reject-fireflies cannot be combined with --gpus %u: the trimmed filter (rene_denoise_robust) is not offered for tile shards -- "
                         "only the plain filter is, through the library (rene_denoise_shard_prepare, rene_gather_denoise, rene_denoise_placed)\n", gpus);
    return 2;
  }
  if (atrous && gpus > 1) {  // the image gathered on GPU 0 has no frame chains to take the variance from
    std::fprintf(stderr, "rene-hip: --denoiser %s cannot be combined with --gpus %u: the filter runs on one unsharded context\n", denoiser.c_str(), gpus);
    return 2;
  }
  if ((!checkpoint_path.empty() || !resume_path.empty()) && gpus > 1) {
    std::fprintf(stderr, "rene-hip: --checkpoint and --resume cannot be combined with --gpus %u: the command line saves and restores one unsharded context\n", gpus);
    return 2;
  }
  if (adaptive && !have_target) {
    std::fprintf(stderr, "rene-hip: --adaptive needs --target-noise T: tiles stop when they have met it\n");
    return 2;
  }
  if (adaptive && gpus > 1) {
    std::fprintf(stderr, "rene-hip: --adaptive cannot be combined with --gpus %u: the adaptive job runs on one context\n", gpus);
    return 2;
  }
  if (adaptive && atrous && !atrous_tiles) {
    std::fprintf(stderr, "rene-hip: --adaptive cannot be combined with --denoiser atrous: the filter takes one frame count, the tiles of an adaptive job differ in theirs "
                         "(--denoiser atrous-tiles filters every tile with its own)\n");
    return 2;
  }
  if (robust && atrous) {
    std::fprintf(stderr, "rene-hip: --robust cannot be combined with --denoiser %s: the filter reads the frame chains, not the robust image "
                         "(--reject-fireflies rejects them inside the filter)\n", denoiser.c_str());
    return 2;
  }
  if (reject && !atrous) {
    std::fprintf(stderr, "rene-hip: --reject-fireflies needs --denoiser atrous or atrous-tiles: it is the filter's own firefly rejection (--robust is the one of the unfiltered image)\n");
    return 2;
  }
  if (reject_params.max_trim > 3 || !(reject_params.gain > 0.0f && std::isfinite(reject_params.gain))) {
    std::fprintf(stderr, "rene-hip: --reject-max-trim must be 0 .. 3 and --reject-gain a positive number\n");
    return 2;
  }
  if (robust_params.max_trim > 3 || !(robust_params.gain > 0.0f && std::isfinite(robust_params.gain))) {
    std::fprintf(stderr, "rene-hip: --robust-max-trim must be 0 .. 3 and --robust-gain a positive number\n");
    return 2;
  }
  const uint32_t tonemap_op = tonemap == "reinhard" ? RENE_TONEMAP_REINHARD : tonemap == "aces" ? RENE_TONEMAP_ACES : RENE_TONEMAP_CLAMP;
  if ((tonemap != "clamp" && tonemap_op == RENE_TONEMAP_CLAMP) || !std::isfinite(exposure_ev) || !std::isfinite(white) || !(white > 0.0f)) {
    std::fprintf(stderr, "rene-hip: --tonemap must be clamp, reinhard or aces, --exposure a number of EV or auto, --white a positive number\n");
    return 2;
  }
  const bool want_robust = robust || !trim_map.empty();
  if (!features_prefix.empty() && gpus > 1) {  // the gather consumes the chains, and exporting every shard before it is not offered
    std::fprintf(stderr, "rene-hip: --features cannot be combined with --gpus %u: the features are exported from one unsharded context\n", gpus);
    return 2;
  }
  const uint32_t gbuffer_source = gbuffer_id == "material" ? RENE_GBUFFER_ID_MATERIAL : gbuffer_id == "primitive" ? RENE_GBUFFER_ID_PRIMITIVE : RENE_GBUFFER_ID_INSTANCE;
  if (gbuffer_id != "instance" && gbuffer_source == RENE_GBUFFER_ID_INSTANCE) {
    std::fprintf(stderr, "rene-hip: --gbuffer-id must be instance, material or primitive\n");
    return 2;
  }
  if (!gbuffer_prefix.empty() && pass_option_refused("gbuffer", "gbuffer", gpus, gbuffer_frames, RENE_GBUFFER_MAX_FRAMES)) return 2;
  rene_exr_params exr_params;
  rene_exr_params_default(&exr_params);
  if (!exr_layer_names.empty()) {
    if (exr_path.empty()) {
      std::fprintf(stderr, "rene-hip: --exr-layers needs --exr PATH: the file the layers go into\n");
      return 2;
    }
    static const struct { const char* name; uint32_t bit; } kLayers[] = {
        {"beauty", RENE_EXR_BEAUTY}, {"albedo", RENE_EXR_ALBEDO}, {"normal", RENE_EXR_NORMAL}, {"denoised", RENE_EXR_DENOISED},
        {"alpha", RENE_EXR_ALPHA},   {"depth", RENE_EXR_DEPTH},   {"position", RENE_EXR_POSITION}, {"ids", RENE_EXR_IDS}};
    exr_params.layers = 0;
    for (size_t at = 0; at <= exr_layer_names.size();) {
      const size_t comma = std::min(exr_layer_names.find(',', at), exr_layer_names.size());
      const std::string name = exr_layer_names.substr(at, comma - at);
      uint32_t bit = 0;
      for (const auto& l : kLayers)
        if (name == l.name) bit = l.bit;
      if (!bit) {
        std::fprintf(stderr, "rene-hip: --exr-layers: unknown layer '%s' (beauty, albedo, normal, denoised, alpha, depth, position, ids)\n", name.c_str());
        return 2;
      }
      exr_params.layers |= bit;
      at = comma + 1;
    }
  }
  uint32_t exr_compression = RENE_EXR_COMPRESSION_NONE;
  if (!exr_compression_name.empty()) {
    if (exr_path.empty() && cryptomatte_path.empty() && exr_passes_path.empty()) {
      std::fprintf(stderr, "rene-hip: --exr-compression needs --exr PATH, --cryptomatte PATH or --exr-passes PATH: the file it compresses\n");
      return 2;
    }
    if (exr_compression_name == "zips") exr_compression = RENE_EXR_COMPRESSION_ZIPS;
    else if (exr_compression_name != "none") {
      std::fprintf(stderr, "rene-hip: --exr-compression: unknown compression '%s' (none, zips)\n", exr_compression_name.c_str());
      return 2;
    }
  }
  if (!exr_path.empty() && (exr_params.layers & RENE_EXR_DENOISED) && !atrous) {
    std::fprintf(stderr, "rene-hip: --exr-layers denoised needs --denoiser atrous or atrous-tiles: the layer is the filter's image\n");
    return 2;
  }
  if (!exr_path.empty() && gpus > 1) {  // every shard would pack the bytes of its tiles; merging them is the caller's, through the library
    std::fprintf(stderr, "rene-hip: --exr cannot be combined with --gpus %u: the file is written from one unsharded context\n", gpus);
    return 2;
  }
  std::vector<uint32_t> cryptomatte_sources;  // --cryptomatte-layers as RENE_GBUFFER_ID_*
  if (!cryptomatte_path.empty()) {
    if (gpus > 1) {
      std::fprintf(stderr, "rene-hip: --cryptomatte cannot be combined with --gpus %u: the file is written from one unsharded context\n", gpus);
      return 2;
    }
    if (cryptomatte_frames > RENE_GBUFFER_MAX_FRAMES) {
      std::fprintf(stderr, "rene-hip: --cryptomatte-frames must be 1 .. %u\n", RENE_GBUFFER_MAX_FRAMES);
      return 2;
    }
    for (size_t at = 0; at <= cryptomatte_layer_names.size();) {
      const size_t comma = std::min(cryptomatte_layer_names.find(',', at), cryptomatte_layer_names.size());
      const std::string name = cryptomatte_layer_names.substr(at, comma - at);
      const uint32_t source = name == "object" ? RENE_GBUFFER_ID_INSTANCE : RENE_GBUFFER_ID_MATERIAL;
      if ((name != "object" && name != "material") || std::count(cryptomatte_sources.begin(), cryptomatte_sources.end(), source)) {
        std::fprintf(stderr, "rene-hip: --cryptomatte-layers: '%s' is not one of object, material, each at most once\n", name.c_str());
        return 2;
      }
      cryptomatte_sources.push_back(source);
      at = comma + 1;
    }
  }
  // --exr-passes: the layer mask, the groups' names
  rene_exr_passes_params passes_params;
  rene_exr_passes_params_default(&passes_params);
  std::vector<std::string> light_names;
  const char* light_name_ptrs[RENE_LIGHTS_GROUPS] = {};
  if (exr_passes_path.empty() && (!exr_pass_layer_names.empty() || have_light_names)) {
    std::fprintf(stderr, "rene-hip: --exr-pass-layers and --exr-light-names need --exr-passes PATH: the file they describe\n");
    return 2;
  }
  if (!exr_passes_path.empty()) {
    if (gpus > 1) {
      std::fprintf(stderr, "rene-hip: --exr-passes cannot be combined with --gpus %u: the file is written from one unsharded context\n", gpus);
      return 2;
    }
    static const struct { const char* name; uint32_t bit; } kPassLayers[] = {{"ao", RENE_EXRP_AO}, {"bent", RENE_EXRP_BENT}, {"direct", RENE_EXRP_DIRECT},
                                                                              {"indirect", RENE_EXRP_INDIRECT}, {"bounces", RENE_EXRP_BOUNCES},
                                                                              {"length", RENE_EXRP_LENGTH}, {"lights", RENE_EXRP_LIGHTS}};
    uint32_t mask = 0;
    if (exr_pass_layer_names.empty()) {  // the layers of the passes the command line asks for, else all
      if (!ao_prefix.empty()) mask |= RENE_EXRP_AO | RENE_EXRP_BENT;
      if (!direct_prefix.empty()) mask |= RENE_EXRP_DIRECT | RENE_EXRP_INDIRECT;
      if (!bounces_prefix.empty()) mask |= RENE_EXRP_BOUNCES | RENE_EXRP_LENGTH;
      if (!lights_prefix.empty()) mask |= RENE_EXRP_LIGHTS;
      if (!mask) mask = RENE_EXRP_ALL;
    } else {
      for (size_t at = 0; at <= exr_pass_layer_names.size();) {
        const size_t comma = std::min(exr_pass_layer_names.find(',', at), exr_pass_layer_names.size());
        const std::string name = exr_pass_layer_names.substr(at, comma - at);
        uint32_t bit = 0;
        for (const auto& l : kPassLayers)
          if (name == l.name) bit = l.bit;
        if (!bit) {
          std::fprintf(stderr, "rene-hip: --exr-pass-layers: unknown layer '%s' (ao, bent, direct, indirect, bounces, length, lights)\n", name.c_str());
          return 2;
        }
        mask |= bit;
        at = comma + 1;
      }
    }
    if ((mask & RENE_EXRP_INDIRECT) && adaptive) {
      std::fprintf(stderr, "rene-hip: --exr-passes: the indirect layer is beauty - direct over the same samples, and an --adaptive job's tiles differ in their frame "
                           "counts; choose the layers without it (--exr-pass-layers)\n");
      return 2;
    }
    passes_params.layers = mask;
    if (have_light_names) {
      if (!(mask & RENE_EXRP_LIGHTS)) {
        std::fprintf(stderr, "rene-hip: --exr-light-names needs the lights layer\n");
        return 2;
      }
      for (size_t at = 0; at <= exr_light_names.size();) {
        const size_t comma = std::min(exr_light_names.find(',', at), exr_light_names.size());
        light_names.push_back(exr_light_names.substr(at, comma - at));
        at = comma + 1;
      }
      bool ok = light_names.size() <= RENE_LIGHTS_GROUPS;
      for (const std::string& n : light_names) {
        ok = ok && n.size() <= RENE_EXRP_MAX_NAME;
        for (const char ch : n) ok = ok && (std::isalnum((unsigned char)ch) || ch == '_' || ch == ' ' || ch == '-');
      }
      if (!ok) {
        std::fprintf(stderr, "rene-hip: --exr-light-names takes up to %u names N0,N1,..., each empty or 1 .. %u bytes of [A-Za-z0-9_ -]\n", RENE_LIGHTS_GROUPS,
                     RENE_EXRP_MAX_NAME);
        return 2;
      }
      for (size_t g = 0; g < light_names.size(); ++g)
        if (!light_names[g].empty()) light_name_ptrs[g] = light_names[g].c_str();
      passes_params.group_names = light_name_ptrs;
    }
  }
  const bool passes_ao = (passes_params.layers & (RENE_EXRP_AO | RENE_EXRP_BENT)) != 0 && !exr_passes_path.empty();
  const bool passes_bounces = (passes_params.layers & (RENE_EXRP_BOUNCES | RENE_EXRP_LENGTH)) != 0 && !exr_passes_path.empty();
  const bool exr_geometry = !exr_path.empty() && (exr_params.layers & (RENE_EXR_ALPHA | RENE_EXR_DEPTH | RENE_EXR_POSITION | RENE_EXR_IDS)) != 0;
  if (exr_geometry && gbuffer_frames > RENE_GBUFFER_MAX_FRAMES) {
    std::fprintf(stderr, "rene-hip: --gbuffer-frames must be 1 .. %u\n", RENE_GBUFFER_MAX_FRAMES);
    return 2;
  }
  if (!ao_prefix.empty() && pass_option_refused("ao", "occlusion", gpus, ao_frames, 0)) return 2;  // (its frames: with its rays and radius, below)
  if ((!ao_prefix.empty() || passes_ao) && (ao_frames > RENE_OCCLUSION_MAX_FRAMES || ao_params.rays < 1u || ao_params.rays > RENE_OCCLUSION_MAX_RAYS ||
                             !std::isfinite(ao_params.radius) || !(ao_params.radius > 0.001f) || !(ao_params.radius <= 100000.0f))) {
    std::fprintf(stderr, "rene-hip: --ao-frames must be 1 .. %u, --ao-rays 1 .. %u and --ao-radius a number above 0.001 and at most 100000\n",
                 RENE_OCCLUSION_MAX_FRAMES, RENE_OCCLUSION_MAX_RAYS);
    return 2;
  }
  if (!direct_prefix.empty() && pass_option_refused("direct", "direct", gpus, direct_frames, RENE_DIRECT_MAX_FRAMES)) return 2;
  if (!bounces_prefix.empty() && pass_option_refused("bounces", "bounces", gpus, bounces_frames, RENE_BOUNCES_MAX_FRAMES)) return 2;
  if ((!bounces_prefix.empty() || passes_bounces) && bounces_max_depth > RENE_BOUNCES_MAX_DEPTH) {
    std::fprintf(stderr, "rene-hip: --bounces-max-depth must be 1 .. %u, or 0 for %u\n", RENE_BOUNCES_MAX_DEPTH, RENE_BOUNCES_MAX_DEPTH);
    return 2;
  }
  if (!lights_prefix.empty() && pass_option_refused("lights", "lights", gpus, lights_frames, RENE_LIGHTS_MAX_FRAMES)) return 2;
  for (float& w : lights_weights) w = 1.0f;
  if (!lights_mix.empty()) {
    if (lights_prefix.empty()) {
      std::fprintf(stderr, "rene-hip: --lights-mix needs --lights PREFIX\n");
      return 2;
    }
    size_t k = 0;
    const char* at = lights_mix.c_str();
    for (bool more = true; more; ++k) {
      char* end = nullptr;
      const float w = std::strtof(at, &end);
      if (k >= RENE_LIGHTS_GROUPS || end == at || (*end != ',' && *end != 0)) {
        std::fprintf(stderr, "rene-hip: --lights-mix takes one to %u factors, W0,W1,...\n", RENE_LIGHTS_GROUPS);
        return 2;
      }
      lights_weights[k] = w;
      more = *end == ',';
      at = end + 1;
    }
  }
  if (robust) exr_params.beauty_source = RENE_OUTPUT_ROBUST;
  if (dilate > 2) {
    std::fprintf(stderr, "rene-hip: --dilate must be 0, 1 or 2\n");
    return 2;
  }
  if (denoiser != "none" && !atrous)  // main.rs:86-98: warn and ignore when not built in
    std::fprintf(stderr, "WARN %s denoiser was enabled but this build has no denoiser. Ignore.\n", denoiser.c_str());
  if (!dump_module.empty()) {  // main.rs:100-106 dumps the SPIR-V module; here: the gfx950 code object
    std::string self = argv[0];
    size_t slash = self.rfind('/');
    std::string co = (slash == std::string::npos ? std::string(".") : self.substr(0, slash)) + "/rene_kernels.co";
    FILE* in = std::fopen(co.c_str(), "rb");
    if (!in) { std::fprintf(stderr, "rene-hip: cannot open %s\n", co.c_str()); return 1; }
    FILE* o = std::fopen(dump_module.c_str(), "wb");
    if (!o) { std::fclose(in); std::fprintf(stderr, "rene-hip: cannot write %s\n", dump_module.c_str()); return 1; }
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, in)) > 0) std::fwrite(buf, 1, n, o);
    std::fclose(in);
    std::fclose(o);
    return 0;
  }
  if (pbrt_path.empty() || spp == 0 || batch == 0 || gpus == 0) { usage(); return 2; }
  if (have_target && !(target_noise > 0.0 && std::isfinite(target_noise))) {
    std::fprintf(stderr, "rene-hip: --target-noise needs a positive number\n");
    return 2;
  }
  const bool want_noise = have_target || !noise_map.empty();
  if (want_noise && spp < 2) {
    std::fprintf(stderr, "rene-hip: the noise estimate needs --spp 2 or more\n");
    return 2;
  }
  if (have_target) batch = std::max(16u, (batch + 7u) / 8u * 8u);  // every frame chain holds two frames or more at the first estimate

  rene_scene* scene = nullptr;
  if (rene_scene_load_pbrt(pbrt_path.c_str(), &scene) != RENE_OK) {
    std::printf("%s\n", rene_last_error());  // main.rs:199-205 prints the error and returns
    return 1;
  }
  rene_scene_desc desc = *rene_scene_get_desc(scene);
  if ((width && width != desc.xresolution) || (height && height != desc.yresolution)) {
    // additive override of the Film size: rescale the projection's x axis to the new aspect
    // (projection_inv = diag(aspect*tan, tan, ..), scene.rs:163-164)
    uint32_t nw = width ? width : desc.xresolution, nh = height ? height : desc.yresolution;
    float old_aspect = (float)desc.xresolution / (float)desc.yresolution, new_aspect = (float)nw / (float)nh;
    desc.uniform.projection_inv[0] *= new_aspect / old_aspect;
    desc.xresolution = nw;
    desc.yresolution = nh;
  }
  auto ms_since = [](std::chrono::steady_clock::time_point t) {
    return (long long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t).count();
  };
  std::fprintf(stderr, "INFO Scene parsed (%lld ms)\n", ms_since(t_start));

  auto t_load = std::chrono::steady_clock::now();
  std::vector<rene_ctx*> ctx(gpus, nullptr);
  for (uint32_t g = 0; g < gpus; ++g) {
    rene_opts o{};
    o.struct_size = sizeof(o);
    o.seed = seed;
    o.device = (int32_t)g;
    o.shard_mode = RENE_SHARD_TILES;
    o.shard_rank = g;
    o.shard_count = gpus;
    if (frame_groups) o.flags |= RENE_FLAG_FRAME_GROUPS;
    // all three layers are accumulated whether or not --aov-* asks for the files, like the reference's raygen
    // (lib.rs:229-232); RENE_FLAG_NO_AOV would save little and its Matte item-loop kernel happens to be the slower one
    if (std::getenv("RENE_DEBUG")) {  // what this context will hold on its device, before it allocates
      rene_memory_plan plan{};
      if (rene_plan_memory(&desc, &o, &plan) != RENE_OK) return die("rene_plan_memory");
      const double gb = 1e-9;
      std::fprintf(stderr, "INFO memory plan, device %u (tile shard %u of %u): chains %.3f GB, versions %.3f GB, image %.3f GB, scene %.3f GB, queues %.3f GB, total %.3f GB\n",
                   g, g, gpus, plan.chain_bytes * gb, plan.version_bytes * gb, plan.image_bytes * gb, plan.scene_bytes * gb, plan.queue_bytes * gb, plan.total_bytes * gb);
    }
    if (rene_create(&desc, &o, &ctx[g]) != RENE_OK) return die("rene_create");
  }
  std::fprintf(stderr, "INFO Scene loaded (%lld ms)\n", ms_since(t_load));

  // the job's noise estimate: every context's (tile shard's) estimate, combined
  rene_noise_estimate noise{};
  auto estimate = [&]() -> bool {
    std::vector<rene_noise_estimate> parts(gpus);
    for (uint32_t g = 0; g < gpus; ++g)
      if (rene_estimate_noise(ctx[g], nullptr, &parts[g]) != RENE_OK) return false;
    return rene_noise_combine(parts.data(), parts.size(), &noise) == RENE_OK;
  };
  const uint32_t tiles_x = (desc.xresolution + RENE_TILE_SIZE - 1u) / RENE_TILE_SIZE, tiles_y = (desc.yresolution + RENE_TILE_SIZE - 1u) / RENE_TILE_SIZE;
  // --adaptive: the tiles that go on after an estimate, and the frames the quietest of them still needs by the 1 / sqrt(N) law
  std::vector<uint8_t> active;
  uint32_t adaptive_needed = 0;
  auto select = [&](uint32_t done) -> int {  // 1: tiles go on, 0: none does, -1: error
    std::vector<rene_noise_tile> rec((size_t)tiles_x * tiles_y);
    if (rene_download_noise_tiles(ctx[0], rec.data(), rec.size()) != RENE_OK) return -1;
    std::vector<uint8_t> next(rec.size(), 0);
    if (rene_noise_select_tiles(rec.data(), active.empty() ? nullptr : active.data(), tiles_x, tiles_y, noise.luminance_floor, target_noise, dilate, next.data()) != RENE_OK) return -1;
    active = next;
    double least = -1.0;
    for (size_t t = 0; t < rec.size(); ++t) {
      if (!active[t]) continue;
      const double nt = (double)rec[t].n_pixels, m = (double)rec[t].sum_lum / nt + (double)noise.luminance_floor;
      const double need = std::ceil((double)done * (((double)rec[t].sum_var / nt) / (m * m)) / (target_noise * target_noise));
      if (least < 0.0 || need < least) least = need;
    }
    if (least < 0.0) return 0;
    adaptive_needed = least < 4294967295.0 ? (uint32_t)least : 0xffffffffu;
    return rene_set_active_tiles(ctx[0], active.data(), active.size()) == RENE_OK ? 1 : -1;
  };
  uint32_t sampled = 0;
  uint32_t frame_base = 0;  // the job's first frame: 0, or what the state of --resume says
  bool go_on = true;
  if (!resume_path.empty()) {  // the chains, the tiles' frame counts and their active flags come from the file
    const char* paths[1] = {resume_path.c_str()};
    if (rene_restore_state_files(ctx[0], nullptr, paths, 1) != RENE_OK) return die("rene_restore_state_files");
    rene_state_info sh{};  // what the file says of the job: read by the library's own parser
    sh.struct_size = sizeof(sh);
    if (rene_state_inspect_file(resume_path.c_str(), &sh, nullptr, 0) != RENE_OK) return die("rene_state_inspect_file");
    std::vector<rene_state_tile> table(sh.n_tiles);
    if (rene_state_inspect_file(resume_path.c_str(), &sh, table.data(), table.size()) != RENE_OK) return die("rene_state_inspect_file");
    if (sh.loaded) {
      std::fprintf(stderr, "rene-hip: %s holds chains put there by rene_load_chains, which nothing renders onto\n", resume_path.c_str());
      return 1;
    }
    sampled = sh.n_frames;
    frame_base = sh.frame_base;
    size_t n_active = 0;
    std::vector<uint8_t> from_file((size_t)tiles_x * tiles_y, 0);
    for (const rene_state_tile& t : table) {
      from_file[t.tile] = (t.flags & RENE_STATE_TILE_ACTIVE) ? 1 : 0;
      n_active += from_file[t.tile];
    }
    if (n_active != from_file.size()) active = from_file;  // (an adaptive job; a set may only shrink)
    std::fprintf(stderr, "INFO Resumed from %s: %u frames restored (frames %u .. %u), %zu of %zu tiles active\n", resume_path.c_str(), sampled, frame_base,
                 frame_base + sampled - 1u, n_active, from_file.size());
    if (!adaptive && n_active != from_file.size()) {
      std::fprintf(stderr, "rene-hip: %s is the state of an --adaptive job (tiles have stopped): resume it with --adaptive --target-noise T\n", resume_path.c_str());
      return 1;
    }
    if (have_target && sampled >= batch && sampled < spp) {  // what the job does after a batch, so that the next batch is the one it would have rendered
      if (!estimate()) return die("rene_estimate_noise");
      if (adaptive) {
        const int go = select(sampled);
        if (go < 0) return die("rene_set_active_tiles");
        go_on = go != 0;
      } else go_on = noise.noise > target_noise;
    } else if (have_target && sampled >= spp && !estimate()) return die("rene_estimate_noise");
  }
  bool unsaved = !checkpoint_path.empty();  // --checkpoint: frames (or a selection) the file does not hold yet
  auto save = [&]() -> bool {
    if (checkpoint_path.empty() || !unsaved || !sampled) return true;
    unsaved = false;
    return rene_save_state_file(ctx[0], nullptr, checkpoint_path.c_str()) == RENE_OK;
  };
  const auto t_render = std::chrono::steady_clock::now();
  while (go_on && sampled < spp) {  // main.rs:1315-1397
    uint32_t n = std::min(spp - sampled, batch);
    if (have_target && sampled && sampled < batch) n = std::min(spp, batch) - sampled;  // (resumed inside the first batch: it is completed before any tile is judged)
    else if (have_target && sampled) {  // half of what the estimate says is missing, at least a batch, a multiple of 8
      const uint32_t needed = adaptive ? adaptive_needed : rene_noise_frames_needed(&noise, target_noise);
      const uint32_t half = (std::max(needed, sampled) - sampled + 1u) / 2u;
      const uint32_t want = std::max(batch, half);
      n = std::min(spp - sampled, want > 0xfffffff8u ? want : (want + 7u) / 8u * 8u);
    }
    auto now = std::chrono::steady_clock::now();
    for (uint32_t g = 0; g < gpus; ++g)
      if (rene_render(ctx[g], frame_base + sampled, n) != RENE_OK) return die("rene_render");
    sampled += n;
    unsaved = !checkpoint_path.empty();
    // queue_wait_idle after every batch, main.rs:1389: the progress line then says what the batch took.  (A batch is one launch,
    // and a launch ends on the longest paths of its last work items: --batch N with N = --spp renders the job as ONE launch,
    // a few per cent faster than fifty batches of 100.)
    for (uint32_t g = 0; g < gpus; ++g)
      if (rene_sync(ctx[g]) != RENE_OK) return die("rene_sync");
    std::fprintf(stderr, "\rSamples: %u / %u (%lld ms)", sampled, spp, ms_since(now));
    if (have_target) {
      if (!estimate()) return die("rene_estimate_noise");
      if (adaptive) {
        if (sampled >= spp) break;  // (the cap: the tiles keep the set they rendered with)
        const int go = select(sampled);
        if (go < 0) return die("rene_set_active_tiles");
        if (go == 0) break;
      } else if (noise.noise <= target_noise) break;
    }
    if (!save()) return die("rene_save_state_file");  // after every batch: the frames and the tiles' selection so far
  }
  if (!save()) return die("rene_save_state_file");  // ... and at the end (the batches that ended the job left the loop before)
  std::fprintf(stderr, "\n");
  const double render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_render).count();

  if (!sample_map.empty()) {  // one grey pixel per tile: its frames over the most any tile received
    const size_t n_tiles = (size_t)tiles_x * tiles_y;
    std::vector<uint32_t> frames(n_tiles, 0u), part(n_tiles);
    for (uint32_t g = 0; g < gpus; ++g) {  // every tile has exactly one owner
      if (rene_tile_frames(ctx[g], part.data(), part.size()) != RENE_OK) return die("rene_tile_frames");
      for (size_t t = 0; t < n_tiles; ++t) frames[t] = std::max(frames[t], part[t]);
    }
    const uint32_t most = *std::max_element(frames.begin(), frames.end());
    std::vector<uint8_t> grey(n_tiles, 0);
    for (size_t t = 0; t < n_tiles; ++t) grey[t] = most ? (uint8_t)std::lround(255.0 * (double)frames[t] / (double)most) : 0;
    if (!write_png(sample_map, grey.data(), tiles_x, tiles_y, 1)) {
      std::fprintf(stderr, "rene-hip: cannot write %s\n", sample_map.c_str());
      return 1;
    }
  }
  if (want_noise) {  // before the exchange, which consumes the frame chains
    if (!have_target && !estimate()) return die("rene_estimate_noise");
    if (!noise_map.empty()) {
      const size_t n_tiles = (size_t)tiles_x * tiles_y;
      std::vector<rene_noise_tile> part(n_tiles);
      std::vector<uint8_t> grey(n_tiles, 0);
      const double scale = have_target ? target_noise : noise.worst_tile_noise;
      for (uint32_t g = 0; g < gpus; ++g) {  // every tile has exactly one owner
        if (rene_download_noise_tiles(ctx[g], part.data(), part.size()) != RENE_OK) return die("rene_download_noise_tiles");
        for (size_t t = 0; t < n_tiles; ++t) {
          if (!part[t].n_pixels) continue;
          const double nt = (double)part[t].n_pixels, m = (double)part[t].sum_lum / nt + (double)noise.luminance_floor;
          const double tn = std::sqrt(((double)part[t].sum_var / nt) / (m * m));
          grey[t] = (uint8_t)std::lround(255.0 * std::min(1.0, scale > 0.0 ? tn / scale : 0.0));
        }
      }
      if (!write_png(noise_map, grey.data(), tiles_x, tiles_y, 1)) {
        std::fprintf(stderr, "rene-hip: cannot write %s\n", noise_map.c_str());
        return 1;
      }
    }
  }
  // the robust resolve, before the exchange (which consumes the frame chains): every context resolves the tiles it owns and hands out zeros
  // elsewhere, so the shards' images and trim planes meet on the host by addition; the summaries are combined
  const size_t n_px = (size_t)desc.xresolution * desc.yresolution;
  // The output transform (average + to_rgb8 / to_aov, main.rs:1758-1810): on one GPU the 8-bit pixels come from the device (rene_output_8bit: the
  // same bytes, 3 per pixel over PCIe instead of 16 per layer); RENE_HOST_OUTPUT=1 keeps the host functions, as every multi-GPU job does
  const char* host_output = std::getenv("RENE_HOST_OUTPUT");
  const bool device_output = gpus == 1 && !(host_output && *host_output && std::strcmp(host_output, "0") != 0);
  std::vector<float> robust_img;
  rene_robust_summary robust_sum{};
  if (want_robust) {
    std::vector<rene_robust_summary> parts(gpus);
    std::vector<float> part, trim(trim_map.empty() ? 0 : n_px, 0.0f);
    robust_img.assign(n_px * 3, 0.0f);
    for (uint32_t g = 0; g < gpus; ++g) {
      if (rene_resolve_robust(ctx[g], &robust_params, &parts[g]) != RENE_OK) return die("rene_resolve_robust");
      if (gpus == 1) {
        if (!device_output && rene_download_robust(ctx[g], RENE_ROBUST_IMAGE, 3, robust_img.data(), robust_img.size()) != RENE_OK) return die("rene_download_robust");
        if (!trim.empty() && rene_download_robust(ctx[g], RENE_ROBUST_TRIM, 1, trim.data(), trim.size()) != RENE_OK) return die("rene_download_robust");
        continue;
      }
      part.resize(n_px * 3);
      if (rene_download_robust(ctx[g], RENE_ROBUST_IMAGE, 3, part.data(), part.size()) != RENE_OK) return die("rene_download_robust");
      for (size_t i = 0; i < robust_img.size(); ++i) robust_img[i] += part[i];
      if (trim.empty()) continue;
      if (rene_download_robust(ctx[g], RENE_ROBUST_TRIM, 1, part.data(), n_px) != RENE_OK) return die("rene_download_robust");
      for (size_t i = 0; i < n_px; ++i) trim[i] += part[i];
    }
    if (rene_robust_combine(parts.data(), parts.size(), &robust_sum) != RENE_OK) return die("rene_robust_combine");
    if (!trim_map.empty()) {
      std::vector<uint8_t> grey(n_px);
      for (size_t i = 0; i < n_px; ++i) grey[i] = (uint8_t)(85u * (uint32_t)trim[i]);
      if (!write_png(trim_map, grey.data(), desc.xresolution, desc.yresolution, 1)) {
        std::fprintf(stderr, "rene-hip: cannot write %s\n", trim_map.c_str());
        return 1;
      }
    }
    std::fprintf(stderr, "INFO robust resolve: kept energy %.4f, %.2f %% of the pixels trimmed (max_trim %u, gain %g, %llu frames)\n", robust_sum.kept_energy,
                 robust_sum.n_pixels ? 100.0 * (double)robust_sum.n_trimmed / (double)robust_sum.n_pixels : 0.0, robust_sum.max_trim, (double)robust_sum.gain,
                 (unsigned long long)robust_sum.n_frames);
  }
  // the denoiser hand-off as files: every feature as [C][H][W] fp32 from the library's own buffer, one PFM per feature
  if (!features_prefix.empty()) {
    static const struct { uint32_t bit; const char* name; } kFeatures[] = {
        {RENE_FEATURE_COLOR, "color"}, {RENE_FEATURE_ALBEDO, "albedo"}, {RENE_FEATURE_NORMAL, "normal"}, {RENE_FEATURE_VARIANCE, "variance"},
        {RENE_FEATURE_HALF_A, "half_a"}, {RENE_FEATURE_HALF_B, "half_b"}, {RENE_FEATURE_FRAMES, "frames"}};
    rene_feature_params fp;
    rene_feature_params_default(&fp);
    fp.features = 0;
    for (const auto& f : kFeatures) fp.features |= f.bit;
    fp.layout = RENE_FEATURES_CHW;
    std::vector<float> t((size_t)rene_feature_channels(fp.features) * n_px);
    if (rene_export_features(ctx[0], &fp, nullptr, 0) != RENE_OK) return die("rene_export_features");
    if (rene_download_features(ctx[0], t.data(), t.size() * sizeof(float)) != RENE_OK) return die("rene_download_features");
    size_t plane = 0;
    for (const auto& f : kFeatures) {
      const uint32_t ch = rene_feature_channels(f.bit);
      const std::string path = features_prefix + "." + f.name + ".pfm";
      if (!write_pfm(path, t.data() + plane * n_px, desc.xresolution, desc.yresolution, ch)) {
        std::fprintf(stderr, "rene-hip: cannot write %s\n", path.c_str());
        return 1;
      }
      plane += ch;
    }
  }
  // the geometry pass as files: the records from the library's own buffer, the means on the host
  rene_gbuffer_params gp;
  rene_gbuffer_params_default(&gp);
  gp.n_frames = gbuffer_frames ? gbuffer_frames : std::max(1u, std::min(spp, 16u));
  gp.id_source = gbuffer_source;
  // (the records stay in the library's buffer: --exr's geometry layers read them there)
  if ((!gbuffer_prefix.empty() || exr_geometry) && rene_gbuffer(ctx[0], &gp, nullptr, 0) != RENE_OK) return die("rene_gbuffer");
  if (!gbuffer_prefix.empty()) {
    std::vector<rene_gbuffer_pixel> rec(n_px);
    if (rene_download_gbuffer(ctx[0], rec.data(), rec.size() * sizeof(rene_gbuffer_pixel)) != RENE_OK) return die("rene_download_gbuffer");
    std::vector<float> depth(n_px, 0.0f), coverage(n_px, 0.0f), position(3 * n_px, 0.0f);
    std::vector<uint8_t> ids(3 * n_px, 0);
    for (size_t i = 0; i < n_px; ++i) {
      const rene_gbuffer_pixel& r = rec[i];
      if (r.n) coverage[i] = (float)r.hits / (float)r.n;
      if (r.hits) {
        depth[i] = r.depth_sum / (float)r.hits;
        for (size_t ch = 0; ch < 3; ++ch) position[ch * n_px + i] = r.position_sum[ch] / (float)r.hits;
      }
      float sum[3] = {0.0f, 0.0f, 0.0f};
      for (int k = 0; k < 4 && r.n; ++k) {
        if (!r.count[k]) continue;
        float rgb[3];
        id_colour(r.id[k], rgb);
        for (int ch = 0; ch < 3; ++ch) sum[ch] += rgb[ch] * ((float)r.count[k] / (float)r.n);
      }
      for (int ch = 0; ch < 3; ++ch) ids[3 * i + ch] = (uint8_t)std::min(255.0f, std::floor(sum[ch] + 0.5f));
    }
    const struct { const char* name; const float* data; uint32_t ch; } kPlanes[] = {{"depth", depth.data(), 1}, {"coverage", coverage.data(), 1}, {"position", position.data(), 3}};
    for (const auto& f : kPlanes) {
      const std::string path = gbuffer_prefix + "." + f.name + ".pfm";
      if (!write_pfm(path, f.data, desc.xresolution, desc.yresolution, f.ch)) {
        std::fprintf(stderr, "rene-hip: cannot write %s\n", path.c_str());
        return 1;
      }
    }
    if (!write_png(gbuffer_prefix + ".id.png", ids.data(), desc.xresolution, desc.yresolution)) {
      std::fprintf(stderr, "rene-hip: cannot write %s.id.png\n", gbuffer_prefix.c_str());
      return 1;
    }
  }
  // the occlusion pass as files: the records from the library's own buffer, the two figures on the host (api.occlusion_ao / occlusion_bent, in fp32)
  if (!ao_prefix.empty()) {
    ao_params.n_frames = ao_frames ? ao_frames : std::max(1u, std::min(spp, 16u));
    if (rene_occlusion(ctx[0], &ao_params, nullptr, 0) != RENE_OK) return die("rene_occlusion");
    std::vector<rene_occlusion_pixel> rec(n_px);
    if (rene_download_occlusion(ctx[0], rec.data(), rec.size() * sizeof(rene_occlusion_pixel)) != RENE_OK) return die("rene_download_occlusion");
    std::vector<float> ao(n_px, 1.0f), bent(3 * n_px, 0.0f);
    std::vector<uint8_t> grey(n_px, 0);
    for (size_t i = 0; i < n_px; ++i) {
      const rene_occlusion_pixel& r = rec[i];
      if (r.rays) ao[i] = 1.0f - (float)r.occluded / (float)r.rays;
      const float* b = r.bent_sum;
      const float len = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
      if (len > 0.0f)
        for (size_t ch = 0; ch < 3; ++ch) bent[ch * n_px + i] = b[ch] / len;
      grey[i] = (uint8_t)std::floor(255.0f * ao[i] + 0.5f);
    }
    const struct { const char* name; const float* data; uint32_t ch; } kPlanes[] = {{"ao", ao.data(), 1}, {"bent", bent.data(), 3}};
    for (const auto& f : kPlanes) {
      const std::string path = ao_prefix + "." + f.name + ".pfm";
      if (!write_pfm(path, f.data, desc.xresolution, desc.yresolution, f.ch)) {
        std::fprintf(stderr, "rene-hip: cannot write %s\n", path.c_str());
        return 1;
      }
    }
    if (!write_png(ao_prefix + ".ao.png", grey.data(), desc.xresolution, desc.yresolution, 1)) {
      std::fprintf(stderr, "rene-hip: cannot write %s.ao.png\n", ao_prefix.c_str());
      return 1;
    }
  }
  // the direct-light pass as files: the records from the library's own buffer, the figures on the host (api.direct_mean / indirect_mean, in fp32)
  if (!direct_prefix.empty()) {
    rene_direct_params dp;
    rene_direct_params_default(&dp);
    dp.n_frames = direct_frames ? direct_frames : std::max(1u, std::min(spp, RENE_DIRECT_MAX_FRAMES));
    if (rene_direct(ctx[0], &dp, nullptr, 0) != RENE_OK) return die("rene_direct");
    std::vector<rene_direct_pixel> rec(n_px);
    if (rene_download_direct(ctx[0], rec.data(), rec.size() * sizeof(rene_direct_pixel)) != RENE_OK) return die("rene_download_direct");
    const char* why = adaptive ? "an --adaptive job's tiles differ in their frame counts"
                      : !resume_path.empty() ? "a resumed job's frames are not the pass's"
                      : (frame_base != 0u || sampled != dp.n_frames) ? "the pass does not cover exactly the job's frames"
                                                                      : nullptr;
    std::vector<float> sum(3 * n_px, 0.0f), direct(3 * n_px, 0.0f), indirect(3 * n_px, 0.0f), beauty;
    if (!why) {
      beauty.assign(3 * n_px, 0.0f);
      if (rene_download(ctx[0], 0, 3, beauty.data(), beauty.size()) != RENE_OK) return die("rene_download");
    }
    for (size_t i = 0; i < n_px; ++i) {
      const rene_direct_pixel& r = rec[i];
      for (size_t ch = 0; ch < 3; ++ch) {
        const float s = (r.seen[ch] + r.distant[ch]) + r.sampled[ch];
        sum[3 * i + ch] = s;
        if (r.n) direct[ch * n_px + i] = s / (float)r.n;
        if (r.n && !why) indirect[ch * n_px + i] = (beauty[3 * i + ch] - s) / (float)r.n;
      }
    }
    if (!write_pfm(direct_prefix + ".direct.pfm", direct.data(), desc.xresolution, desc.yresolution, 3)) {
      std::fprintf(stderr, "rene-hip: cannot write %s.direct.pfm\n", direct_prefix.c_str());
      return 1;
    }
    std::vector<uint8_t> bytes(3 * n_px);
    rene_to_rgb8(sum.data(), sum.size(), dp.n_frames, bytes.data());
    if (!write_png(direct_prefix + ".direct.png", bytes.data(), desc.xresolution, desc.yresolution)) {
      std::fprintf(stderr, "rene-hip: cannot write %s.direct.png\n", direct_prefix.c_str());
      return 1;
    }
    if (why) {
      std::fprintf(stderr, "INFO direct-light pass over frames 0 .. %u: %s.indirect.pfm is not written (%s)\n", dp.n_frames - 1u, direct_prefix.c_str(), why);
    } else {
      if (!write_pfm(direct_prefix + ".indirect.pfm", indirect.data(), desc.xresolution, desc.yresolution, 3)) {
        std::fprintf(stderr, "rene-hip: cannot write %s.indirect.pfm\n", direct_prefix.c_str());
        return 1;
      }
      std::fprintf(stderr, "INFO direct-light pass over frames 0 .. %u, the job's own: %s.direct.pfm and %s.indirect.pfm (beauty - direct)\n", dp.n_frames - 1u,
                   direct_prefix.c_str(), direct_prefix.c_str());
    }
  }
  // the bounce pass as files: the records from the library's own buffer, the figures on the host (api.bounces_depth_mean / bounces_mean_length, in fp32)
  if (!bounces_prefix.empty()) {
    rene_bounces_params bp;
    rene_bounces_params_default(&bp);
    bp.n_frames = bounces_frames ? bounces_frames : std::max(1u, std::min(spp, RENE_BOUNCES_MAX_FRAMES));
    bp.max_depth = bounces_max_depth;
    if (rene_bounces(ctx[0], &bp, nullptr, 0) != RENE_OK) return die("rene_bounces");
    std::vector<rene_bounces_pixel> rec(n_px);
    if (rene_download_bounces(ctx[0], rec.data(), rec.size() * sizeof(rene_bounces_pixel)) != RENE_OK) return die("rene_download_bounces");
    std::vector<float> plane(3 * n_px), length(n_px, 0.0f);
    for (uint32_t d = 0; d < RENE_BOUNCES_BUCKETS; ++d) {
      std::fill(plane.begin(), plane.end(), 0.0f);
      for (size_t i = 0; i < n_px; ++i)
        for (size_t ch = 0; ch < 3 && rec[i].n; ++ch) plane[ch * n_px + i] = rec[i].bucket[d].sum[ch] / (float)rec[i].n;
      const std::string path = bounces_prefix + ".depth" + std::to_string(d) + ".pfm";
      if (!write_pfm(path, plane.data(), desc.xresolution, desc.yresolution, 3)) {
        std::fprintf(stderr, "rene-hip: cannot write %s\n", path.c_str());
        return 1;
      }
    }
    float longest = 0.0f;
    for (size_t i = 0; i < n_px; ++i) {
      if (rec[i].n) length[i] = (float)rec[i].length_sum / (float)rec[i].n;
      longest = std::max(longest, length[i]);
    }
    std::vector<uint8_t> grey(n_px, 0);
    for (size_t i = 0; i < n_px && longest > 0.0f; ++i) grey[i] = (uint8_t)std::floor(255.0f * (length[i] / longest) + 0.5f);
    if (!write_pfm(bounces_prefix + ".length.pfm", length.data(), desc.xresolution, desc.yresolution, 1)) {
      std::fprintf(stderr, "rene-hip: cannot write %s.length.pfm\n", bounces_prefix.c_str());
      return 1;
    }
    if (!write_png(bounces_prefix + ".length.png", grey.data(), desc.xresolution, desc.yresolution, 1)) {
      std::fprintf(stderr, "rene-hip: cannot write %s.length.png\n", bounces_prefix.c_str());
      return 1;
    }
    std::fprintf(stderr, "INFO bounce pass over frames 0 .. %u, at most %u iterations per path: %s.depth0 .. depth9.pfm, %s.length.pfm (largest mean length %.3f)\n",
                 bp.n_frames - 1u, bp.max_depth ? bp.max_depth : RENE_BOUNCES_MAX_DEPTH, bounces_prefix.c_str(), bounces_prefix.c_str(), (double)longest);
  }
  // the light-group pass as files: the records from the library's own buffer under the library's grouping, the figures on the host
  // (api.lights_group_mean / lights_mix, in fp32)
  if (!lights_prefix.empty()) {
    std::vector<uint8_t> inst_group(desc.n_instances), dist_group(desc.n_lights);
    uint8_t bg_group = 0;
    uint32_t n_used = 0;
    if (rene_lights_default_groups(ctx[0], inst_group.data(), desc.n_instances, dist_group.data(), desc.n_lights, &bg_group, &n_used) != RENE_OK)
      return die("rene_lights_default_groups");
    rene_lights_params lp;
    rene_lights_params_default(&lp);  // (no tables: that same grouping)
    lp.n_frames = lights_frames ? lights_frames : std::max(1u, std::min(spp, RENE_LIGHTS_MAX_FRAMES));
    if (rene_lights(ctx[0], &lp, nullptr, 0) != RENE_OK) return die("rene_lights");
    std::vector<rene_lights_pixel> rec(n_px);
    if (rene_download_lights(ctx[0], rec.data(), rec.size() * sizeof(rene_lights_pixel)) != RENE_OK) return die("rene_download_lights");
    std::vector<float> plane(3 * n_px);
    std::string names;
    for (uint32_t g = 0; g < n_used; ++g) {
      std::fill(plane.begin(), plane.end(), 0.0f);
      for (size_t i = 0; i < n_px; ++i)
        for (size_t ch = 0; ch < 3 && rec[i].n; ++ch) plane[ch * n_px + i] = rec[i].group[g].sum[ch] / (float)rec[i].n;
      const std::string path = lights_prefix + ".group" + std::to_string(g) + ".pfm";
      if (!write_pfm(path, plane.data(), desc.xresolution, desc.yresolution, 3)) {
        std::fprintf(stderr, "rene-hip: cannot write %s\n", path.c_str());
        return 1;
      }
      names += "group " + std::to_string(g) + ":";
      if (bg_group == g) names += " background";
      for (uint32_t li = 0; li < desc.n_lights; ++li)
        if (dist_group[li] == g) names += " distant " + std::to_string(li);
      for (uint32_t k = 0; k < desc.n_instances; ++k)
        if (inst_group[k] == g && desc.area_lights[desc.instances[k].area_light_index].type != RENE_AREA_LIGHT_NULL) names += " instance " + std::to_string(k);
      names += "\n";
    }
    {
      const std::string path = lights_prefix + ".groups.txt";
      std::FILE* f = std::fopen(path.c_str(), "w");
      if (!f || std::fputs(names.c_str(), f) < 0 || std::fclose(f) != 0) {
        std::fprintf(stderr, "rene-hip: cannot write %s\n", path.c_str());
        return 1;
      }
    }
    if (!lights_mix.empty()) {
      std::vector<float> mean(3 * n_px, 0.0f);  // interleaved, for the bytes
      std::fill(plane.begin(), plane.end(), 0.0f);
      for (size_t i = 0; i < n_px; ++i)
        for (size_t ch = 0; ch < 3 && rec[i].n; ++ch) {
          float s = lights_weights[0] * rec[i].group[0].sum[ch];
          for (uint32_t g = 1; g < RENE_LIGHTS_GROUPS; ++g) s = s + lights_weights[g] * rec[i].group[g].sum[ch];
          plane[ch * n_px + i] = mean[3 * i + ch] = s / (float)rec[i].n;
        }
      std::vector<uint8_t> bytes(3 * n_px);
      rene_to_rgb8(mean.data(), mean.size(), 1, bytes.data());
      if (!write_pfm(lights_prefix + ".mix.pfm", plane.data(), desc.xresolution, desc.yresolution, 3) ||
          !write_png(lights_prefix + ".mix.png", bytes.data(), desc.xresolution, desc.yresolution)) {
        std::fprintf(stderr, "rene-hip: cannot write %s.mix.pfm / .mix.png\n", lights_prefix.c_str());
        return 1;
      }
    }
    std::fprintf(stderr, "INFO light-group pass over frames 0 .. %u, %u groups: %s.group0 .. group%u.pfm, %s.groups.txt%s\n", lp.n_frames - 1u, n_used, lights_prefix.c_str(),
                 n_used - 1u, lights_prefix.c_str(), lights_mix.empty() ? "" : ", the mix");
  }
  // the pass layers as one OpenEXR file: the passes the layers read, over the job's own frames, into the library's buffers -- behind the files of
  // --ao, --direct, --bounces and --lights, which read the library-owned records these calls overwrite -- then packed and compressed on the device
  if (!exr_passes_path.empty()) {
    const uint32_t F = passes_params.layers;
    if (sampled < 1u || sampled > 65536u) {
      std::fprintf(stderr, "rene-hip: --exr-passes: the passes take 1 .. 65536 frames, the job has %u\n", sampled);
      return 1;
    }
    if (passes_ao) {
      rene_occlusion_params op = ao_params;
      op.first_frame = frame_base, op.n_frames = sampled;
      if (rene_occlusion(ctx[0], &op, nullptr, 0) != RENE_OK) return die("rene_occlusion");
    }
    if (F & (RENE_EXRP_DIRECT | RENE_EXRP_INDIRECT)) {
      rene_direct_params dp;
      rene_direct_params_default(&dp);
      dp.first_frame = frame_base, dp.n_frames = sampled;
      if (rene_direct(ctx[0], &dp, nullptr, 0) != RENE_OK) return die("rene_direct");
    }
    if (passes_bounces) {
      rene_bounces_params bp;
      rene_bounces_params_default(&bp);
      bp.first_frame = frame_base, bp.n_frames = sampled, bp.max_depth = bounces_max_depth;
      if (rene_bounces(ctx[0], &bp, nullptr, 0) != RENE_OK) return die("rene_bounces");
    }
    if (F & RENE_EXRP_LIGHTS) {
      rene_lights_params lp;
      rene_lights_params_default(&lp);  // (no tables: the library's grouping, as --lights)
      lp.first_frame = frame_base, lp.n_frames = sampled;
      if (rene_lights(ctx[0], &lp, nullptr, 0) != RENE_OK) return die("rene_lights");
    }
    if (rene_write_exr_passes(ctx[0], &passes_params, exr_compression, exr_passes_path.c_str()) != RENE_OK) return die("rene_write_exr_passes");
    uint32_t bpp = 0;
    rene_exr_passes_layout(desc.xresolution, desc.yresolution, &passes_params, nullptr, nullptr, &bpp);
    std::fprintf(stderr, "INFO pass layers over frames %u .. %u, layers 0x%02x, %u bytes per pixel: %s\n", frame_base, frame_base + sampled - 1u, F, bpp,
                 exr_passes_path.c_str());
  }
  // The exchange step of a multi-GPU render: every GPU sends the 32x32 tiles it owns to GPU 0 over xGMI (RCCL inside
  // the library, rene_gather_tiles; one process, one communicator over the `gpus` contexts).  Only where RCCL is
  // missing do the per-GPU images meet on the host instead.
  bool gathered = false;
  if (gpus > 1) {
    if (rene_comm_init_all(ctx.data(), (int)gpus) == RENE_OK) {
      bool ok = rene_comm_group_begin() == RENE_OK;
      for (uint32_t g = 0; g < gpus && ok; ++g) ok = rene_gather_tiles(ctx[g], 0) == RENE_OK;
      ok = rene_comm_group_end() == RENE_OK && ok;
      if (!ok) return die("rene_gather_tiles");
      for (uint32_t g = 0; g < gpus; ++g)
        if (rene_sync(ctx[g]) != RENE_OK) return die("rene_sync");
      gathered = true;
    } else {
      std::fprintf(stderr, "WARN %s -- summing the per-GPU images on the host\n", rene_last_error());
    }
  }
  auto layer = [&](int l, std::vector<float>& sum) -> bool {
    sum.assign(n_px * 3, 0.0f);
    if (adaptive) return rene_download_mean(ctx[0], l, 3, sum.data(), sum.size()) == RENE_OK;  // every pixel over its own tile's frames
    if (gathered || gpus == 1) return rene_download(ctx[0], l, 3, sum.data(), sum.size()) == RENE_OK;
    std::vector<float> part(n_px * 3);
    for (uint32_t g = 0; g < gpus; ++g) {
      if (rene_download(ctx[g], l, 3, part.data(), part.size()) != RENE_OK) return false;
      for (size_t i = 0; i < sum.size(); ++i) sum[i] += part[i];
    }
    return true;
  };
  uint64_t rays = 0;
  double kernel_ms = 0.0;
  for (uint32_t g = 0; g < gpus; ++g) {
    rene_stats st;
    if (rene_get_stats(ctx[g], &st) != RENE_OK) return die("rene_get_stats");  // e.g. a hand-off timed out: no image is written
    rays += st.rays_closest + st.rays_shadow + st.rays_emitter;
    kernel_ms = std::max(kernel_ms, st.kernel_ms);
  }
  std::vector<float> img;
  std::vector<uint8_t> rgb(n_px * 3);
  if (atrous) {  // the filtered radiance replaces the download; same unit (sums over spp frames), same output transform
    const auto t_dn = std::chrono::steady_clock::now();
    if (reject) {
      if (atrous_tiles ? rene_denoise_tiles_robust(ctx[0], nullptr, &reject_params) != RENE_OK : rene_denoise_robust(ctx[0], nullptr, &reject_params) != RENE_OK)
        return die(atrous_tiles ? "rene_denoise_tiles_robust" : "rene_denoise_robust");
    } else if (atrous_tiles ? rene_denoise_tiles(ctx[0], nullptr) != RENE_OK : rene_denoise(ctx[0], nullptr) != RENE_OK) return die(atrous_tiles ? "rene_denoise_tiles" : "rene_denoise");
    const double dn_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_dn).count();
    if (!device_output) img.assign(n_px * 3, 0.0f);
    // (an adaptive job's tiles differ in their frame counts: its image is the filtered MEAN, like the unfiltered one it replaces)
    if (!device_output && rene_download_denoised(ctx[0], adaptive ? RENE_DENOISED_MEAN : RENE_DENOISED_RADIANCE, 3, img.data(), img.size()) != RENE_OK) return die("rene_download_denoised");
    std::string invalid;
    if (atrous_tiles) {  // tiles the filter left as they were: fewer than two frames, so fewer than two chains (a job's frames are one range)
      std::vector<uint32_t> frames((size_t)tiles_x * tiles_y);
      if (rene_tile_frames(ctx[0], frames.data(), frames.size()) != RENE_OK) return die("rene_tile_frames");
      const size_t n_invalid = (size_t)std::count_if(frames.begin(), frames.end(), [](uint32_t f) { return f < 2u; });
      invalid = ", " + std::to_string(n_invalid) + " of " + std::to_string(frames.size()) + " tiles invalid (left unfiltered)";
    }
    std::fprintf(stderr, "INFO atrous denoiser: %.3f ms (five passes over %u x %u pixels, its buffers' allocation included%s) after %.1f ms of rendering\n", dn_ms,
                 desc.xresolution, desc.yresolution, invalid.c_str(), render_ms);
    if (reject) {
      std::vector<float> trimmed(n_px);
      if (rene_download_denoised(ctx[0], RENE_DENOISED_TRIM, 1, trimmed.data(), trimmed.size()) != RENE_OK) return die("rene_download_denoised");
      const size_t n_trimmed = (size_t)std::count_if(trimmed.begin(), trimmed.end(), [](float j) { return j > 0.0f; });
      std::fprintf(stderr, "INFO firefly rejection: %.2f %% of the pixels left chains out (max_trim %u, gain %g)\n", n_px ? 100.0 * (double)n_trimmed / (double)n_px : 0.0,
                   reject_params.max_trim, (double)reject_params.gain);
    }
  } else if (!device_output) {
    if (robust) img = robust_img;  // a mean already
    else if (!layer(RENE_LAYER_RADIANCE, img)) return die("rene_download");
  }
  const uint32_t divisor = adaptive ? 1u : sampled;  // (the adaptive job's layers are means already)
  // --exposure: eighth-stops, given or from the image's luminance histogram (`stats`: counted on the device or on the host)
  auto exposure_scale = [&](const rene_luminance_stats* stats) {
    int e8 = (int)std::floor(std::min(std::max(exposure_ev, -1e6), 1e6) * 8.0 + 0.5);
    if (auto_exposure) {
      e8 = rene_auto_exposure_e8(stats, RENE_EXPOSURE_KEY_E8);
      std::fprintf(stderr, "INFO auto exposure: %+.3f EV (%d eighth-stops; mean bin %.2f of %u, %u of %u pixels dark)\n", e8 / 8.0, e8,
                   rene_luminance_mean_bin_x256(stats) / 256.0, (unsigned)RENE_LUMINANCE_BINS, stats->n_dark, stats->n_pixels);
    }
    return rene_exposure_scale(e8);
  };
  auto device_image = [&](uint32_t source) -> bool {  // `rgb` = the 8-bit pixels of `source`, transformed on the device
    rene_output_params op;
    rene_output_params_default(&op);
    op.source = source;
    return rene_output_8bit(ctx[0], &op, nullptr, 0) == RENE_OK && rene_download_output(ctx[0], rgb.data(), rgb.size()) == RENE_OK;
  };
  if (device_output) {
    const uint32_t source = atrous ? (adaptive ? RENE_OUTPUT_DENOISED_MEAN : RENE_OUTPUT_DENOISED) : robust ? RENE_OUTPUT_ROBUST : RENE_OUTPUT_RADIANCE;
    if (tonemapped) {
      rene_luminance_stats stats{};
      if (auto_exposure && rene_luminance_histogram(ctx[0], source, &stats) != RENE_OK) return die("rene_luminance_histogram");
      rene_tonemap_params tp;
      rene_tonemap_params_default(&tp);
      tp.source = source;
      tp.op = tonemap_op;
      tp.scale = exposure_scale(&stats);
      tp.white = white;
      if (rene_output_tonemapped(ctx[0], &tp, nullptr, 0) != RENE_OK || rene_download_output(ctx[0], rgb.data(), rgb.size()) != RENE_OK) return die("rene_output_tonemapped");
    } else if (!device_image(source)) return die("rene_output_8bit");
  } else if (tonemapped) {  // the same arithmetic on the host: the means the device would divide out, then rene_tonemap_rgb8
    const float denom = (float)(robust ? 1u : divisor);
    for (float& v : img) v = v / denom;
    rene_luminance_stats stats{};
    if (auto_exposure && rene_luminance_histogram_host(img.data(), n_px, 3, &stats) != RENE_OK) return die("rene_luminance_histogram_host");
    if (rene_tonemap_rgb8(img.data(), n_px, 3, tonemap_op, exposure_scale(&stats), white, rgb.data()) != RENE_OK) return die("rene_tonemap_rgb8");
  } else rene_to_rgb8(img.data(), img.size(), robust ? 1u : divisor, rgb.data());  // average + to_rgb8, main.rs:1621, 1649
  // the job's layers as one OpenEXR file: the body packed on the device, behind the denoiser and the geometry pass whose results it reads
  if (!exr_path.empty() && exr_compression == RENE_EXR_COMPRESSION_NONE && rene_write_exr(ctx[0], &exr_params, exr_path.c_str()) != RENE_OK) return die("rene_write_exr");
  if (!exr_path.empty() && exr_compression != RENE_EXR_COMPRESSION_NONE && rene_write_exr_compressed(ctx[0], &exr_params, exr_compression, exr_path.c_str()) != RENE_OK)
    return die("rene_write_exr_compressed");
  // the id mattes by name: one geometry pass per layer -- behind --gbuffer's files and --exr's, which read the library-owned records this overwrites
  if (!cryptomatte_path.empty()) {
    rene_gbuffer_params cg;
    rene_gbuffer_params_default(&cg);
    cg.n_frames = cryptomatte_frames ? cryptomatte_frames : std::max(1u, std::min(spp, 16u));
    std::vector<const char*> names[2];
    rene_cryptomatte_layer layers[2] = {};
    rene_ctx* second = nullptr;  // holds the second layer's records
    std::string info = "INFO cryptomatte:";
    for (size_t k = 0; k < cryptomatte_sources.size(); ++k) {
      const bool objects = cryptomatte_sources[k] == RENE_GBUFFER_ID_INSTANCE;
      const uint32_t n = objects ? desc.n_instances : desc.n_materials;
      for (uint32_t i = 0; i < n; ++i) names[k].push_back(objects ? rene_scene_instance_name(scene, i) : rene_scene_material_name(scene, i));
      layers[k].name = objects ? "CryptoObject" : "CryptoMaterial";
      layers[k].id_source = cg.id_source = cryptomatte_sources[k];
      layers[k].n_names = n;
      layers[k].names = names[k].data();
      if (k == 0) {
        if (rene_gbuffer(ctx[0], &cg, nullptr, 0) != RENE_OK) return die("rene_gbuffer");
      } else {
        rene_opts o{};
        o.struct_size = sizeof(o);
        o.seed = seed;
        o.shard_mode = RENE_SHARD_TILES;
        o.shard_count = 1;
        if (frame_groups) o.flags |= RENE_FLAG_FRAME_GROUPS;
        void* records = nullptr;
        size_t record_bytes = 0;
        if (rene_create(&desc, &o, &second) != RENE_OK) return die("rene_create");
        if (rene_gbuffer(second, &cg, nullptr, 0) != RENE_OK || rene_gbuffer_buffer(second, &records, &record_bytes) != RENE_OK) return die("rene_gbuffer");
        layers[k].records = records;
      }
      info += std::string(k ? ", " : " ") + layers[k].name + " " + std::to_string(std::set<std::string>(names[k].begin(), names[k].end()).size()) + " distinct names over " +
              std::to_string(n) + (objects ? " instances" : " materials");
    }
    std::fprintf(stderr, "%s\n", info.c_str());
    rene_cryptomatte_params cp;
    rene_cryptomatte_params_default(&cp);
    cp.n_layers = (uint32_t)cryptomatte_sources.size();
    cp.layers = layers;
    const int rc = rene_write_cryptomatte(ctx[0], &cp, exr_compression, cryptomatte_path.c_str());
    if (second) rene_destroy(second);
    if (rc != RENE_OK) return die("rene_write_cryptomatte");
  }
  std::string filename = out_override.empty() ? rene_scene_film_filename(scene) : out_override;
  if (filename.size() >= 4 && filename.compare(filename.size() - 4, 4, ".exr") == 0) {
    std::fprintf(stderr, "INFO .exr output is not yet supported. Save as .png\n");  // main.rs:1651-1656
    filename += ".png";
  }
  if (!write_png(filename, rgb.data(), desc.xresolution, desc.yresolution)) {
    std::fprintf(stderr, "rene-hip: cannot write %s\n", filename.c_str());
    return 1;
  }
  if (!aov_normal.empty()) {  // main.rs:1667-1676
    if (device_output) {
      if (!device_image(RENE_OUTPUT_NORMAL)) return die("rene_output_8bit");
    } else {
      if (!layer(RENE_LAYER_NORMAL, img)) return die("rene_download");
      rene_to_aov8(img.data(), img.size(), divisor, 1, rgb.data());
    }
    if (!write_png(aov_normal, rgb.data(), desc.xresolution, desc.yresolution)) return 1;
  }
  if (!aov_albedo.empty()) {  // main.rs:1678-1687
    if (device_output) {
      if (!device_image(RENE_OUTPUT_ALBEDO)) return die("rene_output_8bit");
    } else {
      if (!layer(RENE_LAYER_ALBEDO, img)) return die("rene_download");
      rene_to_aov8(img.data(), img.size(), divisor, 0, rgb.data());
    }
    if (!write_png(aov_albedo, rgb.data(), desc.xresolution, desc.yresolution)) return 1;
  }
  for (rene_ctx* c : ctx) rene_destroy(c);
  rene_scene_free(scene);
  std::fprintf(stderr, "INFO %llu rays, %.1f Mrays/s (%.1f ms of rendering on %u GPU(s); launch durations add up to %.1f ms)\n",
               (unsigned long long)rays, render_ms > 0 ? rays / render_ms / 1e3 : 0.0, render_ms, gpus, kernel_ms);
  std::fprintf(stderr, "INFO End (%lld ms)\n", ms_since(t_start));
  if (want_noise)
    std::fprintf(stderr, "noise: %.6g (worst tile %.6g at %u,%u) after %u samples\n", noise.noise, noise.worst_tile_noise, noise.worst_tile % tiles_x,
                 noise.worst_tile / tiles_x, sampled);
  return 0;
}
