// rene_hip.cpp -- implementation of the C ABI declared in include/rene_hip.h (render path part).
// Compiled with hipcc; owns all device memory; never throws or aborts across the boundary.
#include "../../include/rene_hip.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <rccl/rccl.h>  // types only: the library is loaded on demand (rccl() below)

#include <algorithm>
#include <array>
#include <cerrno>
#include <chrono>
#include <thread>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "device_scene.h"
#include "exr_deflate.h"
#include "kernels.h"
#include "launch_plan.h"
#include "scene_pack.h"

namespace {

thread_local std::string g_error;

int fail(int code, const std::string& msg) {
  g_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(e_ == hipErrorOutOfMemory ? RENE_ERR_OUT_OF_MEMORY : RENE_ERR_DEVICE,            \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                              \
  } while (0)

// a tuning knob of the environment as launch_plan.h takes it: the variable's integer, or nothing where it is not set
std::optional<int> env_int(const char* name) {
  const char* e = std::getenv(name);
  return e ? std::optional<int>(std::atoi(e)) : std::nullopt;
}

// PCG32si restated for the host-side seed schedule (rene-shader/src/rand.rs:4-52)
struct HostPcg {
  uint32_t s;
  explicit HostPcg(uint32_t seed) : s(seed) {
    step();
    s += seed;
    step();
  }
  void step() { s = s * 747796405u + 2891336453u; }
  uint32_t next() {
    uint32_t o = s;
    step();
    uint32_t w = ((o >> ((o >> 28) + 4u)) ^ o) * 277803737u;
    return (w >> 22) ^ w;
  }
  // n steps at once (the LCG's n-fold composition by repeated squaring): frame k's seed is the k-th output, and a
  // caller may ask for frame four billion without anybody having produced the ones before it
  void skip(uint64_t n) {
    uint32_t mul = 747796405u, add = 2891336453u, acc_mul = 1u, acc_add = 0u;
    for (; n; n >>= 1) {
      if (n & 1u) {
        acc_mul *= mul;
        acc_add = acc_add * mul + add;
      }
      add = (mul + 1u) * add;
      mul *= mul;
    }
    s = acc_mul * s + acc_add;
  }
};

}  // namespace

namespace rene {
void set_last_error(const std::string& msg) { g_error = msg; }
thread_local uint32_t g_launched_blocks = 0;
void log_render_launch(const void* kernel, hipStream_t st) {  // RENE_TEST_KERNEL_LOG (kernels.h)
  const char* path = std::getenv("RENE_TEST_KERNEL_LOG");
  if (!path || !*path) return;
  const char* name = hipKernelNameRefByPtr(kernel, st);
  if (FILE* f = std::fopen(path, "a")) {
    std::fprintf(f, "%s\n", name ? name : "?");
    std::fclose(f);
  }
}
}

// ---- RCCL, loaded on demand: a host that never shards keeps running where librccl.so is absent -----------------
namespace {
struct Rccl {
  void* handle = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclReduce) Reduce = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string error;
};
Rccl* rccl() {
  static Rccl* r = [] {
    Rccl* x = new Rccl();
    // a process that already holds an RCCL (PyTorch ships its own copy) uses that one; else the ROCm installation's
    // (RENE_RCCL_LIB=<path> names the library instead: hosts that keep it elsewhere, and the test of the missing-library path)
    const char* over = std::getenv("RENE_RCCL_LIB");
    const char* defaults[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    std::vector<const char*> names;
    static std::vector<std::string> over_names;  // RENE_RCCL_LIB may hold several candidates, ':'-separated, tried in order like the defaults
    if (over && *over) {
      std::string all(over);
      for (size_t b = 0; b <= all.size();) {
        size_t e = all.find(':', b);
        if (e == std::string::npos) e = all.size();
        if (e > b) over_names.push_back(all.substr(b, e - b));
        b = e + 1;
      }
      for (const std::string& n : over_names) names.push_back(n.c_str());
    } else names.assign(defaults, defaults + 3);
    for (const char* n : names) {
      x->handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
      if (x->handle) break;
    }
    std::string why;  // a COPY: dlerror()'s buffer belongs to the loader and the next failing dlopen() rewrites it
    for (const char* n : names) {
      if (x->handle) break;
      x->handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (!x->handle && why.empty()) {
        if (const char* m = dlerror()) why = m;
      }
    }
    if (!x->handle) {
      x->error = std::string("RCCL is not available: ") + (why.empty() ? "librccl.so not found" : why);
      return x;
    }
    bool ok = true;
    auto sym = [&](const char* name) {
      void* p = dlsym(x->handle, name);
      if (!p) { ok = false; x->error = std::string("RCCL lacks ") + name; }
      return p;
    };
    x->GetUniqueId = reinterpret_cast<decltype(x->GetUniqueId)>(sym("ncclGetUniqueId"));
    x->CommInitRank = reinterpret_cast<decltype(x->CommInitRank)>(sym("ncclCommInitRank"));
    x->CommInitAll = reinterpret_cast<decltype(x->CommInitAll)>(sym("ncclCommInitAll"));
    x->CommDestroy = reinterpret_cast<decltype(x->CommDestroy)>(sym("ncclCommDestroy"));
    x->Reduce = reinterpret_cast<decltype(x->Reduce)>(sym("ncclReduce"));
    x->Send = reinterpret_cast<decltype(x->Send)>(sym("ncclSend"));
    x->Recv = reinterpret_cast<decltype(x->Recv)>(sym("ncclRecv"));
    x->GroupStart = reinterpret_cast<decltype(x->GroupStart)>(sym("ncclGroupStart"));
    x->GroupEnd = reinterpret_cast<decltype(x->GroupEnd)>(sym("ncclGroupEnd"));
    x->GetErrorString = reinterpret_cast<decltype(x->GetErrorString)>(sym("ncclGetErrorString"));
    if (!ok) { dlclose(x->handle); x->handle = nullptr; }
    return x;
  }();
  return r;
}
#define RCCL_TRY(expr)                                                                                   \
  do {                                                                                                   \
    ncclResult_t r_ = (expr);                                                                            \
    if (r_ != ncclSuccess) return fail(RENE_ERR_DEVICE, std::string(#expr) + ": " + R->GetErrorString(r_)); \
  } while (0)
}  // namespace


// Host-side waits poll (hipEventQuery / hipStreamQuery read the completion signal) instead of blocking in the runtime: a
// blocked wait depends on a wake-up from the driver, and on this pool a job of many launches was seen to sit in
// one for minutes now and then (docs/history.md section 4g); polling costs one host thread a few microseconds of latency.
static hipError_t wait_event(hipEvent_t ev) {
  const auto t0 = std::chrono::steady_clock::now();
  int told = 0;
  for (uint64_t spins = 0;; ++spins) {
    const hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    if ((spins & 0xfffu) == 0xfffu && std::getenv("RENE_DEBUG")) {
      const double s_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (s_ > 10.0 * (told + 1)) {
        ++told;
        std::fprintf(stderr, "[rene] still waiting for a launch to complete after %.0f s (its completion signal has not fired)\n", s_);
      }
    }
    if (spins < 2000) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}
static hipError_t wait_stream(hipStream_t st) {
  for (uint64_t spins = 0;; ++spins) {
    const hipError_t e = hipStreamQuery(st);
    if (e != hipErrorNotReady) return e;
    if (spins < 2000) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

// the tiles rank `rank` of `count` owns of a grid of n_tiles: rank, rank + count, ...
static uint32_t owned_tiles(uint32_t n_tiles, uint32_t rank, uint32_t count) { return n_tiles > rank ? (n_tiles - rank + count - 1u) / count : 0u; }

// Memory that goes with its owner -- a context, or a probe call's scope: the pointer and its capacity in one place.  Device memory (DevBuf), or
// pinned host memory for the stagings (HostBuf).  A context allocates what every job needs in rene_create and the rest when a call first needs it,
// grown to the largest request so far; all of it is freed with the context (rene_destroy selects the device before it deletes the context).
template <bool Pinned>
struct Buf {
  void* p = nullptr;
  size_t cap = 0;  // bytes
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }
  static hipError_t alloc(void** p, size_t bytes) { return Pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return Pinned ? hipHostFree(p) : hipFree(p); }
  void release() {
    if (p) free(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  // Nothing where the capacity suffices; else what is there is freed and `bytes` are allocated.  A buffer that could not be had is empty (capacity 0).
  // The caller sees to it that no launch in flight reads the memory a growing buffer frees.
  hipError_t grow(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    hipError_t e = p ? free(p) : hipSuccess;
    p = nullptr;
    cap = 0;
    if (e == hipSuccess) e = alloc(&p, bytes);
    if (e != hipSuccess) p = nullptr;
    else cap = bytes;
    return e;
  }
  int reserve(size_t bytes, const std::string& label) {
    const hipError_t e = grow(bytes);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RENE_ERR_OUT_OF_MEMORY : RENE_ERR_DEVICE, label + ": " + hipGetErrorString(e));
    return RENE_OK;
  }
};
using DevBuf = Buf<false>;
using HostBuf = Buf<true>;
// ... device memory of one element type, read where a T* is wanted
template <class T>
struct DevArray : DevBuf {
  operator T*() const { return as<T>(); }
};
// A result a call leaves in a device buffer of the library's own where the caller gives no destination: the buffer (allocated by the first such
// call, grown to the largest so far), the bytes of the last result (0 while there is none), and what it was made with
struct Result {
  DevBuf buf;
  size_t bytes = 0;
  bool valid = false;
  std::array<uint32_t, 3> key{};
  // A producing call starts: no result until commit(), at least max(16, need) bytes, `dst` is where they go.  With a key the producer writes the
  // pixels of the owned tiles only and the rest must read zero: the whole buffer is zeroed when it regrew or the key differs from the last call's,
  // on `stream`, ahead of the kernel (rene_resolve_robust has the reason).  Without one the producer writes every byte itself.
  int begin(size_t need, std::initializer_list<uint32_t> k, hipStream_t stream, const std::string& label, void*& dst) {
    invalidate();
    const size_t want = std::max<size_t>(16, need);
    const bool regrow = want > buf.cap;
    if (int rc = buf.reserve(want, label); rc != RENE_OK) return rc;
    std::array<uint32_t, 3> now{};
    std::copy(k.begin(), k.end(), now.begin());
    if (k.size() && (regrow || now != key)) {
      const hipError_t e = hipMemsetAsync(buf.p, 0, buf.cap, stream);
      if (e != hipSuccess) return fail(RENE_ERR_DEVICE, label + ": " + hipGetErrorString(e));
      key = now;
    }
    dst = buf.p;
    return RENE_OK;
  }
  void commit(size_t n) {
    bytes = n;
    valid = true;
  }
  void invalidate() {
    bytes = 0;
    valid = false;
  }
};

// An event that is destroyed with its scope, or with the launch record that holds it
struct Event {
  hipEvent_t ev = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
  Event& operator=(Event&&) = delete;
  ~Event() {
    if (ev) hipEventDestroy(ev);
  }
  hipError_t create() { return hipEventCreate(&ev); }
  operator hipEvent_t() const { return ev; }
};

struct rene_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  rene_opts opts{};
  std::deque<DevBuf> allocations;  // the scene's tables (upload) and the wavefront integrator's queues
  rene::SceneView view{};
  rene::LaunchConfig cfg{};
  uint32_t width = 0, height = 0, tiles_x = 0, n_tiles = 0, n_work = 0, n_materials = 0, n_mediums = 0;  // n_work: the owned pixel slots (device_scene.h)
  float* fb = nullptr;
  DevBuf fb_own;  // the image where rene_opts gave no framebuffer (else empty: `fb` is the caller's, borrowed)
  size_t fb_floats = 0;
  // frame chains (device_scene.h, CHAINS): the kernels accumulate into `chains`, [CHAINS][3][n_work][4] over the owned pixel slots, the library's own; `fb` -- the context's or
  // the caller's -- is the image handed out: the chains added in chain order whenever a drain finds launches since the last one (`fb_stale`)
  DevArray<float> chains;
  bool fb_stale = false;
  float* ray_dump = nullptr;     // rene_ray_dump in progress: where the counting restart kernel records its queries
  uint32_t ray_dump_cap = 0;
  static constexpr uint32_t kCounters = 60;  // launches between two drains: each takes its own zeroed work counter
  DevArray<uint32_t> d_work_counters;            // [kCounters]: batches of work ids handed out
  DevArray<unsigned long long> d_wave_times;     // RENE_DEBUG: [kCounters][8192][2], allocated by the first launch under it
  uint32_t counters_used = 0;
  uint32_t epoch = 0, prev_final = 0;
  // frames per work item: kWholeLaunch = one item per pixel and launch; 0 = not tuned (rene_tune picks): 64 for the
  // item-loop kernels, whose item switches cost a memory round trip of the whole wave, 32 for the BVH kernels, where
  // pixels differ more in cost and a lane that waits is a lane the ballots miss
  static constexpr uint32_t kWholeLaunch = rene::kWholeLaunch;
  uint32_t item_frames = 0;
  std::vector<uint32_t> inst_material;  // material index of every instance (rene_bsdf_eval looks an instance of its material up)
  std::vector<uint8_t> inst_emits;      // 1: the instance carries an area light (Inst::emit[3]; rene_lights_default_groups)
  DevArray<uint32_t> d_item_done;  // [CHAINS][n_work] versions, traversal-restart kernels only (device_code.inc, item_flag_publish)
  DevArray<unsigned long long> d_counters;
  // stage-separated wavefront integrator (BVH scenes): path state in HBM + a pinned word for the host loop
  bool wavefront = false;
  rene::WaveState wave{};
  HostBuf h_done;  // (one uint32_t)
  // per-launch resources that must outlive the asynchronous launch
  struct Pending {
    Event start, stop;
    uint32_t epoch = 0;
    bool replayable = false;    // a persistent render launch: what it was launched with, should it have to be launched again
    rene::RenderParams P{};
    rene::LaunchConfig cfg{};
  };
  uint64_t replays = 0;         // launches launched again by drain() (RENE_DEBUG prints them)
  std::deque<Pending> pending;
  uint64_t frames = 0, launches = 0, owned_pixels = 0, paths = 0;
  double kernel_ms = 0.0, last_ms = 0.0;
  bool handoff_failed = false;
  std::string handoff_detail;
  // multi-GPU exchange (rene_comm_*): the RCCL communicator this context belongs to
  ncclComm_t comm = nullptr;
  int comm_ranks = 0, comm_rank = -1;
  bool exchanged = false;  // an exchange has put other ranks' sums into `fb`, which the next drain would overwrite with this context's chains: rene_reset before rendering again
  DevBuf tile_buf;            // rene_gather_tiles: packed owned tiles (root: of every rank)
  HostBuf h_stage;            // pinned host staging of one layer (rene_download)
  HostBuf h_upload;           // pinned host staging of the scene upload (rene_create), released when it is done
  int unpack_root = -1;       // >= 0: tiles received by rene_gather_tiles wait in tile_buf to be placed (flush_exchange)
  // the `atrous` denoiser (rene_denoise): frames each chain has received since the last reset (host bookkeeping by the kernels' rule, rene_render),
  // and the buffers of the filter, allocated by the first rene_denoise: two ping-pong records + guides + output + variance plane
  uint64_t chain_frames[rene::CHAINS] = {};
  DevBuf dn_rec[2];                       // [H][W][4] demodulated colour, variance of the mean
  DevBuf dn_guides;                       // [H][W][2][4] normal.xyz, albedo.r | albedo.gb, 0, 0
  DevBuf dn_out;                          // [H][W][4] the denoised radiance sums (alpha 0)
  DevBuf dn_var;                          // [H][W] the unfiltered variance of the mean
  bool dn_valid = false;                  // dn_out / dn_var hold the result of a rene_denoise / rene_denoise_tiles since the last reset
  // ... and what RENE_DENOISED_MEAN needs of that call: which of dn_rec holds the filtered records (the other one is free for the means), the
  // floor they were demodulated with, and after a rene_denoise_tiles the N_t of its invalid tiles on the full grid (valid tiles: DN_TILE_VALID)
  uint32_t dn_cur = 0;
  float dn_albedo_floor = 0.0f;
  bool dn_masked = false;
  std::vector<uint32_t> dn_invalid_frames;
  static constexpr uint32_t DN_TILE_VALID = 0xffffffffu;
  // rene_denoise_robust / rene_denoise_tiles_robust: [H][W] one word per pixel, j | kept << 8 (kernels.h), allocated by the first such call; and
  // whether the last denoise of any kind was one of them (RENE_DENOISED_TRIM: otherwise zeros)
  DevBuf dn_trim;
  bool dn_robust = false;
  // the denoiser on tile shards.  A shard: the packed buffer of the last rene_denoise_shard_prepare (header, N_t table, 52 bytes per owned slot).
  // A root: the round in progress -- which ranks have been placed since the last completed rene_denoise_placed, the header the others must agree
  // with, the invalid tiles' N_t on the full grid -- a device staging buffer for a body that is placed, and what rene_gather_denoise received
  Result dn_shard;
  std::vector<uint8_t> dn_placed;
  rene_denoise_shard_header dn_round{};
  std::vector<uint32_t> dn_round_invalid;
  DevBuf dn_place_buf;
  DevBuf dn_gather_buf;           // the root of a rene_gather_denoise: the other ranks' packed buffers, one after the other in rank order
  int dn_gather_root = -1;        // >= 0: buffers wait to be placed by rene_denoise_placed (the received ones and this context's own)
  // the noise estimate (rene_estimate_noise): 16 bytes per owned tile on the device, allocated by the first call, and the last estimate's
  // records on the image's full tile grid (rene_download_noise_tiles)
  DevBuf noise_dev;
  std::vector<rene_noise_tile> noise_tiles;
  bool noise_valid = false;
  // adaptive sampling (rene_set_active_tiles): which owned tiles render (empty: no mask has been set, all of them), the frames a tile had when it was
  // switched off (an active tile has received every frame of the context: N_t = frames), the mask's bits on the device for the launches
  // (RenderParams::active_tiles), and whether the frames so far are ONE range [frame_base, frame_base + frames) -- what lets a tile's chain counts
  // follow from N_t alone
  std::vector<uint8_t> tile_active;
  std::vector<uint32_t> tile_stop;
  uint32_t n_inactive = 0;
  uint64_t inactive_pixels = 0;  // pixels inside the image of the inactive owned tiles
  bool frames_contiguous = true;
  uint32_t frame_base = 0;  // first_frame of the first rene_render since the context was created or reset
  // rene_load_chains (probe) has put the caller's sums into the chains: their version words no longer describe them, so nothing renders onto them
  // until rene_reset
  bool loaded = false;
  DevBuf mask_dev;
  // rene_download_mean: one layer of means and the tiles' frame counts on the full grid -- allocated by the first call that needs them
  DevBuf mean_dev, tile_frames_dev;
  // the chain passes on uneven tiles (upload_tile_sets): one set per distinct N_t -- the noise estimate's constants or the chain counts of the
  // robust resolve and the feature export -- and the set of every owned tile; ONE pair of buffers for all of them, allocated by the first call
  // that needs them and grown to the largest table so far
  DevBuf sets_dev, tile_set_dev;
  // the firefly-robust resolve (rene_resolve_robust): [H][W][4] {robust mean rgb, (float)j} and 16 bytes per owned tile on the device, allocated by the
  // first call (the image zeroed once: a context writes its owned tiles only, always all of them), and the last resolve's records on the image's
  // full tile grid (rene_download_robust_tiles)
  DevBuf robust_img, robust_dev;
  std::vector<rene_robust_tile> robust_tiles;
  bool robust_valid = false;
  // the denoiser hand-off (rene_export_features): the library-owned tensor of an export without a destination of the caller's, zeroed again when the
  // mask, the format or the layout change
  Result features;
  // the output transform (rene_output_8bit, rene_output_tonemapped): the sRGB thresholds on the device (uploaded by the first call) and the library-owned
  // image of a call without a destination of the caller's, zeroed again when the format changes
  DevBuf out_thresholds;
  Result out;
  DevBuf lum_rows;  // rene_luminance_histogram's scratch: every workgroup's counts, and their sum behind them
  // the geometry pass (rene_gbuffer): the frames' seeds on the device and the library-owned record array (outside rene_plan_memory's figures)
  DevBuf pass_seeds;  // (shared by the five per-pixel frame-range passes, run_pixel_pass: each drains the stream before it overwrites them)
  Result gbuf;  // (rene_reset leaves it alone: the pass reads the scene and the seed, no frame of the context's)
  // the occlusion pass (rene_occlusion): the library-owned record array, outside rene_plan_memory's figures and left alone by rene_reset like the
  // geometry pass's
  Result occl;
  // the direct-light pass (rene_direct): its library-owned record array, on the same terms
  Result direct;
  // the bounce pass (rene_bounces): its library-owned record array, on the same terms
  Result bounces;
  // the light-group pass (rene_lights): its library-owned record array, on the same terms, and the call's grouping tables on the device --
  // instance_group, then distant_group -- which a call overwrites behind a drained stream, like pass_seeds
  Result lights;
  DevBuf lights_tables;
  // the multi-channel OpenEXR body (rene_output_exr): the library-owned bytes of a call without a destination of the caller's, zeroed again when the
  // layer mask changes
  Result exr;
  // the compressed file's tail (rene_exr_compress): the library-owned table and chunks of a call without a destination of the caller's (its bytes:
  // `written`), outside rene_plan_memory's figures; and the kernels' scratch -- the tail's length, then every chunk's size
  Result exr_tail;
  DevBuf zips_scratch;
  // the Cryptomatte body (rene_output_cryptomatte): the library-owned bytes of a call without a destination of the caller's, the layers' name
  // hashes on the device, and which ids the library-owned geometry records hold (the id_source of the rene_gbuffer that left them)
  Result cryptomatte;
  DevBuf cryptomatte_hashes;
  uint32_t gbuf_id_source = RENE_GBUFFER_ID_INSTANCE;
  // the pass-layer body (rene_output_exr_passes): the library-owned bytes of a call without a destination of the caller's, and the frames the
  // library-owned direct records are sums over (what RENE_EXRP_INDIRECT holds the context's own frames against)
  Result exr_passes;
  uint32_t direct_first_frame = 0, direct_n_frames = 0;
  // the checkpoint (rene_save_state / rene_restore_state): the scene's fingerprint, taken once by rene_create; and what the first of the calls allocates --
  // two device chunk buffers and two pinned stagings of chunk_tiles tiles each, the tiles' checksums on the device, a stream for the copies and the
  // events that order the copies and the kernels of the two buffers
  uint64_t fingerprint[2] = {0, 0};
  DevBuf state_dev[2], state_sums;
  HostBuf state_host[2];
  hipStream_t state_stream = nullptr;
  Event state_kernel_done[2], state_copy_done[2];
  uint32_t n_owned() const { return n_work / rene::TILE_SLOTS; }
  uint32_t owned_tile(uint32_t k) const {  // image tile of owned tile k
    return opts.shard_mode == RENE_SHARD_TILES ? opts.shard_rank + k * opts.shard_count : k;
  }
  uint32_t tile_pixels(uint32_t tile) const {  // its pixels inside the image
    const uint32_t x0 = (tile % tiles_x) * RENE_TILE_SIZE, y0 = (tile / tiles_x) * RENE_TILE_SIZE;
    return std::min<uint32_t>(RENE_TILE_SIZE, width - x0) * std::min<uint32_t>(RENE_TILE_SIZE, height - y0);
  }
  uint32_t tile_n(uint32_t k) const {  // N_t of owned tile k
    if (n_inactive && !tile_active[k]) return tile_stop[k];
    return (uint32_t)std::min<uint64_t>(frames, 0xffffffffull);
  }
  bool uneven() const {  // do owned tiles differ in N_t?
    if (!n_inactive) return false;
    for (uint32_t k = 0; k < n_owned(); ++k)
      if (tile_n(k) != tile_n(0)) return true;
    return false;
  }
  void clear_active_tiles() {
    tile_active.clear();
    tile_stop.clear();
    n_inactive = 0;
    inactive_pixels = 0;
    frames_contiguous = true;
    frame_base = 0;
  }
  // the frame-wide sample stream of a launch as a table (device_scene.h, FRAME_STREAM_*), Matte small-scene kernels only: allocated by the first
  // launch that reads it, grown to the longest launch so far (1 KB per launch frame), refilled on the stream before every launch
  DevBuf frame_stream;
  int frame_stream_reserve(uint32_t rows) {
    const size_t bytes = (size_t)rows * rene::FRAME_STREAM_STRIDE * 4 * sizeof(float);
    if (bytes <= frame_stream.cap) return RENE_OK;
    int rc = drain();  // launches in flight -- and their replays -- read the table that is about to be freed
    if (rc != RENE_OK) return rc;
    return frame_stream.reserve(bytes, "frame stream table");
  }
  // the frames every chain receives from `count` consecutive frames the first of which belongs to chain phase % CHAINS: frame i goes to chain
  // (phase + i) % CHAINS.  The launches are counted with it, and a tile's chain counts follow from it: its frames are [frame_base, frame_base + N_t)
  static void chain_counts(uint32_t phase, uint32_t count, uint64_t out[rene::CHAINS]) {
    for (uint32_t i = 0; i < rene::CHAINS; ++i) out[(phase + i) % rene::CHAINS] = count / rene::CHAINS + (i < count % rene::CHAINS ? 1u : 0u);
  }
  void count_chain_frames(uint32_t phase, uint32_t count) {
    uint64_t n[rene::CHAINS];
    chain_counts(phase, count, n);
    for (uint32_t g = 0; g < rene::CHAINS; ++g) chain_frames[g] += n[g];
  }
  // seed schedule cache: seeds[k] = k-th next_u32 of PCG32si::new(master)

  template <class T>
  int upload(const std::vector<T>& v, const T** out) {
    size_t bytes = std::max<size_t>(1, v.size()) * sizeof(T);
    if (int rc = allocations.emplace_back().reserve(bytes, "rene_create: scene tables"); rc != RENE_OK) return rc;
    void* p = allocations.back().p;
    if (!v.empty()) {
      int rc = staged_upload(p, v.data(), v.size() * sizeof(T), nullptr);
      if (rc != RENE_OK) return rc;
    } else {
      HIP_TRY(hipMemset(p, 0, bytes));
    }
    *out = static_cast<const T*>(p);
    return RENE_OK;
  }
  // host memory -> device memory through pinned staging, in pieces: a copy straight from pageable memory makes the runtime register the
  // caller's pages with the driver for the duration of the copy (see rene_download).  st == nullptr: synchronous copies (rene_create);
  // else every piece is copied on `st` and waited for, the staging buffer being written again by the next one (rene_load_chains)
  static constexpr size_t kPiece = 8u << 20;
  int staged_upload(void* dst, const void* src_, size_t total, hipStream_t st) {
    if (int rc = h_upload.reserve(kPiece, "upload staging"); rc != RENE_OK) return rc;
    const char* src = static_cast<const char*>(src_);
    for (size_t off = 0; off < total; off += kPiece) {
      const size_t n = std::min(kPiece, total - off);
      std::memcpy(h_upload.p, src + off, n);
      if (st) {
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + off, h_upload.p, n, hipMemcpyHostToDevice, st));
        HIP_TRY(wait_stream(st));
      } else {
        HIP_TRY(hipMemcpy(static_cast<char*>(dst) + off, h_upload.p, n, hipMemcpyHostToDevice));
      }
    }
    return RENE_OK;
  }
  // ... and its mirror, device memory -> host memory, for the results a context hands out as bytes (result_download, which says for which): whatever
  // their size, in pieces through h_stage, which need hold no more than one
  int staged_fetch(void* dst, const void* src, size_t total) {
    if (int rc = h_stage.reserve(std::min(kPiece, total), "download staging"); rc != RENE_OK) return rc;
    for (size_t off = 0; off < total; off += kPiece) {
      const size_t n = std::min(kPiece, total - off);
      HIP_TRY(hipMemcpy(h_stage.p, static_cast<const char*>(src) + off, n, hipMemcpyDeviceToHost));
      std::memcpy(static_cast<char*>(dst) + off, h_stage.p, n);
    }
    return RENE_OK;
  }

  // root of a rene_gather_tiles: place the other ranks' tiles (enqueued behind the receives on `stream`)
  int flush_exchange() {
    if (unpack_root < 0) return RENE_OK;
    const uint32_t n = (uint32_t)comm_ranks;
    const size_t tile_floats = (size_t)3 * RENE_TILE_SIZE * RENE_TILE_SIZE * 4;
    size_t off = 0;
    for (uint32_t r = 0; r < n; ++r) {
      const uint32_t owned_r = owned_tiles(n_tiles, r, n);
      if ((int)r == unpack_root || owned_r == 0) continue;
      hipError_t e = rene::launch_pack_tiles(fb, tile_buf.as<float>() + off, width, height, tiles_x, n_tiles, r, n, true, stream);
      if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("rene_gather_tiles unpack: ") + hipGetErrorString(e));
      off += owned_r * tile_floats;
    }
    unpack_root = -1;
    return RENE_OK;
  }

  // Zeroes device memory and WAITS for it.  (hipMemset on the null stream returns before the fill has run -- it is a kernel, and
  // behind a persistent launch on another queue it gets a slot only when that launch's first waves leave: the work counters
  // of launches already running were then zeroed under them, their ids handed out a second time, and the duplicates waited
  // for versions that had passed.  docs/history.md section 4g.)
  hipError_t zero_now(void* p, size_t bytes) {
    hipError_t e = hipMemsetAsync(p, 0, bytes, stream);
    return e == hipSuccess ? wait_stream(stream) : e;
  }

  int drain();  // wait for the stream and fold finished launches into the timing totals (below, in its steps)
};

// ---- rene_ctx::drain, in the order it runs ---------------------------------------------------------------------------------------------------------
// RENE_DEBUG: per launch, when its waves started and ended (ms since the first start)
static void report_wave_times(rene_ctx* c) {
  std::vector<unsigned long long> t((size_t)c->counters_used * 8192 * 2);
  if (hipMemcpy(t.data(), c->d_wave_times, t.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
    unsigned long long t0 = ~0ull;
    for (auto v : t) if (v && v < t0) t0 = v;
    for (uint32_t k = 0; k < c->counters_used; ++k) {
      std::vector<double> st, en;
      for (uint32_t w = 0; w < 8192; ++w) {
        const unsigned long long a = t[((size_t)k * 8192 + w) * 2], b = t[((size_t)k * 8192 + w) * 2 + 1];
        if (a) st.push_back((a - t0) * 1e-5);
        if (b) en.push_back((b - t0) * 1e-5);
      }
      std::sort(st.begin(), st.end());
      std::sort(en.begin(), en.end());
      auto q = [](const std::vector<double>& v, double f) { return v.empty() ? -1.0 : v[(size_t)(f * (v.size() - 1))]; };
      std::fprintf(stderr, "[rene] launch slot %u: %zu waves; starts min/50%%/90%%/max %.3f %.3f %.3f %.3f ms; ends min/10%%/50%%/90%%/max %.3f %.3f %.3f %.3f %.3f ms\n", k, st.size(),
                   q(st, 0), q(st, .5), q(st, .9), q(st, 1), q(en, 0), q(en, .1), q(en, .5), q(en, .9), q(en, 1));
    }
  }
  c->zero_now(c->d_wave_times, (size_t)c->counters_used * 8192 * 2 * 8);
}

// the four words at counters + 8: how many lanes dropped their item, then what the first of them left -- its pixel and chain, the launch and the
// version it saw, the version it wanted -- as the RENE_DEBUG line and the error text put it
static std::string dropped_item(const unsigned long long t[4]) {
  return "pixel (" + std::to_string(t[1] & 0x3fffull) + ", " + std::to_string((t[1] >> 14) & 0x3fffull) + ") chain " + std::to_string((t[1] >> 28) & 0x7ull) + ", in launch " +
         std::to_string(t[2] >> 32) + ", wanted version " + std::to_string(t[3]) + ", saw " + std::to_string(t[2] & 0xffffffffull);
}

// Items whose hand-off did not come were DROPPED by their lanes (device_code.inc: the waves that render the awaited
// item can be parked by the driver behind this launch's own -- a queue eviction restores the queues in its own order --
// and from then on every waiter of this and of the following launches drops too).  Nothing wrong has been added to the
// image: the launches since the last sync are launched again, one at a time on an idle device, in their order and with
// their own parameters; an item that was committed the first time finds its pixel's version ahead of it and is skipped.
static int replay_dropped(rene_ctx* c) {
  for (int attempt = 0; attempt < 3; ++attempt) {
    unsigned long long t[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(t, c->d_counters + 8, sizeof(t), hipMemcpyDeviceToHost));
    if (!t[0]) break;
    bool all = true;
    for (const rene_ctx::Pending& p : c->pending) all = all && p.replayable;
    if (!all) break;  // (the wavefront integrator's launches are not of this kind)
    if (std::getenv("RENE_DEBUG"))
      std::fprintf(stderr, "[rene] %llu work items were dropped (the first: %s): launching the last %zu launch(es), %u..%u, again, serially (attempt %d)\n", t[0], dropped_item(t).c_str(),
                   c->pending.size(), c->pending.front().epoch, c->pending.back().epoch, attempt + 1);
    HIP_TRY(c->zero_now(c->d_counters + 8, 4 * sizeof(unsigned long long)));
    for (rene_ctx::Pending& p : c->pending) {
      HIP_TRY(c->zero_now(c->d_work_counters, rene_ctx::kCounters * sizeof(uint32_t)));
      rene::RenderParams P = p.P;
      P.flags &= ~rene::RENE_FLAG_INTERNAL_TEST_DROP;
      rene::g_launched_blocks = p.cfg.grid;
      const auto tr = std::chrono::steady_clock::now();
      hipError_t e = rene::launch_render(p.cfg, c->view, P, c->stream);
      if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("render launch (replay): ") + hipGetErrorString(e));
      HIP_TRY(wait_stream(c->stream));
      c->kernel_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr).count();  // rene_stats.launches counts it too
      ++c->replays;
    }
    HIP_TRY(c->zero_now(c->d_work_counters, rene_ctx::kCounters * sizeof(uint32_t)));
  }
  return RENE_OK;
}

static int fold_pending(rene_ctx* c) {
  while (!c->pending.empty()) {
    rene_ctx::Pending& p = c->pending.front();
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, p.start, p.stop));
    if (std::getenv("RENE_DEBUG")) std::fprintf(stderr, "[rene] launch %u: %.3f ms\n", p.epoch, ms);
    c->kernel_ms += ms;
    c->last_ms = ms;
    c->pending.pop_front();
  }
  return RENE_OK;
}

// items still dropped after three replays on an idle device: something else is wrong, and every call that hands
// results to the caller (rene_sync, rene_download, rene_get_stats, rene_reduce) must say so
static int handoff_verdict(rene_ctx* c) {
  unsigned long long t[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(t, c->d_counters + 8, sizeof(t), hipMemcpyDeviceToHost));
  c->handoff_failed = t[0] != 0;
  if (c->handoff_failed) c->handoff_detail = " [" + std::to_string(t[0]) + " lanes gave up; the first: " + dropped_item(t) + "]";
  return RENE_OK;
}

// frame chains: the image handed out = the chains added in chain order (the chains go on accumulating)
static int resolve_image(rene_ctx* c) {
  const bool tiles = c->opts.shard_mode == RENE_SHARD_TILES;  // (a tile shard: only the tiles it owns are written)
  hipError_t e = rene::launch_resolve_chains(c->chains, c->fb, c->width, c->height, c->tiles_x, c->n_work, tiles ? c->opts.shard_rank : 0u, tiles ? c->opts.shard_count : 1u, c->stream);
  if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("resolve_chains: ") + hipGetErrorString(e));
  HIP_TRY(wait_stream(c->stream));
  c->fb_stale = false;
  return RENE_OK;
}

int rene_ctx::drain() {
  if (int rc = flush_exchange(); rc != RENE_OK) return rc;
  HIP_TRY(wait_stream(stream));
  const bool check_handoff = !pending.empty() && d_counters && !handoff_failed;
  if (counters_used && d_wave_times) report_wave_times(this);
  if (counters_used) {  // the stream is idle: the work counters can be handed out again
    HIP_TRY(zero_now(d_work_counters, kCounters * sizeof(uint32_t)));
    counters_used = 0;
  }
  if (check_handoff)
    if (int rc = replay_dropped(this); rc != RENE_OK) return rc;
  if (int rc = fold_pending(this); rc != RENE_OK) return rc;
  if (check_handoff)
    if (int rc = handoff_verdict(this); rc != RENE_OK) return rc;
  if (handoff_failed) return fail(RENE_ERR_DEVICE, "work items were dropped inside the render kernel and replaying their launches did not complete them (results invalid; rene_reset clears the condition)" + handoff_detail);
  return fb_stale ? resolve_image(this) : RENE_OK;
}

// No exception crosses the C boundary: the entry points that allocate host memory run under this guard.
template <class F>
static int guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(RENE_ERR_OUT_OF_MEMORY, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(RENE_ERR_DEVICE, std::string("unexpected exception: ") + e.what());
  }
}

// ---- what the passes over the frame chains share on the host (chain_pass.h is the device side) -----------------------------------------------------
static rene::TileGrid tile_grid(const rene_ctx* c) {
  const bool tiles = c->opts.shard_mode == RENE_SHARD_TILES && c->opts.shard_count > 1;
  return rene::TileGrid{c->width, c->height, c->tiles_x, c->n_work, tiles ? c->opts.shard_rank : 0u, tiles ? c->opts.shard_count : 1u};
}

// How rene_estimate_noise, rene_resolve_robust and rene_export_features begin, after the checks of their own arguments: the refusals they share,
// then `more` -- the caller's remaining checks, which still come before anything waits, launches or allocates -- then the device, the drain
// (waits for the launches issued so far and resolves the image) and the launch's geometry.
template <class More>
static int begin_chain_pass(const char* fn, rene_ctx* c, bool counts_u32, rene::TileGrid& G, More&& more) {
  if (c->opts.shard_mode != RENE_SHARD_TILES && c->opts.shard_count > 1)
    return fail(RENE_ERR_UNSUPPORTED, std::string(fn) + ": a frame shard (RENE_SHARD_FRAMES, shard_count > 1) holds only its share of every pixel's frames; use an unsharded context or tile shards");
  if (c->exchanged)
    return fail(RENE_ERR_UNSUPPORTED, std::string(fn) + ": the image has been through rene_reduce / rene_gather_tiles, which consumed the frame chains; rene_reset and render again");
  for (uint64_t f : c->chain_frames)
    if (counts_u32 && f > 0xffffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, std::string(fn) + ": a frame chain holds more than 2^32 - 1 frames");
  HIP_TRY(hipSetDevice(c->device));
  int rc = more();
  if (rc != RENE_OK) return rc;
  rc = c->drain();
  if (rc != RENE_OK) return rc;
  G = tile_grid(c);
  return RENE_OK;
}

// RENE_DEBUG: an event between every two launches of a call, so that its log says what each kernel took.  mark() records one on the stream
// (nothing where the variable is not set); ms(i, j) is the time between two of them once the stream has been waited for; `complete` says that
// every mark asked for is there.  The events go with the scope, whichever way the call leaves it.
struct Marks {
  const hipStream_t stream;
  const bool debug = std::getenv("RENE_DEBUG") != nullptr;
  bool complete = debug;
  std::vector<Event> events;
  explicit Marks(hipStream_t s) : stream(s) {}
  void mark() {
    if (!debug) return;
    Event ev;
    if (ev.create() != hipSuccess) {
      complete = false;
      return;
    }
    hipEventRecord(ev, stream);
    events.push_back(std::move(ev));
  }
  size_t size() const { return events.size(); }
  float ms(size_t i, size_t j) const {
    float t = 0.0f;
    hipEventElapsedTime(&t, events[i], events[j]);
    return t;
  }
};

// a launch that failed: what was enqueued before it runs to its end, then "<fn> launch: ..."
static int launch_failed(const std::string& fn, rene_ctx* c, hipError_t e) {
  hipStreamSynchronize(c->stream);
  return fail(RENE_ERR_DEVICE, fn + " launch: " + hipGetErrorString(e));
}

// One kernel launch and the wait for it.  RENE_DEBUG: a mark on either side of the launch, so that the log says what the kernel took (log(ms))
template <class Launch, class Log>
static int timed_launch(const char* fn, rene_ctx* c, Launch&& launch, Log&& log) {
  Marks M(c->stream);
  M.mark();
  const hipError_t e = launch();
  M.mark();
  if (e != hipSuccess) return launch_failed(fn, c, e);
  HIP_TRY(wait_stream(c->stream));
  if (M.complete) log(M.ms(0, 1));
  return RENE_OK;
}

// The caller's parameter struct where there is one -- its struct_size must be this build's -- else the defaults
template <class P>
static int read_params(const char* type, void (*defaults)(P*), const P* given, P& p) {
  defaults(&p);
  if (!given) return RENE_OK;
  if (given->struct_size != sizeof(P)) return fail(RENE_ERR_INVALID_ARGUMENT, std::string(type) + ".struct_size mismatch (ABI skew)");
  p = *given;
  return RENE_OK;
}
static int check_robust_params(const std::string& me, const rene_robust_params& p) {
  if (p.max_trim > 3u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": max_trim must be 0 .. 3");
  if (!std::isfinite(p.gain) || !(p.gain > 0.0f)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": gain must be finite and positive");
  return RENE_OK;
}

// the constants of the variance estimate for chains that have received cf[g] frames, in the order of a NoiseLaunch set (kernels.h): 1 / N, 1 / (k - 1),
// n_c / N, 1 / n_c; false: frames in fewer than two chains.  ONE piece of code for the denoiser, for the noise estimate of a uniform context and for
// every distinct N_t of an uneven one: a tile's constants are the same numbers either way.
static bool chain_constants(const uint64_t cf[rene::CHAINS], float out[rene::NOISE_SET_FLOATS], uint64_t* n_out = nullptr, uint32_t* k_out = nullptr) {
  uint64_t N = 0;
  uint32_t k = 0;
  for (uint32_t g = 0; g < rene::CHAINS; ++g) {
    N += cf[g];
    k += cf[g] ? 1u : 0u;
  }
  if (n_out) *n_out = N;
  if (k_out) *k_out = k;
  if (k < 2) return false;
  out[0] = 1.0f / (float)N;
  out[1] = 1.0f / (float)(k - 1u);
  for (uint32_t g = 0; g < rene::CHAINS; ++g) {
    out[2u + g] = cf[g] ? (float)cf[g] / (float)N : 0.0f;
    out[2u + rene::CHAINS + g] = cf[g] ? 1.0f / (float)cf[g] : 0.0f;
  }
  return true;
}

// Adaptive sampling, for the kernels that take one workgroup per owned tile: the distinct N_t of the owned tiles (at most one per change of the active
// tiles, plus one) and which of them every owned tile has.  A pass hands over one set of constants per distinct N_t, picked per tile.
static void distinct_tile_counts(const rene_ctx* c, std::vector<uint32_t>& counts, std::vector<uint32_t>& tile_set) {
  tile_set.resize(c->n_owned());
  for (uint32_t i = 0; i < c->n_owned(); ++i) {
    const uint32_t nt = c->tile_n(i);
    tile_set[i] = (uint32_t)(std::find(counts.begin(), counts.end(), nt) - counts.begin());
    if (tile_set[i] == counts.size()) counts.push_back(nt);
  }
}

// ... uploaded into the context's one pair of buffers before the call returns.  The stream is idle -- every caller has drained it, and uploads before
// it launches and waits for its kernel -- so no kernel is reading the table a call overwrites, and the passes can share the pair.
template <class T>
static int upload_tile_sets(rene_ctx* c, const std::vector<T>& sets, const std::vector<uint32_t>& tile_set, const T** sets_dev, const uint32_t** tile_set_dev) {
  const size_t bytes = sets.size() * sizeof(T);
  if (int rc = c->sets_dev.reserve(bytes, "tile sets"); rc != RENE_OK) return rc;
  if (int rc = c->tile_set_dev.reserve(tile_set.size() * sizeof(uint32_t), "tile sets"); rc != RENE_OK) return rc;
  HIP_TRY(hipMemcpy(c->sets_dev.p, sets.data(), bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->tile_set_dev.p, tile_set.data(), tile_set.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  *sets_dev = c->sets_dev.as<const T>();
  *tile_set_dev = c->tile_set_dev.as<const uint32_t>();
  return RENE_OK;
}

// the chain counts the robust resolve and the feature export are launched with: the context's, and on uneven tiles every distinct N_t's
static int fill_chain_counts(rene_ctx* c, rene::ChainCounts& C) {
  for (uint32_t g = 0; g < rene::CHAINS; ++g) C.chain_n[g] = (uint32_t)c->chain_frames[g];
  if (!c->uneven()) return RENE_OK;
  std::vector<uint32_t> counts, tile_set, sets;
  distinct_tile_counts(c, counts, tile_set);
  for (uint32_t nt : counts) {
    uint64_t cf[rene::CHAINS];
    rene_ctx::chain_counts(c->frame_base, nt, cf);
    for (uint64_t f : cf) sets.push_back((uint32_t)f);
  }
  return upload_tile_sets(c, sets, tile_set, &C.sets, &C.tile_set);
}

// the records of the owned tiles on the image's full tile grid (tiles the context does not own: zero)
template <class T>
static void scatter_owned_tiles(const rene_ctx* c, const std::vector<T>& owned, std::vector<T>& grid) {
  grid.assign(c->n_tiles, T{});
  for (uint32_t k = 0; k < owned.size(); ++k)
    if (c->owned_tile(k) < c->n_tiles) grid[c->owned_tile(k)] = owned[k];
}

// One image from the device to the caller: `src` holds [H][W][floats_per_pixel], `dst` receives [H][W][channels] -- the record's first three lanes, as the
// fourth the record's own or (zero_alpha) 0; one channel: lane `lane` alone.  `fix`, where there is one, edits the staged records before they are
// repacked.  Through a pinned staging buffer the context keeps: a copy into pageable memory makes the runtime pin and unpin the destination's pages
// on the fly (a registration of user memory with the driver per call)
static int staged_download(rene_ctx* c, const float* src, size_t floats_per_pixel, int channels, float* dst, bool zero_alpha = false, size_t lane = 0,
                           const std::function<void(float*)>& fix = nullptr) {
  const size_t n = (size_t)c->width * c->height;
  if (int rc = c->h_stage.reserve(n * 4 * sizeof(float), "download staging"); rc != RENE_OK) return rc;  // (a layer, whichever part of it is asked for)
  HIP_TRY(hipMemcpy(c->h_stage.p, src, n * floats_per_pixel * sizeof(float), hipMemcpyDeviceToHost));
  float* tmp = c->h_stage.as<float>();
  if (fix) fix(tmp);
  if ((size_t)channels == floats_per_pixel && !zero_alpha) {
    std::memcpy(dst, tmp, n * floats_per_pixel * sizeof(float));
    return RENE_OK;
  }
  if (channels == 1) {
    for (size_t i = 0; i < n; ++i) dst[i] = tmp[floats_per_pixel * i + lane];
    return RENE_OK;
  }
  for (size_t i = 0; i < n; ++i) {  // f32_4_to_3, rene/src/main.rs:1749-1756
    float* d = dst + (size_t)channels * i;
    d[0] = tmp[4 * i];
    d[1] = tmp[4 * i + 1];
    d[2] = tmp[4 * i + 2];
    if (channels == 4) d[3] = 0.0f;
  }
  return RENE_OK;
}

// The accessors of a library-owned result (Result): `fn` is the call's name, `none` what it says where no producing call has left one.
// <result>_buffer: the device pointer and the bytes (n_optional: a NULL n_bytes is allowed)
static int result_buffer(const char* fn, rene_ctx* c, Result rene_ctx::*result, const char* none, void** device_ptr, size_t* n_bytes, bool n_optional = false) {
  if (!c || !device_ptr || (!n_bytes && !n_optional)) return fail(RENE_ERR_INVALID_ARGUMENT, std::string(fn) + ": NULL argument");
  const Result& r = c->*result;
  if (!r.valid) return fail(RENE_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + none);
  *device_ptr = r.buf.p;
  if (n_bytes) *n_bytes = r.bytes;
  return RENE_OK;
}
// rene_download_<result>: its bytes into the caller's memory (`small`: what the call says of a destination that is too small).  staged: through the
// pinned staging, as the image downloads go.  The feature tensor and the packed shard are copied straight into the caller's pages instead: measured on
// 1920 x 1080, 21 calls into one reused array each way, medians in ms straight / staged (profiles/result_download_ab.json): 74.6 MB of features 1.34 /
// 4.44, 141.0 MB of features 2.52 / 8.31, a 108.6 MB shard 1.94 / 6.42
static int result_download(const char* fn, rene_ctx* c, Result rene_ctx::*result, const char* none, const char* small, bool staged, void* dst, size_t dst_bytes) {
  if (!c || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, std::string(fn) + ": NULL argument");
  const Result& r = c->*result;
  if (!r.valid) return fail(RENE_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + none);
  if (dst_bytes < r.bytes) return fail(RENE_ERR_INVALID_ARGUMENT, std::string(fn) + ": " + small);
  HIP_TRY(hipSetDevice(c->device));
  if (staged) return c->staged_fetch(dst, r.buf.p, r.bytes);
  HIP_TRY(hipMemcpy(dst, r.buf.p, r.bytes, hipMemcpyDeviceToHost));
  return RENE_OK;
}
static const char kNoShard[] = "no rene_denoise_shard_prepare since the context was created or reset";
static const char kNoFeatures[] = "no rene_export_features into the library's buffer since the context was created or reset";
static const char kNoOutput[] = "no rene_output_8bit into the library's buffer since the context was created or reset";
static const char kNoGbuffer[] = "no rene_gbuffer into the library's buffer since the context was created";
static const char kNoOcclusion[] = "no rene_occlusion into the library's buffer since the context was created";
static const char kNoDirect[] = "no rene_direct into the library's buffer since the context was created";
static const char kNoBounces[] = "no rene_bounces into the library's buffer since the context was created";
static const char kNoLights[] = "no rene_lights into the library's buffer since the context was created";

// A caller's destination, before anything is launched: `need` bytes (`need_is`: what they are the product of) behind an address aligned to `align`, in
// device memory of `device`, with dst_bytes inside its allocation -- a host pointer (which the runtime does not know, or knows as host memory)
// must never reach a kernel
static int check_device_destination(const std::string& me, int device, const void* device_dst, size_t dst_bytes, size_t need, const char* need_is, size_t align,
                                    const char* align_is) {
  if (dst_bytes < need) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than " + need_is);
  if (reinterpret_cast<uintptr_t>(device_dst) % align) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the destination is not " + align_is);
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, device_dst) != hipSuccess) {
    (void)hipGetLastError();  // (the runtime's sticky-until-read error)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the destination is not memory the HIP runtime knows (a host pointer?)");
  }
  if (attr.type != hipMemoryTypeDevice) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the destination is not device memory");
  if (attr.device != device) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the destination is on another device than the context");
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(device_dst)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the destination's allocation cannot be queried");
  }
  const size_t behind = size - (size_t)(static_cast<const char*>(device_dst) - static_cast<const char*>(base));
  if (static_cast<const char*>(device_dst) < static_cast<const char*>(base) || behind > size || dst_bytes > behind)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes reaches past the end of the destination's allocation");
  return RENE_OK;
}
static const char kImageBytes[] = "height x width x bytes per pixel";

// Every table of the scene that a context holds on the device, in upload order: f(the packed vector, where the SceneView keeps its pointer).
// rene_plan_memory sizes them and rene_create uploads them over this one list (the Uniforms record is made up by rene_create and follows them).
template <class F>
static int for_each_scene_table(const rene::PackedScene& ps, rene::SceneView& v, F&& f) {
  int rc = RENE_OK;
  auto one = [&](const auto& vec, auto& field) {
    if (rc == RENE_OK) rc = f(vec, field);
  };
  one(ps.main.nodes, v.main.nodes), one(ps.main.isect, v.main.isect), one(ps.emit.nodes, v.emit.nodes), one(ps.emit.isect, v.emit.isect);
  one(ps.main.items, v.main.items), one(ps.emit.items, v.emit.items), one(ps.shade, v.shade), one(ps.emit_pdf, v.emit_pdf);
  one(ps.spheres, v.spheres), one(ps.insts, v.insts), one(ps.emit_objects, v.emit_objects), one(ps.emit_tris, v.emit_tris);
  one(ps.materials, v.materials), one(ps.textures, v.textures), one(ps.lights, v.lights), one(ps.mediums, v.mediums);
  one(ps.inst_medium, v.inst_medium), one(ps.images, v.images), one(ps.image_pool, v.image_pool), one(ps.small_image, v.small_image);
  return rc;
}

// A probe's round trip on `stream`: device buffers for the call's inputs and outputs -- local, freed whichever way the call ends -- the inputs copied
// in, launch(d) with d[i] the device copy of the i-th of the inputs and then the outputs, the outputs copied back, the wait; any HIP error is the
// call's "<name>: ..." device error.
using ProbeIn = std::pair<const void*, size_t>;  // host pointer, bytes
using ProbeOut = std::pair<void*, size_t>;
template <class Launch>
static int run_probe(const char* name, hipStream_t stream, std::initializer_list<ProbeIn> ins, std::initializer_list<ProbeOut> outs, Launch&& launch) {
  std::vector<DevBuf> bufs(ins.size() + outs.size());
  std::vector<void*> d;
  hipError_t e = hipSuccess;
  auto alloc = [&](size_t bytes) {
    if (e == hipSuccess) e = bufs[d.size()].grow(bytes);
    d.push_back(bufs[d.size()].p);
  };
  for (const ProbeIn& in : ins) alloc(in.second);
  for (const ProbeOut& out : outs) alloc(out.second);
  size_t i = 0;
  for (const ProbeIn& in : ins) {
    if (e == hipSuccess) e = hipMemcpyAsync(d[i], in.first, in.second, hipMemcpyHostToDevice, stream);
    ++i;
  }
  if (e == hipSuccess) e = launch(d.data());
  for (const ProbeOut& out : outs) {
    if (e == hipSuccess) e = hipMemcpyAsync(out.first, d[i], out.second, hipMemcpyDeviceToHost, stream);
    ++i;
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(e));
  return RENE_OK;
}

// ---- the per-pixel frame-range passes (pixel_pass.h): what rene_gbuffer, rene_occlusion, rene_direct, rene_bounces and rene_lights and their probes share on the host
// One pass over frames first_frame .. first_frame + n_frames - 1 into the caller's device destination or, without one, the library's `result`:
// [H][W] records of record_bytes each.  The frames' seeds go to the device through pass_seeds, which the five passes share; launch(seeds on the
// device, destination) builds the pass's launch struct and launches; log(ms) is the RENE_DEBUG line.  The caller has checked its parameters and c.
template <class Launch, class Log>
static int run_pixel_pass(const std::string& me, rene_ctx* c, uint32_t first_frame, uint32_t n_frames, size_t record_bytes, Result rene_ctx::*result, void* device_dst,
                          size_t dst_bytes, Launch&& launch, Log&& log) {
  const size_t need = (size_t)c->width * c->height * record_bytes;
  HIP_TRY(hipSetDevice(c->device));
  if (device_dst)
    if (int rc = check_device_destination(me, c->device, device_dst, dst_bytes, need, kImageBytes, 16, "16-byte aligned"); rc != RENE_OK) return rc;
  if (need == 0) return RENE_OK;  // (an empty film)
  std::vector<uint32_t> seeds(n_frames);
  rene_frame_seeds(c->opts.seed, first_frame, n_frames, seeds.data());
  HIP_TRY(wait_stream(c->stream));  // (a pass in flight reads the seeds this call overwrites)
  if (int rc = c->pass_seeds.reserve(seeds.size() * sizeof(uint32_t), me + " seeds"); rc != RENE_OK) return rc;
  void* dst = device_dst;
  if (!device_dst)
    if (int rc = (c->*result).begin(need, {}, c->stream, me + " buffer", dst); rc != RENE_OK) return rc;  // (zeroed below, like a caller's destination)
  HIP_TRY(hipMemcpyAsync(c->pass_seeds.p, seeds.data(), seeds.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(wait_stream(c->stream));  // (`seeds` is pageable memory of this scope)
  // the pixels of tiles the context does not own are the all-zero record.  On the context's stream, ahead of the kernel
  HIP_TRY(hipMemsetAsync(dst, 0, need, c->stream));
  const int rc = timed_launch(me.c_str(), c, [&] { return launch(c->pass_seeds.as<uint32_t>(), dst); }, log);
  if (rc != RENE_OK) return rc;
  if (!device_dst) (c->*result).commit(need);
  return RENE_OK;
}

// A pass's per-sample probe into host memory: [n_frames][per_frame][H][W] records of record_bytes each, at most 2^cap_log2 of them (`noun` and
// `operands` word the two refusals); launch as above, with the probe's own device buffers.  The caller has checked its parameters, c and host_dst.
template <class Launch>
static int run_pixel_pass_samples(const std::string& me, rene_ctx* c, uint32_t first_frame, uint32_t n_frames, size_t per_frame, size_t record_bytes, unsigned cap_log2,
                                  const char* noun, const char* operands, void* host_dst, size_t n, Launch&& launch) {
  const size_t n_px = (size_t)c->width * c->height, need = n_px * n_frames * per_frame;
  if (need > ((size_t)1 << cap_log2))
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": more than 2^" + std::to_string(cap_log2) + " " + noun + " (" + operands + "); ask for fewer frames");
  if (n < need) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n is smaller than " + operands);
  if (need == 0) return RENE_OK;
  std::vector<uint32_t> seeds(n_frames);
  rene_frame_seeds(c->opts.seed, first_frame, n_frames, seeds.data());
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = need * record_bytes;
  return run_probe(me.c_str(), c->stream, {{seeds.data(), seeds.size() * sizeof(uint32_t)}}, {{host_dst, bytes}}, [&](void* const* d) {
    const hipError_t e = hipMemsetAsync(d[1], 0, bytes, c->stream);  // the records of tiles the context does not own, and of the occlusion probe's primary misses
    if (e != hipSuccess) return e;
    return launch((const uint32_t*)d[0], d[1]);
  });
}

extern "C" {

const char* rene_last_error(void) { return g_error.c_str(); }
uint32_t rene_abi_version(void) { return RENE_ABI_VERSION; }

void rene_frame_seeds(uint32_t master_seed, uint32_t first_frame, uint32_t n, uint32_t* out) {
  HostPcg g(master_seed);
  g.skip(first_frame);
  for (uint32_t k = 0; k < n; ++k) out[k] = g.next();
}

// ---- the scene fingerprint (include/rene_hip.h, the checkpoint's section): the desc as a stream of uint32 words through two 64-bit lanes ----------
namespace {
struct Fingerprint {
  uint64_t a = 0x243F6A8885A308D3ull, b = 0x13198A2E03707344ull;
  void word(uint32_t s) {
    a = (a ^ s) * 0x00000100000001B3ull;
    b = (((b << 27) | (b >> 37)) + s) * 0x9E3779B97F4A7C15ull;
  }
  void words(const void* p, size_t n) {  // n words of a table whose records are 4-byte fields without padding
    const unsigned char* q = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) {
      uint32_t s;
      std::memcpy(&s, q + 4 * i, 4);
      word(s);
    }
  }
  static uint64_t finish(uint64_t h) {
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    return h;
  }
};
static_assert(sizeof(rene_uniform) == 53 * 4 && sizeof(rene_instance) == 18 * 4 && sizeof(rene_vertex) == 8 * 4 && sizeof(rene_material) == 13 * 4 && sizeof(rene_texture) == 9 * 4 &&
                  sizeof(rene_area_light) == 5 * 4 && sizeof(rene_light) == 9 * 4 && sizeof(rene_medium) == 9 * 4,
              "the fingerprint reads the tables as words: their records have no padding");
}  // namespace
static int scene_fingerprint(const rene_scene_desc* d, uint64_t out[2]) {
  if (!d || !out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_scene_fingerprint: NULL argument");
  if (d->struct_size != sizeof(rene_scene_desc)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_scene_fingerprint: rene_scene_desc.struct_size mismatch (ABI skew)");
  if ((d->n_instances && !d->instances) || (d->n_meshes && !d->meshes) || (d->n_materials && !d->materials) || (d->n_textures && !d->textures) ||
      (d->n_area_lights && !d->area_lights) || (d->n_lights && !d->lights) || (d->n_images && !d->images) || (d->n_mediums && !d->mediums))
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_scene_fingerprint: a NULL table with a count above 0");
  Fingerprint f;
  f.word(d->integrator), f.word(d->xresolution), f.word(d->yresolution);
  f.words(&d->uniform, 53);
  for (uint32_t n : {d->n_instances, d->n_meshes, d->n_materials, d->n_textures, d->n_area_lights, d->n_lights, d->n_images, d->n_mediums}) f.word(n);
  f.words(d->instances, (size_t)d->n_instances * 18);
  for (uint32_t m = 0; m < d->n_meshes; ++m) {
    const rene_mesh& mesh = d->meshes[m];
    if ((mesh.n_vertices && !mesh.vertices) || (mesh.n_indices && !mesh.indices)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_scene_fingerprint: a NULL table with a count above 0");
    f.word(mesh.n_vertices), f.word(mesh.n_indices);
    f.words(mesh.vertices, (size_t)mesh.n_vertices * 8);
    f.words(mesh.indices, mesh.n_indices);
  }
  f.words(d->materials, (size_t)d->n_materials * 13);
  f.words(d->textures, (size_t)d->n_textures * 9);
  f.words(d->area_lights, (size_t)d->n_area_lights * 5);
  f.words(d->lights, (size_t)d->n_lights * 9);
  for (uint32_t i = 0; i < d->n_images; ++i) {
    const rene_image& im = d->images[i];
    const size_t n = (size_t)im.width * im.height * 4;
    if (n && !im.rgba) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_scene_fingerprint: a NULL table with a count above 0");
    f.word(im.width), f.word(im.height);
    f.words(im.rgba, n);
  }
  f.words(d->mediums, (size_t)d->n_mediums * 9);
  out[0] = Fingerprint::finish(f.a);
  out[1] = Fingerprint::finish(f.b);
  return RENE_OK;
}

static int rene_scene_pack_info_impl(const rene_scene_desc* scene, rene_pack_info* out) {
  if (!scene || !out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_scene_pack_info: NULL argument");
  rene::PackedScene ps;
  std::string err;
  int rc = rene::pack_scene(scene, ps, err);
  if (rc != RENE_OK) return fail(rc, err);
  std::memset(out, 0, sizeof(*out));
  out->n_instances = (uint32_t)ps.insts.size();
  out->n_triangles = ps.n_triangles;
  out->n_spheres = (uint32_t)ps.spheres.size();
  out->n_nodes_main = (uint32_t)ps.main.nodes.size();
  out->n_slots_main = (uint32_t)ps.main.isect.size();
  out->depth_main = ps.main.depth;
  out->n_nodes_emit = (uint32_t)ps.emit.nodes.size();
  out->n_slots_emit = (uint32_t)ps.emit.isect.size();
  out->depth_emit = ps.emit.depth;
  out->features = ps.features;
  out->emit_object_len = (uint32_t)ps.emit_objects.size();
  out->lights_len = (uint32_t)ps.lights.size();
  out->n_items_main = (ps.features & rene::FEAT_SMALL) ? ps.main.n_loop : 0u;
  out->n_items_emit = (ps.features & rene::FEAT_SMALL) ? ps.emit.n_loop : 0u;
  out->device_bytes = ps.main.nodes.size() * sizeof(rene::Node) + ps.main.isect.size() * sizeof(rene::PrimIsect) +
                      ps.emit.nodes.size() * sizeof(rene::Node) + ps.emit.isect.size() * sizeof(rene::PrimIsect) +
                      ps.shade.size() * sizeof(rene::PrimShade) + ps.emit_pdf.size() * sizeof(rene::EmitPdf) +
                      ps.spheres.size() * sizeof(rene::Sphere) + ps.insts.size() * sizeof(rene::Inst) +
                      ps.emit_objects.size() * sizeof(rene::EmitObject) + ps.emit_tris.size() * sizeof(rene::EmitTri) +
                      ps.materials.size() * sizeof(rene::Material) + ps.textures.size() * sizeof(rene::Texture) +
                      ps.lights.size() * sizeof(rene::Light) + ps.image_pool.size() * sizeof(float) +
                      ps.mediums.size() * sizeof(rene::Medium) + ps.inst_medium.size() * sizeof(rene::InstMedium);
  return RENE_OK;
}

static int rene_scene_small_items_impl(const rene_scene_desc* scene, int which, float* out, uint32_t cap_items, uint32_t* n_loop, uint32_t* n_total) {
  if (!scene || !n_loop || (cap_items && !out)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_scene_small_items: NULL argument");
  if (which != 0 && which != 1) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_scene_small_items: which must be 0 (main) or 1 (emitter)");
  rene::PackedScene ps;
  std::string err;
  int rc = rene::pack_scene(scene, ps, err);
  if (rc != RENE_OK) return fail(rc, err);
  const rene::BuiltAccel& acc = which == 0 ? ps.main : ps.emit;
  const bool small = (ps.features & rene::FEAT_SMALL) != 0;
  const size_t n = small ? acc.items.size() : 0;
  *n_loop = small ? acc.n_loop : 0u;
  if (n_total) *n_total = (uint32_t)n;
  const size_t take = std::min<size_t>(n, cap_items);
  if (take) std::memcpy(out, acc.items.data(), take * sizeof(rene::SmallItem));
  return RENE_OK;
}

// What a context of this scene and these options holds on the device, and every check rene_create makes on them before it allocates
// (rene_plan_memory: the same function, without a GPU).  Chains and versions are sized by the pixel slots of the owned tiles (device_scene.h).
namespace {
struct ContextPlan {
  rene_memory_plan bytes{};
  uint32_t tiles_x = 0, n_tiles = 0, n_slots = 0, features = 0, depth = 0, stack = 0;
  uint64_t owned_pixels = 0;
  bool wavefront = false;
  static constexpr uint32_t kWaveMaxLights = 4;  // shadow-ray slots of the wavefront integrator
  // wavefront queues, in allocation order: ro, rd, color, ctl, hit, sh_wi, sh_c, status, n_done, trace_counter, wave_sums
  static constexpr int kQueues = 11;
  size_t queue[kQueues] = {};
};
}  // namespace
static size_t fixed_bytes() { return rene_ctx::kCounters * sizeof(uint32_t) + 32 * sizeof(unsigned long long); }  // work counters, counters
static int read_opts(const rene_opts* opts, rene_opts& o) {
  o = rene_opts{};
  o.struct_size = sizeof(rene_opts);
  o.seed = RENE_DEFAULT_SEED;
  if (opts) {
    if (opts->struct_size != sizeof(rene_opts))
      return fail(RENE_ERR_INVALID_ARGUMENT, "rene_opts.struct_size mismatch (ABI skew)");
    o = *opts;
  }
  if (o.shard_count == 0) o.shard_count = 1;
  if (o.shard_rank >= o.shard_count) return fail(RENE_ERR_INVALID_ARGUMENT, "shard_rank >= shard_count");
  if (o.shard_mode > RENE_SHARD_FRAMES) return fail(RENE_ERR_INVALID_ARGUMENT, "unknown shard_mode");
  return RENE_OK;
}
static int plan_context(const rene::PackedScene& ps, const rene_opts& o, ContextPlan& m) {
  m = ContextPlan{};
  if (ps.width > rene::MAX_RESOLUTION || ps.height > rene::MAX_RESOLUTION)  // a lane keeps its pixel and chain as x | y << 14 | chain << 28
    return fail(RENE_ERR_INVALID_ARGUMENT, "resolutions above 16384 are not supported");
  for (int i = 0; i < 16; ++i)  // the kernels read the camera's origin off the matrix instead of multiplying a zero point through it
    if (!std::isfinite(ps.uniform.camera_to_world[i]) || !std::isfinite(ps.uniform.projection_inv[i]))
      return fail(RENE_ERR_INVALID_ARGUMENT, "rene_uniform: camera_to_world / projection_inv must be finite");
  // traversal stack: enough for the deeper of the two trees, in LDS, [depth][256 lanes]
  m.depth = std::max(ps.main.depth, ps.emit.depth);
  m.stack = 16;
  while (m.stack < m.depth) m.stack += 4;  // 40 entries x 1024 lanes x 4 B = the whole 160 KB of a CU at 4 waves per SIMD
  if (m.stack > 96) return fail(RENE_ERR_UNSUPPORTED, "BVH deeper than the 96-entry traversal stack");
  // (occupancy experiments: RENE_STACK_ENTRIES may only GROW the stack -- a stack shallower than the tree's worst case would let a deep query write
  // past its column into other lanes' entries and the LDS tables: refused)
  if (const char* e = std::getenv("RENE_STACK_ENTRIES")) {
    const int want = std::atoi(e);
    if (want < (int)m.depth) return fail(RENE_ERR_INVALID_ARGUMENT, "RENE_STACK_ENTRIES is below the traversal stack this scene's BVH can need (" + std::to_string(m.depth) + " entries)");
    m.stack = (uint32_t)std::min(96, want);
  }
  m.features = ps.features;
  if (o.flags & RENE_FLAG_FORCE_BVH) m.features &= ~rene::FEAT_SMALL;

  m.tiles_x = (ps.width + RENE_TILE_SIZE - 1) / RENE_TILE_SIZE;
  const uint32_t tiles_y = (ps.height + RENE_TILE_SIZE - 1) / RENE_TILE_SIZE;
  m.n_tiles = m.tiles_x * tiles_y;
  uint32_t tile_rank = 0, tile_count = 1;
  if (o.shard_mode == RENE_SHARD_TILES) {
    tile_rank = o.shard_rank;
    tile_count = o.shard_count;
  }
  const uint32_t owned = owned_tiles(m.n_tiles, tile_rank, tile_count);
  // (at most 2^18 tiles of 1024 slots: a level's work ids, slots x CHAINS, stay within 2^31; the kernels hand them out in batches that
  // never straddle a level, device_code.inc batch_decode, so levels x ids need not fit 32 bits)
  m.n_slots = owned * rene::TILE_SLOTS;
  // pixels of the image inside the owned tiles: paths per rendered frame (the kernels do not count what the host knows)
  for (uint32_t t = tile_rank; t < m.n_tiles; t += tile_count) {
    const uint32_t x0 = (t % m.tiles_x) * RENE_TILE_SIZE, y0 = (t / m.tiles_x) * RENE_TILE_SIZE;
    m.owned_pixels += (uint64_t)std::min<uint32_t>(RENE_TILE_SIZE, ps.width - x0) * std::min<uint32_t>(RENE_TILE_SIZE, ps.height - y0);
  }
  // Which integrator renders this scene: the item-loop megakernel (small scenes), the volpath megakernel,
  // or -- for everything that needs the BVH -- the traversal-restart megakernel; RENE_FLAG_WAVEFRONT selects
  // the stage-separated wavefront (wavefront.inc) instead, unless the scene has more distant lights than
  // it keeps shadow-ray slots for.
  m.wavefront = !(m.features & (rene::FEAT_SMALL | rene::FEAT_VOLPATH)) && (o.flags & RENE_FLAG_WAVEFRONT) && !(o.flags & RENE_FLAG_NO_RESTART) &&
                ps.lights.size() <= ContextPlan::kWaveMaxLights && m.n_slots > 0;
  if (m.wavefront) {
    const size_t n = m.n_slots, lights = ps.lights.size();
    const size_t q[ContextPlan::kQueues] = {n * 16, n * 16, n * 16, n * 16, n * 16, n * 16 * lights, n * 16 * lights, n * 4, 4, 8, ((n + 255) / 256) * 4 * 8 * sizeof(unsigned long long)};
    for (int i = 0; i < ContextPlan::kQueues; ++i) {
      m.queue[i] = std::max<size_t>(16, q[i]);
      m.bytes.queue_bytes += m.queue[i];
    }
  }
  m.bytes.chain_bytes = (uint64_t)rene::CHAINS * 3u * m.n_slots * 4u * sizeof(float);
  m.bytes.version_bytes = (uint64_t)rene::CHAINS * m.n_slots * sizeof(uint32_t);
  m.bytes.image_bytes = o.framebuffer ? 0u : (uint64_t)3u * ps.width * ps.height * 4u * sizeof(float);
  uint64_t scene = 0;
  rene::SceneView nowhere{};
  for_each_scene_table(ps, nowhere, [&](const auto& v, auto&) {  // rene_ctx::upload
    scene += std::max<size_t>(1, v.size()) * sizeof(v[0]);
    return RENE_OK;
  });
  scene += sizeof(rene::Uniforms);
  m.bytes.scene_bytes = scene;
  m.bytes.total_bytes = m.bytes.chain_bytes + m.bytes.version_bytes + m.bytes.image_bytes + m.bytes.scene_bytes + m.bytes.queue_bytes + fixed_bytes();
  return RENE_OK;
}

static int rene_plan_memory_impl(const rene_scene_desc* scene, const rene_opts* opts, rene_memory_plan* out) {
  if (!scene || !out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_plan_memory: NULL argument");
  rene_opts o;
  int rc = read_opts(opts, o);
  if (rc != RENE_OK) return rc;
  rene::PackedScene ps;
  std::string err;
  rc = rene::pack_scene(scene, ps, err);
  if (rc != RENE_OK) return fail(rc, err);
  ContextPlan m;
  rc = plan_context(ps, o, m);
  if (rc != RENE_OK) return rc;
  *out = m.bytes;
  return RENE_OK;
}

static int rene_create_impl(const rene_scene_desc* scene, const rene_opts* opts, rene_ctx** out) {
  if (!scene || !out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_create: NULL argument");
  *out = nullptr;
  rene_opts o;
  int rc = read_opts(opts, o);
  if (rc != RENE_OK) return rc;

  rene::PackedScene ps;
  std::string err;
  rc = rene::pack_scene(scene, ps, err);
  if (rc != RENE_OK) return fail(rc, err);
  uint64_t fingerprint[2];  // of the tables as they were received (a checkpoint carries it)
  rc = scene_fingerprint(scene, fingerprint);
  if (rc != RENE_OK) return rc;

  int n_dev = 0;
  HIP_TRY(hipGetDeviceCount(&n_dev));
  if (n_dev <= 0) return fail(RENE_ERR_DEVICE, "no HIP device visible (the render path has no CPU fallback)");
  if (o.device < 0 || o.device >= n_dev) return fail(RENE_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  HIP_TRY(hipSetDevice(o.device));
  ContextPlan m;  // the checks and the sizes of everything allocated below (rene_plan_memory)
  rc = plan_context(ps, o, m);
  if (rc != RENE_OK) return rc;

  std::unique_ptr<rene_ctx, void (*)(rene_ctx*)> c(new rene_ctx(), rene_destroy);  // (a failure below destroys what there is by then)
  c->device = o.device;
  c->opts = o;
  c->width = ps.width;
  c->height = ps.height;
  c->n_materials = (uint32_t)ps.materials.size();
  c->n_mediums = (uint32_t)ps.mediums.size();  // 0 unless the integrator is volpath
  c->fingerprint[0] = fingerprint[0];
  c->fingerprint[1] = fingerprint[1];

  if (o.stream) {
    c->stream = static_cast<hipStream_t>(o.stream);
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }

  rene::SceneView& v = c->view;
  rc = for_each_scene_table(ps, v, [&](const auto& vec, auto& field) { return c->upload(vec, &field); });
  if (rc != RENE_OK) return rc;
  v.main.n_top = ps.main.n_top;
  v.emit.n_top = ps.emit.n_top;
  v.main.n_items = ps.main.n_loop;  // the loop's items; the auxiliary records of box items follow them
  v.emit.n_items = ps.emit.n_loop;
  v.main.n_nodes = (uint32_t)ps.main.nodes.size();
  v.main.n_slots = (uint32_t)ps.main.isect.size();
  v.emit.n_nodes = (uint32_t)ps.emit.nodes.size();
  v.emit.n_slots = (uint32_t)ps.emit.isect.size();
  c->inst_material.clear();
  for (const rene::Inst& in : ps.insts) c->inst_material.push_back(in.material);
  c->inst_emits.clear();
  for (const rene::Inst& in : ps.insts) c->inst_emits.push_back(in.emit[3] != 0.0f ? 1 : 0);
  v.small_bytes = (uint32_t)(ps.small_image.size() * sizeof(float));
  for (uint32_t k = 0; k < rene::SMALL_OFF_COUNT; ++k) v.small_off[k] = ps.small_off[k];
  {
    std::vector<rene::Uniforms> u(1);
    std::memset(&u[0], 0, sizeof(u[0]));
    std::memcpy(u[0].c2w, ps.uniform.camera_to_world, 64);
    std::memcpy(u[0].proj_inv, ps.uniform.projection_inv, 64);
    std::memcpy(u[0].bg_matrix, ps.uniform.background_matrix, 64);
    std::memcpy(u[0].bg_color, ps.uniform.background_color, 16);
    u[0].bg_kind = 0;
    if (ps.uniform.background_texture < ps.textures.size() && !std::getenv("RENE_NO_RESOLVE")) {
      const rene::Texture& t = ps.textures[ps.uniform.background_texture];
      if (t.type == RENE_TEXTURE_SOLID) {
        u[0].bg_kind = 1;
        std::memcpy(u[0].bg_solid, t.v0, 12);
      } else if (t.type == RENE_TEXTURE_IMAGEMAP && t.u0[0] < ps.images.size()) {
        u[0].bg_kind = 2;
        u[0].bg_image_offset = ps.images[t.u0[0]].offset;
        u[0].bg_image_width = ps.images[t.u0[0]].width;
        u[0].bg_image_height = ps.images[t.u0[0]].height;
      }
    }
    int rc_ = c->upload(u, &v.uni);
    if (rc_ != RENE_OK) return rc_;
  }
  v.bg_texture = ps.uniform.background_texture;
  v.lights_len = (uint32_t)ps.lights.size();                // rene/src/scene.rs:166
  v.emit_object_len = (uint32_t)ps.emit_objects.size();     // rene/src/main.rs:3279
  v.width = ps.width;
  v.height = ps.height;

  c->cfg.features = m.features;
  c->cfg.stack_depth = m.stack;
  c->cfg.n_insts = (uint32_t)ps.insts.size();
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, o.device));
  c->cfg.grid = (uint32_t)prop.multiProcessorCount * 8u;  // persistent launch: upper bound, clamped to the co-resident blocks at launch
  c->cfg.cus = (uint32_t)prop.multiProcessorCount;
  if (const char* e = std::getenv("RENE_BLOCKS_PER_CU")) {  // tuning knob (experiments only)
    int b = std::atoi(e);
    if (b > 0 && b <= 64) c->cfg.grid = (uint32_t)prop.multiProcessorCount * (uint32_t)b;
  }

  c->tiles_x = m.tiles_x;
  c->n_tiles = m.n_tiles;
  c->n_work = m.n_slots;
  c->owned_pixels = m.owned_pixels;
  c->fb_floats = (size_t)3 * ps.width * ps.height * 4;
  // every allocation of the context that a job needs, or the call's return code
#define RESERVE(buf, bytes, what)                                                          \
  do {                                                                                     \
    if (int rc_ = (buf).reserve(bytes, "rene_create: " what); rc_ != RENE_OK) return rc_; \
  } while (0)
  RESERVE(c->chains, std::max<size_t>(16, m.bytes.chain_bytes), "frame chains");  // over the owned pixel slots (device_scene.h)
  if (o.framebuffer) {
    c->fb = static_cast<float*>(o.framebuffer);
  } else {
    RESERVE(c->fb_own, m.bytes.image_bytes, "image");
    c->fb = c->fb_own.as<float>();
  }
  c->cfg.wave_stack = std::max(1u, m.depth);
  c->wavefront = m.wavefront;
  if (c->wavefront) {
    rene::WaveState& q = c->wave;
    q.n_slots = c->n_work;
    q.max_lights = (uint32_t)ps.lights.size();
    q.fp16_payload = (o.flags & RENE_FLAG_FP16_PAYLOAD) ? 1u : 0u;
    void** dst[ContextPlan::kQueues] = {reinterpret_cast<void**>(&q.ro), reinterpret_cast<void**>(&q.rd), reinterpret_cast<void**>(&q.color), reinterpret_cast<void**>(&q.ctl),
                                        reinterpret_cast<void**>(&q.hit), reinterpret_cast<void**>(&q.sh_wi), reinterpret_cast<void**>(&q.sh_c), reinterpret_cast<void**>(&q.status),
                                        reinterpret_cast<void**>(&q.n_done), reinterpret_cast<void**>(&q.trace_counter), reinterpret_cast<void**>(&q.wave_sums)};
    for (int i = 0; i < ContextPlan::kQueues; ++i) {
      RESERVE(c->allocations.emplace_back(), m.queue[i], "wavefront queues");
      *dst[i] = c->allocations.back().p;
    }
    RESERVE(c->h_done, sizeof(uint32_t), "wavefront done word");
  }
  RESERVE(c->d_work_counters, rene_ctx::kCounters * sizeof(uint32_t), "work counters");
  HIP_TRY(hipMemsetAsync(c->d_work_counters, 0, rene_ctx::kCounters * sizeof(uint32_t), c->stream));
  RESERVE(c->d_counters, 32 * sizeof(unsigned long long), "counters");
  RESERVE(c->d_item_done, std::max<size_t>(16, m.bytes.version_bytes), "versions");  // one version word per pixel slot and chain
#undef RESERVE
  HIP_TRY(hipMemsetAsync(c->d_item_done, 0, m.bytes.version_bytes, c->stream));
  HIP_TRY(hipMemsetAsync(c->chains, 0, m.bytes.chain_bytes, c->stream));  // main.rs:1229-1237
  HIP_TRY(hipMemsetAsync(c->fb, 0, c->fb_floats * sizeof(float), c->stream));
  HIP_TRY(hipMemsetAsync(c->d_counters, 0, 32 * sizeof(unsigned long long), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipDeviceSynchronize());  // everything the uploads left on the null stream (the fills of empty tables) has run: see zero_now

  c->h_upload.release();
  // tests: start the launch numbering just below the wrap of the 22-bit epoch (MAX_EPOCH), so that a handful of launches cross it
  if (const char* e = std::getenv("RENE_TEST_EPOCH")) c->epoch = (uint32_t)std::min<unsigned long>(rene::MAX_EPOCH, std::strtoul(e, nullptr, 0));
  *out = c.release();
  return RENE_OK;
}

void rene_destroy(rene_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->comm && rccl()->handle) rccl()->CommDestroy(c->comm);
  if (c->state_stream) {
    hipStreamSynchronize(c->state_stream);
    hipStreamDestroy(c->state_stream);
  }
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  delete c;  // (with it its memory and the events of launches never drained: the device is selected above, the stream has run dry)
}

static int rene_render_impl(rene_ctx* c, uint32_t first_frame, uint32_t n_frames) {
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_render: NULL context");
  if (c->loaded) return fail(RENE_ERR_UNSUPPORTED, "rene_render: the frame chains were put there by rene_load_chains (their version words do not describe them); rene_reset before rendering");
  if (n_frames == 0) return RENE_OK;
  if (c->exchanged) return fail(RENE_ERR_INVALID_ARGUMENT, "the image has been through rene_reduce / rene_gather_tiles: rene_reset before rendering again");
  if ((uint64_t)first_frame + n_frames > 0xffffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, "frame range overflows u32");
  if (n_frames > rene::MAX_LAUNCH_FRAMES) {  // one launch renders at most this many frames (its seed tables)
    for (uint32_t done = 0; done < n_frames;) {
      const uint32_t n = std::min(rene::MAX_LAUNCH_FRAMES, n_frames - done);
      int rc = rene_render_impl(c, first_frame + done, n);
      if (rc != RENE_OK) return rc;
      done += n;
    }
    return RENE_OK;
  }
  if (c->n_inactive) {  // adaptive sampling: tiles are switched off
    if (c->n_inactive == c->n_owned()) return RENE_OK;  // all of them: nothing to launch, nothing to count
    if (first_frame != c->frame_base + c->frames)
      return fail(RENE_ERR_INVALID_ARGUMENT, "rene_render: tiles are switched off (rene_set_active_tiles): first_frame must continue the frames rendered so far, at " +
                                                 std::to_string(c->frame_base + c->frames) + ", so that every tile's frames stay one range (rene_reset starts again)");
  }
  HIP_TRY(hipSetDevice(c->device));
  // Plan, launch, commit: everything down to the launch reads the context and fills locals -- the launch's plan (launch_plan.h), its RenderParams, its
  // Pending record; the context's counts are written once, when the launch has been issued.  (What waits or allocates on the way -- the three drains,
  // the frame-stream table, the RENE_DEBUG wave times -- leaves the counts alone.)
  const rene::FrameShare share = rene::frame_share(first_frame, n_frames, c->opts.shard_mode, c->opts.shard_rank, c->opts.shard_count);
  // the Matte small-scene kernels read the frame-wide sample stream from a table of the launch's frames (grown here, before anything is counted)
  const bool frame_stream = !c->wavefront && share.count != 0 && c->n_work != 0 && rene::select_kernel(c->cfg, c->view, c->opts.flags).reads_frame_stream;
  if (frame_stream) {
    int rc = c->frame_stream_reserve(share.count);
    if (rc != RENE_OK) return rc;
  }
  // the request's frames into the context's counts -- also where none of them is this context's, or it owns no pixel: nothing is launched then
  const auto count_frames = [&] {
    if (c->frames == 0) c->frame_base = first_frame;
    else if (first_frame != c->frame_base + c->frames) c->frames_contiguous = false;
    c->frames += n_frames;
    c->count_chain_frames(share.chain_phase(), share.count);
  };
  if (share.count == 0 || c->n_work == 0) {
    count_frames();
    return RENE_OK;
  }
  const uint64_t launch_paths = (uint64_t)share.count * (c->owned_pixels - c->inactive_pixels);  // the paths of the active tiles

  if (c->epoch >= rene::MAX_EPOCH) {  // the hand-off flags are cleared when the epoch wraps: nothing may be in flight then
    int rc = c->drain();
    if (rc != RENE_OK) return rc;
  }
  // A launch is a kernel launch between two event records -- no allocation, no copy, no memset: those need a copy engine
  // or a free CU slot, which a persistent launch that holds the chip gives up only when it ends.  Hence the pool of work
  // counters (zeroed again in drain()) instead of one that is reset per launch.
  if (c->counters_used >= rene_ctx::kCounters) {
    int rc = c->drain();
    if (rc != RENE_OK) return rc;
  }
  // Launches are serial on the context's one stream.  (Rounds 1-2 alternated consecutive launches between two streams so that
  // the next launch filled the slots the previous one's tail vacated; the waves of the later launch then waited, holding
  // their slots, for pixels of the earlier one -- and when the driver evicted and restored the process's queues, the earlier
  // launch's waves could find their slots taken: a stall of seconds, docs/history.md section 4g.  One launch per job in short work
  // items has the same tail to hide -- none between launches -- and no launch ever waits for another.)
  hipStream_t stream = c->stream;
  if (std::getenv("RENE_DEBUG") && !c->d_wave_times) {
    if (int rc = c->d_wave_times.reserve((size_t)rene_ctx::kCounters * 8192 * 2 * 8, "rene_render: wave times"); rc != RENE_OK) return rc;
    HIP_TRY(c->zero_now(c->d_wave_times, (size_t)rene_ctx::kCounters * 8192 * 2 * 8));
  }
  rene_ctx::Pending pend;  // (its events go with it if the launch does not happen)
  hipError_t e = pend.start.create();
  if (e == hipSuccess) e = pend.stop.create();
  if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("rene_render setup: ") + hipGetErrorString(e));
  rene::RenderParams P{};
  P.framebuffer = c->chains;
  P.seed_state0 = HostPcg(c->opts.seed).s;
  P.first_frame = share.first;
  P.frame_stride = share.stride;
  P.work_counter = c->d_work_counters + c->counters_used;
  P.wave_times = c->d_wave_times ? c->d_wave_times + (size_t)c->counters_used * 8192 * 2 : nullptr;
  P.item_done = c->d_item_done;
  P.ray_dump = c->ray_dump;
  P.ray_dump_cap = c->ray_dump_cap;
  P.frame_stream = frame_stream ? c->frame_stream.as<float>() : nullptr;
  P.active_tiles = c->n_inactive ? c->mask_dev.as<uint32_t>() : nullptr;  // (uploaded by rene_set_active_tiles behind a drain: nothing is copied here)
  P.counters = c->d_counters;
  P.n_frames = share.count;
  // frame chains (device_scene.h): global frame f belongs to chain (f / frame_stride) % CHAINS -- a rule on the frame's number, so that a pixel's
  // chains hold the same sums however a job is cut into calls; a level's work ids: pixel slot * CHAINS + chain
  P.n_work = c->n_work * rene::CHAINS;
  P.chain_phase = share.chain_phase();
  P.group_frames = share.group_frames();
  P.shard_rank = c->opts.shard_mode == RENE_SHARD_TILES ? c->opts.shard_rank : 0;
  P.shard_count = c->opts.shard_mode == RENE_SHARD_TILES ? c->opts.shard_count : 1;
  P.tiles_x = c->tiles_x;
  P.inv_tiles_x = 1.0f / (float)std::max(1u, c->tiles_x);
  P.inv_shard_count = 1.0f / (float)P.shard_count;
  P.n_tiles = c->n_tiles;
  P.flags = c->opts.flags;
  // No work item may belong to a wave that is not resident: items wait for their predecessors, and a statically owned
  // first batch of a wave that has not been given a slot -- the device shared with another process, or the previous
  // launch still draining -- can be waited for by every wave that has one (seen: two processes' counting launches on
  // one GPU, each holding the slots the other's missing waves needed).  With every batch taken from the atomic
  // counter the item a lane waits for is always in the hands of a resident lane.  (The static first batch saved
  // 0.05 ms per launch.)
  P.flags |= RENE_FLAG_DYNAMIC_FIRST;
  // (tests: RENE_TEST_KERNEL_LOG=<path> logs the kernel of every render launch, kernels.h)
  if (const char* e = std::getenv("RENE_TEST_DROP"))  // fault injection (tests): the context's launch number e drops some of its items
    if ((uint32_t)std::atoi(e) == c->epoch + 1u) P.flags |= rene::RENE_FLAG_INTERNAL_TEST_DROP;
  // every pixel's frames in work items (launch_plan.h, item_cut; the knobs are read at every call: tests set them between two)
  const rene::ItemKnobs knobs{env_int("RENE_ITEM_FRAMES"), env_int("RENE_ITEM_TAIL"), env_int("RENE_LEVELS")};
  const bool small_scene = (c->cfg.features & rene::FEAT_SMALL) != 0, single_level = (c->opts.flags & RENE_FLAG_SINGLE_LEVEL) != 0;
  // an untuned item-loop context of the path integrator with no knob set: the policy in front of the cut (launch_plan.h: a long first item, a short
  // last one, never more levels); 0 = the untuned cut.  rene_tune, kWholeLaunch, the knobs and RENE_FLAG_SINGLE_LEVEL go past it.
  uint32_t item_frames = c->item_frames;
  if (small_scene && !(c->cfg.features & rene::FEAT_VOLPATH) && item_frames == 0 && !single_level && !knobs.item_frames && !knobs.item_tail && !knobs.levels)
    item_frames = rene::small_scene_item_frames(P.group_frames, c->owned_pixels, (uint64_t)c->cfg.grid * (uint32_t)rene::render_block_size());
  const rene::ItemCut cut = rene::item_cut(P.group_frames, small_scene, c->owned_pixels, item_frames, single_level, knobs);
  P.level_step = cut.level_step;
  P.n_uniform = cut.n_uniform;
  P.n_levels = cut.n_levels;
  if (c->epoch >= rene::MAX_EPOCH) {  // (drained above) the epoch wraps: every pixel record back to version 0 -- whether or not the launch then happens
    hipMemset2DAsync(c->chains + 3, 4 * sizeof(float), 0, sizeof(float), (size_t)rene::CHAINS * 3u * c->n_work, stream);
    hipMemsetAsync(c->d_item_done, 0, (size_t)rene::CHAINS * c->n_work * sizeof(uint32_t), stream);
    c->epoch = 0;
    c->prev_final = 0;
  }
  P.prev_final = c->prev_final;
  P.epoch = c->epoch + 1u;
  // swept with the BVH4 (tools/dev_sweep4.py): dragon-class (Matte) peaks at 24 / 12 (4.96 Grays/s; 20 / 16 gave 4.6);
  // teapot-class, whose logic step is the general-BSDF one, keeps gaining up to ~44 waiting lanes (5.3 vs 4.7)
  P.ready_min = (c->cfg.features & rene::FEAT_GENERAL_BSDF) ? 40 : 24;
  P.leaf_min = 6;  // re-swept in round 3 on whole one-launch jobs: flat from 2 to 12 (dragon-class 686 - 689 ms, the teapot scene 3748 - 3789)
  if (const char* e = std::getenv("RENE_READY_MIN")) P.ready_min = (uint32_t)std::max(1, std::atoi(e));  // tuning knobs
  if (const char* e = std::getenv("RENE_LEAF_MIN")) P.leaf_min = (uint32_t)std::max(1, std::atoi(e));
  // what a launch that has been issued leaves in the context's counts: the frames, the paths, and the version it leaves on every pixel record
  const auto commit = [&] {
    count_frames();
    c->paths += launch_paths;
    c->epoch = P.epoch;
    c->prev_final = (P.epoch << rene::VERSION_LEVEL_BITS) | P.n_levels;
  };
  if (c->wavefront) {
    // Host-driven rounds of three kernels (wavefront.inc) until every slot has rendered its frames.  The
    // number of rounds is the largest number of bounces any pixel needs over the launch's frames, known
    // only to the device: run a batch sized from the frame count, then poll the done counter (a 4-byte
    // copy + one stream sync per batch).  rene_render is therefore synchronous for these scenes.
    // (Its launches are many and cannot be taken back: it counts before the first, and keeps its counts when a round fails.)
    commit();
    uint32_t* const h_done = c->h_done.as<uint32_t>();
    rene::LaunchConfig cfg = c->cfg;
    hipEventRecord(pend.start, c->stream);
    e = rene::launch_wave_init(c->wave, c->stream);
    uint32_t batch = std::max(8u, 2u * P.n_frames);
    uint64_t rounds = 0;
    const uint64_t max_rounds = 64ull + 51ull * P.n_frames;  // depth cap 50 (lib.rs:192) + regeneration rounds
    while (e == hipSuccess) {
      e = rene::launch_wave_rounds(cfg, c->view, P, c->wave, batch, c->stream);
      rounds += batch;
      if (e == hipSuccess) e = hipMemcpyAsync(h_done, c->wave.n_done, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess || *h_done >= c->wave.n_slots) break;
      if (rounds > max_rounds) {
        hipEventRecord(pend.stop, c->stream);
        c->pending.push_back(std::move(pend));
        return fail(RENE_ERR_DEVICE, "wavefront integrator: pixels left unfinished after the maximum number of rounds");
      }
      batch = std::max(8u, P.n_frames / 4u);
    }
    if (e == hipSuccess) e = rene::launch_wave_finish(P, c->wave, c->stream);
    hipEventRecord(pend.stop, c->stream);
    c->pending.push_back(std::move(pend));
    c->launches++;
    c->fb_stale = true;
    if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("wavefront launch: ") + hipGetErrorString(e));
    return c->drain();
  }
  rene::LaunchConfig cfg = c->cfg;
  const rene::WorkBatch batches = rene::work_batch(P.n_levels, P.n_work, cfg.grid, (uint32_t)rene::render_block_size(), env_int("RENE_WORK_BATCH"));
  cfg.grid = batches.grid;
  P.work_batch = batches.work_batch;
  P.level_batches = batches.level_batches;
  P.inv_level_batches = 1.0f / (float)P.level_batches;
  hipEventRecord(pend.start, stream);
  rene::g_launched_blocks = cfg.grid;
  e = rene::launch_render(cfg, c->view, P, stream);
  // nothing was launched: no pending entry (a replay must not launch what the caller was told failed), no counter slot, nothing counted,
  // and the next launch does not wait for versions this one would have written
  if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("render launch: ") + hipGetErrorString(e));
  hipEventRecord(pend.stop, stream);
  pend.epoch = P.epoch;
  pend.replayable = true;
  pend.P = P;
  pend.cfg = cfg;
  commit();
  c->counters_used++;
  c->pending.push_back(std::move(pend));
  c->launches++;
  c->fb_stale = true;
  if (c->pending.size() >= rene_ctx::kCounters) return c->drain();
  return RENE_OK;
}

int rene_sync(rene_ctx* c) {
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_sync: NULL context");
  HIP_TRY(hipSetDevice(c->device));
  return c->drain();
}

int rene_reset(rene_ctx* c) {
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_reset: NULL context");
  HIP_TRY(hipSetDevice(c->device));
  int rc = c->drain();
  if (rc != RENE_OK && !c->handoff_failed) return rc;
  c->handoff_failed = false;  // the counters are cleared below and the image starts again from zero
  c->exchanged = false;
  HIP_TRY(hipMemsetAsync(c->chains, 0, (size_t)rene::CHAINS * 3u * c->n_work * 4u * sizeof(float), c->stream));  // (the owned pixel slots only)
  HIP_TRY(hipMemsetAsync(c->fb, 0, c->fb_floats * sizeof(float), c->stream));
  c->fb_stale = false;
  HIP_TRY(hipMemsetAsync(c->d_counters, 0, 32 * sizeof(unsigned long long), c->stream));
  HIP_TRY(hipMemsetAsync(c->d_item_done, 0, (size_t)rene::CHAINS * c->n_work * sizeof(uint32_t), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->prev_final = 0;  // the pixel records carry version 0 again
  c->frames = 0;
  for (uint64_t& f : c->chain_frames) f = 0;
  c->dn_valid = false;
  c->dn_shard.invalidate();  // (a round of placed records is not this context's frames: it stays)
  c->dn_gather_root = -1;  // ... but what rene_gather_denoise left to be placed went with this context's own packed buffer
  c->noise_valid = false;
  c->robust_valid = false;
  c->features.invalidate();
  c->out.invalidate();
  c->exr.invalidate();
  c->exr_tail.invalidate();
  c->cryptomatte.invalidate();
  c->exr_passes.invalidate();
  c->clear_active_tiles();  // every tile active again, no tile has frames
  c->loaded = false;
  c->paths = 0;
  c->launches = 0;
  c->replays = 0;
  c->kernel_ms = 0.0;
  c->last_ms = 0.0;
  return RENE_OK;
}

int rene_tune(rene_ctx* c, uint32_t n_frames) {
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_tune: NULL context");
  if (c->wavefront || n_frames < 4 || c->n_work == 0 || (c->opts.flags & RENE_FLAG_SINGLE_LEVEL)) return RENE_OK;
  HIP_TRY(hipSetDevice(c->device));
  int rc = c->drain();
  if (rc != RENE_OK) return rc;
  const uint32_t saved = c->item_frames;
  uint32_t best = saved;
  double best_ms = 0.0;
  // candidates: one item per pixel, chain and launch, then items of 256 / 128 / 64 / 32 / 16 frames (of the chain's share of the launch)
  const uint32_t items[6] = {rene_ctx::kWholeLaunch, 256u, 128u, 64u, 32u, 16u};
  const uint32_t chain_frames = (n_frames + rene::CHAINS - 1u) / rene::CHAINS;
  for (int i = 0; i < 6; ++i) {
    if (i > 0 && items[i] * 2u > chain_frames) continue;
    c->item_frames = items[i];
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < 3 && rc == RENE_OK; ++k) rc = rene_render(c, 0, n_frames);  // what is rendered does not matter
    if (rc == RENE_OK) rc = c->drain();
    if (rc != RENE_OK) {
      c->item_frames = saved;
      return rc;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (i == 0 || ms < 0.985 * best_ms) {  // finer items must pay for their bookkeeping
      best_ms = ms;
      best = c->item_frames;
    }
  }
  c->item_frames = best;
  if (std::getenv("RENE_DEBUG"))
    std::fprintf(stderr, "[rene] tuned: work items of %u frames for launches of %u frames\n", best == rene_ctx::kWholeLaunch ? n_frames : best, n_frames);
  return rene_reset(c);
}

int rene_framebuffer(rene_ctx* c, void** device_ptr, size_t* n_floats) {
  if (!c || !device_ptr) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_framebuffer: NULL argument");
  *device_ptr = c->fb;
  if (n_floats) *n_floats = c->fb_floats;
  HIP_TRY(hipSetDevice(c->device));
  {  // frame chains: the image is the chains added together, which a drain does (not in stream order)
    int rc = c->drain();
    if (rc != RENE_OK) return rc;
  }
  return c->flush_exchange();
}

// ---- the `atrous` denoiser (kernels_denoise.hip; the filter is specified in include/rene_hip.h) ----------------------------------------
void rene_denoise_params_default(rene_denoise_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->iterations = 5;
  out->sigma_luminance = 4.0f;
  out->sigma_normal2 = 1.0f / 64.0f;
  out->sigma_albedo2 = 1.0f / 16.0f;
  out->albedo_floor = 0.05f;
  out->relative_floor = 1e-3f;
}

// ---- what the denoiser's entry points share: rene_denoise / rene_denoise_tiles and their trimmed forms (denoise_run), and the calls that prepare on
// tile shards and filter on one context (rene_denoise_shard_prepare, rene_denoise_place_shard, rene_denoise_placed) --------------------------------------
// the caller's params, or the defaults, checked
static int denoise_read_params(const std::string& me, const rene_denoise_params* params, rene_denoise_params& p) {
  if (int rc = read_params("rene_denoise_params", rene_denoise_params_default, params, p); rc != RENE_OK) return rc;
  if (p.iterations < 1 || p.iterations > 8) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": iterations must be 1 .. 8");
  const float positive[5] = {p.sigma_luminance, p.sigma_normal2, p.sigma_albedo2, p.albedo_floor, p.relative_floor};
  const char* names[5] = {"sigma_luminance", "sigma_normal2", "sigma_albedo2", "albedo_floor", "relative_floor"};
  for (int i = 0; i < 5; ++i)
    if (!std::isfinite(positive[i]) || !(positive[i] > 0.0f)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": " + names[i] + " must be finite and positive");
  return RENE_OK;
}

static const char* const kDenoiseFewFrames = ": the variance estimate needs frames in at least two of the eight frame chains (render two or more consecutive frames first)";

// the tile-by-tile calls' table: one set of constants per distinct N_t of the owned tiles, the set of every owned tile, and what the log and
// RENE_DENOISED_MEAN need of them
struct DenoiseTilePlan {
  std::vector<float> sets;               // [distinct N_t][set_floats]
  std::vector<uint32_t> tile_set;        // the set of every owned tile, NOISE_SET_NONE for an invalid one
  std::vector<uint32_t> invalid_frames;  // on the image's full tile grid: N_t of this context's invalid tiles, DN_TILE_VALID elsewhere
  uint64_t N = 0;                        // of the most-sampled valid tile
  uint32_t k = 0, n_invalid = 0;
};
// one set per distinct N_t, as rene_estimate_noise derives them; an even context: the context's own chain counts, as rene_denoise takes them.
// RENE_ERR_INVALID_ARGUMENT where the context owns tiles and none of them is valid
static int denoise_plan_tiles(const std::string& me, const rene_ctx* c, bool robust, DenoiseTilePlan& P) {
  const uint32_t set_floats = robust ? rene::DENOISE_ROBUST_SET_FLOATS : rene::DENOISE_SET_FLOATS;
  std::vector<uint32_t> counts;
  distinct_tile_counts(c, counts, P.tile_set);
  const bool uneven = c->uneven();
  P.sets.assign(counts.size() * set_floats, 0.0f);
  std::vector<uint32_t> set_of(counts.size());
  for (uint32_t s = 0; s < counts.size(); ++s) {
    uint64_t cf[rene::CHAINS], n = 0;
    uint32_t kk = 0;
    if (uneven) rene_ctx::chain_counts(c->frame_base, counts[s], cf);
    else std::copy(c->chain_frames, c->chain_frames + rene::CHAINS, cf);
    float* set = &P.sets[(size_t)s * set_floats];
    set_of[s] = chain_constants(cf, set, &n, &kk) ? s : rene::NOISE_SET_NONE;
    set[rene::NOISE_SET_FLOATS] = (float)n;
    for (uint32_t g = 0; robust && g < rene::CHAINS; ++g) {  // the n_c themselves, as bits
      const uint32_t n_c = (uint32_t)cf[g];
      std::memcpy(&set[rene::DENOISE_SET_FLOATS + g], &n_c, sizeof n_c);
    }
    if (set_of[s] != rene::NOISE_SET_NONE && n >= P.N) {
      P.N = n;
      P.k = kk;
    }
  }
  P.invalid_frames.assign(c->n_tiles, rene_ctx::DN_TILE_VALID);
  for (uint32_t i = 0; i < P.tile_set.size(); ++i) {
    P.tile_set[i] = set_of[P.tile_set[i]];
    if (P.tile_set[i] != rene::NOISE_SET_NONE) continue;
    P.n_invalid += 1u;
    if (c->owned_tile(i) < c->n_tiles) P.invalid_frames[c->owned_tile(i)] = c->tile_n(i);
  }
  if (P.n_invalid == P.tile_set.size() && !P.tile_set.empty()) return fail(RENE_ERR_INVALID_ARGUMENT, me + kDenoiseFewFrames + " -- no owned tile has");
  return RENE_OK;
}

// the filter's buffers: RENE_DENOISE_BYTES_PER_PIXEL bytes per pixel, allocated once
static int denoise_alloc_buffers(const std::string& me, rene_ctx* c) {
  if (c->dn_var.p) return RENE_OK;  // (the last of the five)
  const size_t n_px = (size_t)c->width * c->height;
  DevBuf* bufs[5] = {&c->dn_rec[0], &c->dn_rec[1], &c->dn_guides, &c->dn_out, &c->dn_var};
  const size_t floats[5] = {4, 4, 8, 4, 1};
  for (int i = 0; i < 5; ++i)
    if (int rc = bufs[i]->reserve(n_px * floats[i] * sizeof(float), me + " buffers"); rc != RENE_OK) return rc;
  if (std::getenv("RENE_DEBUG"))
    std::fprintf(stderr, "[rene] denoiser buffers: %u bytes per pixel, %.3f GB\n", (unsigned)RENE_DENOISE_BYTES_PER_PIXEL, (double)n_px * RENE_DENOISE_BYTES_PER_PIXEL * 1e-9);
  return RENE_OK;
}

// the launch structure's part that comes from the params and the environment's A/B knobs; returns stage_max
static int denoise_fill_launch(rene::DenoiseLaunch& D, const rene_denoise_params& p) {
  D.sigma_l = p.sigma_luminance;
  D.inv_sigma_n2 = 1.0f / p.sigma_normal2;
  D.inv_sigma_a2 = 1.0f / p.sigma_albedo2;
  D.albedo_floor = p.albedo_floor;
  D.relative_floor = p.relative_floor;
  D.tile_columns = 32;  // (swept 0 / 4 / 8 / 16 / 32 at 1920 x 1080 and 7680 x 4320)
  if (const char* e = std::getenv("RENE_DENOISE_TILE_COLUMNS")) D.tile_columns = (uint32_t)std::max(0, std::min(512, std::atoi(e)));  // A/B knob (0: tiles in launch order)
  int stage_max = rene::denoise_stage_max();
  if (const char* e = std::getenv("RENE_DENOISE_STAGE_MAX")) stage_max = std::atoi(e);  // A/B knob: 0 = no pass stages its tile in LDS, 4 = steps 1, 2 and 4 do
  return stage_max;
}

// How every call that filters ends: the passes and finalize over the records that wait in dn_rec[0] (put there by the caller's prepare or place
// launches, whose last mark is M's last), the wait, the log, and -- in this one place -- the state the downloads read.  `masked`: the kernels that
// leave the invalid tiles alone (kernels_denoise.hip, MASKED), `invalid_frames` their N_t on the full grid.  The caller has set dn_valid = false before
// its first launch; it is true again only here.  RENE_DEBUG: head(parts, total) prints whatever the caller's own launches have to report, leaves their
// part of the line and of the total, and returns the line's head; the passes' times follow.
static int denoise_filter(const std::string& me, rene_ctx* c, rene::DenoiseLaunch& D, const rene_denoise_params& p, int stage_max, bool masked, bool robust,
                          std::vector<uint32_t> invalid_frames, Marks& M, const std::function<std::string(std::string&, float&)>& head) {
  float* const rec[2] = {c->dn_rec[0].as<float>(), c->dn_rec[1].as<float>()};
  float* const guides = c->dn_guides.as<float>();
  const size_t first = M.size();  // (the first mark of this function's own; the one before it starts the first pass)
  hipError_t e = hipSuccess;
  uint32_t cur = 0;
  for (uint32_t i = 0; i < p.iterations && e == hipSuccess; ++i) {
    D.step = 1u << i;
    e = rene::launch_atrous_pass(rec[cur], guides, rec[cur ^ 1u], D, masked, stage_max, c->stream);
    cur ^= 1u;
    M.mark();
  }
  if (e == hipSuccess) e = rene::launch_denoise_finalize(rec[cur], guides, c->dn_out.as<float>(), D, masked, c->stream);
  M.mark();
  if (e != hipSuccess) return launch_failed(me, c, e);
  HIP_TRY(wait_stream(c->stream));
  if (M.complete) {
    std::string parts;
    float total = 0.0f;
    const std::string line_head = head(parts, total);
    for (size_t i = first; i < M.size(); ++i) {
      const float ms = M.ms(i - 1, i);
      total += ms;
      char buf[64];
      if (i + 1 == M.size()) std::snprintf(buf, sizeof buf, "finalize %.4f", ms);
      else {
        const uint32_t s = 1u << (i - first);  // (the staged kernels exist for steps 1, 2 and 4: launch_atrous_pass)
        std::snprintf(buf, sizeof buf, "step %u%s %.4f", s, (int)s <= stage_max && s <= 4u ? " (LDS)" : "", ms);
      }
      parts += (parts.empty() ? "" : ", ") + std::string(buf);
    }
    std::fprintf(stderr, "%s, ms: %s; total %.4f\n", line_head.c_str(), parts.c_str(), total);
  }
  c->dn_cur = cur;
  c->dn_albedo_floor = p.albedo_floor;
  c->dn_masked = masked;
  c->dn_robust = robust;
  c->dn_invalid_frames = std::move(invalid_frames);
  c->dn_valid = true;
  return RENE_OK;
}

// What rene_denoise and rene_denoise_tiles share -- all but who gets which constants.  `tiles`: every owned tile with the constants of its own N_t
// from a table (one set on an even context), tiles with frames in fewer than two chains masked out (kernels_denoise.hip, TILES).  `robust`: the
// trimmed prepare (kernels_denoise_trim.hip decides which chains a pixel leaves out, the TRIM prepare of kernels_denoise.hip takes the rest); the
// table's sets then carry the chain counts themselves behind the constants.  Everything after prepare is the same launches either way.
static int denoise_run(const char* fn, rene_ctx* c, const rene_denoise_params* params, bool tiles, bool robust = false, const rene_robust_params* robust_params = nullptr) {
  const std::string me = fn;
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  rene_denoise_params p;
  if (int prc = denoise_read_params(me, params, p); prc != RENE_OK) return prc;
  rene_robust_params rp;
  if (int prc = read_params("rene_robust_params", rene_denoise_robust_params_default, robust ? robust_params : nullptr, rp); prc != RENE_OK) return prc;
  if (robust)
    if (int prc = check_robust_params(me, rp); prc != RENE_OK) return prc;
  if (c->opts.shard_count > 1)
    return fail(RENE_ERR_UNSUPPORTED, me + ": a sharded context (shard_count > 1) holds only its share of the image or of the frames; " +
                                          (robust ? "the plain filter is available for tile shards (rene_denoise_shard_prepare, rene_denoise_place_shard, rene_denoise_placed), the trimmed one is not: "
                                                    "denoise an unsharded context"
                                                  : "denoise an unsharded context, or prepare tile shards with rene_denoise_shard_prepare and filter them on one context "
                                                    "(rene_denoise_place_shard / rene_gather_denoise, rene_denoise_placed)"));
  uint64_t N = 0;  // (tiles: of the most-sampled valid tile, for the log)
  uint32_t k = 0;
  float consts[rene::NOISE_SET_FLOATS] = {};
  const uint32_t set_floats = robust ? rene::DENOISE_ROBUST_SET_FLOATS : rene::DENOISE_SET_FLOATS;
  DenoiseTilePlan plan;
  rene::DenoiseLaunch D{};
  int rc = begin_chain_pass(fn, c, robust, D.grid, [&] {
    if (!tiles) {
      if (c->uneven())
        return fail(RENE_ERR_UNSUPPORTED, me + ": the context's tiles differ in their frame counts (rene_set_active_tiles) and the filter takes one count; rene_reset and render again");
      return chain_constants(c->chain_frames, consts, &N, &k) ? (int)RENE_OK : fail(RENE_ERR_INVALID_ARGUMENT, me + kDenoiseFewFrames);
    }
    const int prc = denoise_plan_tiles(me, c, robust, plan);
    N = plan.N;
    k = plan.k;
    return prc;
  });  // (... and the drain: waits for the launches issued so far and resolves the image, from which the guide layers are read)
  if (rc != RENE_OK) return rc;
  const size_t n_px = (size_t)c->width * c->height;
  rc = denoise_alloc_buffers(me, c);
  if (rc != RENE_OK) return rc;
  if (robust) {  // 4 bytes per pixel more, allocated by the first robust call
    rc = c->dn_trim.reserve(std::max<size_t>(4, n_px * sizeof(uint32_t)), me + " trim plane");
    if (rc != RENE_OK) return rc;
  }
  rene::DenoiseTileSets T{nullptr, nullptr};
  if (tiles) {
    rc = upload_tile_sets(c, plan.sets, plan.tile_set, &T.sets, &T.tile_set);
    if (rc != RENE_OK) return rc;
  }
  D.n_frames = (float)N;
  D.inv_n = consts[0];
  D.inv_km1 = consts[1];
  for (uint32_t g = 0; g < rene::CHAINS; ++g) {
    D.chain_share[g] = consts[2u + g];
    D.chain_inv[g] = consts[2u + rene::CHAINS + g];
  }
  const int stage_max = denoise_fill_launch(D, p);
  float* const rec0 = c->dn_rec[0].as<float>();
  float* const guides = c->dn_guides.as<float>();
  float* const var = c->dn_var.as<float>();
  uint32_t* const trim = c->dn_trim.as<uint32_t>();
  Marks M(c->stream);
  c->dn_valid = false;
  c->dn_placed.clear();  // (records placed by rene_denoise_place_shard and not filtered yet are overwritten: that round starts again)
  M.mark();
  hipError_t e = hipSuccess;
  rene::DenoisePrepare A{rec0, guides, var, nullptr, T, {}};
  if (robust) {
    rene::DenoiseTrimLaunch L{};
    L.grid = D.grid;
    L.max_trim = rp.max_trim;
    L.gain = rp.gain;
    A.trimmed.trim = trim;
    for (uint32_t g = 0; g < rene::CHAINS; ++g) L.chain_n[g] = A.trimmed.chain_n[g] = (uint32_t)c->chain_frames[g];
    L.sets = T.sets;
    L.tile_set = T.tile_set;
    e = rene::launch_denoise_trim(c->chains, trim, L, c->stream);
    M.mark();
  }
  if (e == hipSuccess) e = rene::launch_denoise_prepare(c->chains, c->fb, A, D, c->stream);
  M.mark();
  if (e != hipSuccess) return launch_failed(me, c, e);
  const size_t n_sets = plan.sets.size() / set_floats;
  const uint32_t n_invalid = plan.n_invalid;
  return denoise_filter(me, c, D, p, stage_max, tiles, robust, std::move(plan.invalid_frames), M, [&](std::string& parts, float& total) {
    size_t prepared = 1;  // the mark behind prepare
    if (robust) {  // the trim kernel's interval, reported in front: the marks after it are those of a plain call
      std::fprintf(stderr, "[rene] denoise, trimmed prepare (max_trim %u, gain %g), ms: trim %.4f\n", rp.max_trim, (double)rp.gain, M.ms(0, 1));
      prepared = 2;
    }
    total = M.ms(prepared - 1, prepared);
    char buf[256];
    std::snprintf(buf, sizeof buf, "prepare %.4f", total);
    parts = buf;
    if (tiles)
      std::snprintf(buf, sizeof buf, "[rene] denoise, tile by tile, %u x %u, %zu frame counts, up to %llu frames in %u chains, %u invalid tiles", c->width, c->height, n_sets,
                    (unsigned long long)N, k, n_invalid);
    else std::snprintf(buf, sizeof buf, "[rene] denoise %u x %u, %llu frames in %u chains", c->width, c->height, (unsigned long long)N, k);
    return std::string(buf);
  });
}

int rene_denoise(rene_ctx* c, const rene_denoise_params* params) { return guarded([&] { return denoise_run("rene_denoise", c, params, false); }); }
int rene_denoise_tiles(rene_ctx* c, const rene_denoise_params* params) { return guarded([&] { return denoise_run("rene_denoise_tiles", c, params, true); }); }


// ---- the denoiser on tile shards (kernels_denoise.hip, PACKED; include/rene_hip.h has the layout of the packed buffer and the order of the calls) -------
static size_t shard_body_offset(uint32_t n_owned) { return sizeof(rene_denoise_shard_header) + (((size_t)n_owned * sizeof(rene_denoise_shard_tile) + 15u) & ~(size_t)15u); }

size_t rene_denoise_shard_bytes(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count) {
  static_assert(sizeof(rene_denoise_shard_header) == 64 && sizeof(rene_denoise_shard_tile) == 8, "the packed buffer's layout (include/rene_hip.h)");
  static_assert(RENE_DENOISE_SHARD_TILE_BYTES == rene::DN_PACKED_TILE_BYTES, "the header's and the kernels' tile block");
  if (width == 0 || height == 0 || width > rene::MAX_RESOLUTION || height > rene::MAX_RESOLUTION || shard_count == 0 || shard_rank >= shard_count) return 0;
  const uint32_t n_tiles = ((width + RENE_TILE_SIZE - 1) / RENE_TILE_SIZE) * ((height + RENE_TILE_SIZE - 1) / RENE_TILE_SIZE);
  const uint32_t n_owned = owned_tiles(n_tiles, shard_rank, shard_count);
  return shard_body_offset(n_owned) + (size_t)n_owned * rene::DN_PACKED_TILE_BYTES;
}

static int rene_denoise_shard_prepare_impl(rene_ctx* c, const rene_denoise_params* params) {
  const char* fn = "rene_denoise_shard_prepare";
  const std::string me = fn;
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  rene_denoise_params p;
  if (int prc = denoise_read_params(me, params, p); prc != RENE_OK) return prc;
  DenoiseTilePlan plan;
  rene::DenoiseLaunch D{};
  int rc = begin_chain_pass(fn, c, false, D.grid, [&] { return denoise_plan_tiles(me, c, false, plan); });
  if (rc != RENE_OK) return rc;
  const uint32_t n_owned = c->n_owned();
  const size_t body_off = shard_body_offset(n_owned), bytes = body_off + (size_t)n_owned * rene::DN_PACKED_TILE_BYTES;
  if (bytes != rene_denoise_shard_bytes(c->width, c->height, D.grid.shard_rank, D.grid.shard_count)) return fail(RENE_ERR_DEVICE, me + ": the context's owned tiles do not match its shard");
  void* packed = nullptr;
  rc = c->dn_shard.begin(bytes, {}, c->stream, me + " packed buffer", packed);  // (header, table and body: every byte is written below)
  if (rc != RENE_OK) return rc;
  rene::DenoiseTileSets T{nullptr, nullptr};
  if (n_owned) {
    rc = upload_tile_sets(c, plan.sets, plan.tile_set, &T.sets, &T.tile_set);
    if (rc != RENE_OK) return rc;
  }
  denoise_fill_launch(D, p);
  // header and N_t table, from the host; the body from the kernel
  std::vector<unsigned char> head(body_off, 0);
  rene_denoise_shard_header h{};
  h.magic = RENE_DENOISE_SHARD_MAGIC;
  h.header_bytes = sizeof(h);
  h.width = c->width;
  h.height = c->height;
  h.shard_rank = D.grid.shard_rank;
  h.shard_count = D.grid.shard_count;
  h.n_owned = n_owned;
  h.params = p;
  h.params.reserved = 0;
  std::memcpy(head.data(), &h, sizeof h);
  for (uint32_t i = 0; i < n_owned; ++i) {
    const rene_denoise_shard_tile tt{c->tile_n(i), plan.tile_set[i] != rene::NOISE_SET_NONE ? 1u : 0u};
    std::memcpy(head.data() + sizeof h + (size_t)i * sizeof tt, &tt, sizeof tt);
  }
  HIP_TRY(hipMemcpy(packed, head.data(), head.size(), hipMemcpyHostToDevice));
  rc = timed_launch(fn, c, [&] { return rene::launch_denoise_prepare(c->chains, c->fb, rene::DenoisePrepare{nullptr, nullptr, nullptr, static_cast<char*>(packed) + body_off, T, {}}, D, c->stream); },
                    [&](float ms) {
                      std::fprintf(stderr, "[rene] denoise shard %u of %u, %u x %u, %u owned tiles (%u invalid), %zu frame counts, %zu bytes, ms: packed prepare %.4f\n", h.shard_rank,
                                   h.shard_count, c->width, c->height, n_owned, plan.n_invalid, plan.sets.size() / rene::DENOISE_SET_FLOATS, bytes, ms);
                    });
  if (rc != RENE_OK) return rc;
  c->dn_shard.commit(bytes);
  return RENE_OK;
}

int rene_denoise_shard_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) {
  return result_buffer("rene_denoise_shard_buffer", c, &rene_ctx::dn_shard, kNoShard, device_ptr, n_bytes, true);
}
int rene_download_denoise_shard(rene_ctx* c, void* dst, size_t dst_bytes) {
  return result_download("rene_download_denoise_shard", c, &rene_ctx::dn_shard, kNoShard, "dst_bytes is smaller than the packed buffer", false, dst, dst_bytes);
}

// One packed buffer onto the root's records.  body_here: `src` is memory of the root's own device that stays as it is until the kernel has run (the
// staging of rene_gather_denoise, the root's own packed buffer): its body is read in place; otherwise it is copied into the root's staging first
static int place_shard(rene_ctx* c, const void* src, size_t bytes, bool body_here) {
  const std::string me = "rene_denoise_place_shard";
  if (bytes < sizeof(rene_denoise_shard_header)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": " + std::to_string(bytes) + " bytes are fewer than a header");
  rene_denoise_shard_header h;
  HIP_TRY(hipMemcpy(&h, src, sizeof h, hipMemcpyDefault));
  if (h.magic != RENE_DENOISE_SHARD_MAGIC || h.header_bytes != sizeof h) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": not a packed denoise shard (bad magic or header size)");
  if (h.width != c->width || h.height != c->height)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the buffer is of a " + std::to_string(h.width) + " x " + std::to_string(h.height) + " film, the context's is " + std::to_string(c->width) + " x " +
                                               std::to_string(c->height));
  if (h.shard_count == 0 || h.shard_rank >= h.shard_count) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the header's shard_rank is not below its shard_count");
  // (a shard layout may have more shards than the film has tiles, but no more than the largest film has: the round keeps a flag per rank)
  constexpr uint32_t kMaxShards = (rene::MAX_RESOLUTION / RENE_TILE_SIZE) * (rene::MAX_RESOLUTION / RENE_TILE_SIZE);
  if (h.shard_count > kMaxShards) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the header's shard_count " + std::to_string(h.shard_count) + " is above " + std::to_string(kMaxShards));
  const uint32_t n_owned = owned_tiles(c->n_tiles, h.shard_rank, h.shard_count);
  if (h.n_owned != n_owned) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the header's tile count is not that of its shard");
  const size_t want = rene_denoise_shard_bytes(h.width, h.height, h.shard_rank, h.shard_count);
  if (bytes != want) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": " + std::to_string(bytes) + " bytes, the packed buffer of shard " + std::to_string(h.shard_rank) + " of " + std::to_string(h.shard_count) + " has " + std::to_string(want));
  {
    rene_denoise_params checked;
    if (int prc = denoise_read_params(me, &h.params, checked); prc != RENE_OK) return prc;
  }
  const bool round_open = std::find(c->dn_placed.begin(), c->dn_placed.end(), (uint8_t)1) != c->dn_placed.end();
  if (round_open) {
    if (h.shard_count != c->dn_round.shard_count)
      return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a buffer of " + std::to_string(h.shard_count) + " shards among buffers of " + std::to_string(c->dn_round.shard_count) + " placed in this round");
    if (std::memcmp(&h.params, &c->dn_round.params, sizeof h.params) != 0)
      return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the buffer was prepared with other rene_denoise_params than those placed in this round");
  }
  std::vector<rene_denoise_shard_tile> table(n_owned);
  if (n_owned) HIP_TRY(hipMemcpy(table.data(), static_cast<const char*>(src) + sizeof h, (size_t)n_owned * sizeof(rene_denoise_shard_tile), hipMemcpyDefault));
  int rc = denoise_alloc_buffers(me, c);
  if (rc != RENE_OK) return rc;
  const size_t body_off = shard_body_offset(n_owned), body_bytes = (size_t)n_owned * rene::DN_PACKED_TILE_BYTES;
  const void* body = static_cast<const char*>(src) + body_off;
  if (!body_here && body_bytes) {
    rc = c->dn_place_buf.reserve(body_bytes, me + " staging");
    if (rc != RENE_OK) return rc;
    // on the context's stream, ahead of the kernel that reads the staging: a device-to-device hipMemcpy returns before the copy has run, and the
    // null stream does not order it with a non-blocking stream -- the kernel could read what the shard placed before had left there
    HIP_TRY(hipMemcpyAsync(c->dn_place_buf.p, body, body_bytes, hipMemcpyDefault, c->stream));
    body = c->dn_place_buf.p;
  }
  if (!round_open) {  // a new round: the records of the last result are about to be overwritten
    c->dn_valid = false;
    c->dn_round = h;
    c->dn_placed.assign(h.shard_count, 0);
    c->dn_round_invalid.assign(c->n_tiles, rene_ctx::DN_TILE_VALID);
  }
  const rene::TileGrid G{c->width, c->height, c->tiles_x, 0u, h.shard_rank, h.shard_count};
  rc = timed_launch("rene_denoise_place_shard", c, [&] { return rene::launch_denoise_shard_place(body, n_owned, c->dn_rec[0].as<float>(), c->dn_guides.as<float>(), c->dn_var.as<float>(), G, c->stream); },
                    [&](float ms) { std::fprintf(stderr, "[rene] denoise shard %u of %u placed, %u tiles, ms: place %.4f\n", h.shard_rank, h.shard_count, n_owned, ms); });
  if (rc != RENE_OK) return rc;
  for (uint32_t i = 0; i < n_owned; ++i)
    c->dn_round_invalid[h.shard_rank + i * h.shard_count] = table[i].valid ? rene_ctx::DN_TILE_VALID : table[i].n_frames;
  c->dn_placed[h.shard_rank] = 1;
  return RENE_OK;
}

static int rene_denoise_place_shard_impl(rene_ctx* c, const void* src, size_t bytes) {
  if (!c || !src) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_denoise_place_shard: NULL argument");
  HIP_TRY(hipSetDevice(c->device));
  return place_shard(c, src, bytes, false);
}

static int rene_denoise_placed_impl(rene_ctx* c) {
  const std::string me = "rene_denoise_placed";
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  HIP_TRY(hipSetDevice(c->device));
  if (c->dn_gather_root >= 0) {  // what rene_gather_denoise left: the receives have been enqueued on the stream by now
    HIP_TRY(wait_stream(c->stream));
    const uint32_t n = (uint32_t)c->comm_ranks;
    size_t off = 0;
    for (uint32_t r = 0; r < n; ++r) {
      const bool own = (int)r == c->dn_gather_root;
      const size_t bytes = own ? c->dn_shard.bytes : rene_denoise_shard_bytes(c->width, c->height, r, n);
      const int rc = place_shard(c, own ? c->dn_shard.buf.p : c->dn_gather_buf.as<char>() + off, bytes, true);
      if (rc != RENE_OK) return rc;
      if (!own) off += bytes;
    }
    c->dn_gather_root = -1;
  }
  std::string missing;
  for (uint32_t r = 0; r < c->dn_placed.size(); ++r)
    if (!c->dn_placed[r]) missing += (missing.empty() ? "" : ", ") + std::to_string(r);
  const bool any = std::find(c->dn_placed.begin(), c->dn_placed.end(), (uint8_t)1) != c->dn_placed.end();
  if (!any) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": no packed buffer has been placed since the last completed filter (rene_denoise_place_shard, rene_gather_denoise)");
  if (!missing.empty())
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": of " + std::to_string(c->dn_placed.size()) + " shards, rank(s) " + missing + " have not been placed since the last completed filter");
  const rene_denoise_params p = c->dn_round.params;
  rene::DenoiseLaunch D{};
  D.grid = rene::TileGrid{c->width, c->height, c->tiles_x, c->n_tiles * rene::TILE_SLOTS, 0u, 1u};
  const int stage_max = denoise_fill_launch(D, p);
  Marks M(c->stream);
  c->dn_valid = false;
  M.mark();
  const int rc = denoise_filter(me, c, D, p, stage_max, true, false, c->dn_round_invalid, M, [&](std::string&, float&) {
    uint32_t n_invalid = 0;
    for (uint32_t v : c->dn_round_invalid) n_invalid += v != rene_ctx::DN_TILE_VALID ? 1u : 0u;
    char buf[160];
    std::snprintf(buf, sizeof buf, "[rene] denoise, placed records of %zu shards, %u x %u, %u invalid tiles", c->dn_placed.size(), c->width, c->height, n_invalid);
    return std::string(buf);
  });
  if (rc != RENE_OK) return rc;
  c->dn_placed.clear();  // the round is over (the records in dn_rec[0] have been filtered over: placing starts again)
  return RENE_OK;
}

// the trimmed prepare's own defaults: the robust resolve's rule with a gain that leaves quiet pixels alone (DESIGN.md section 4c has the study)
void rene_denoise_robust_params_default(rene_robust_params* out) {
  rene_robust_params_default(out);
  if (out) out->gain = 0.35f;
}
int rene_denoise_robust(rene_ctx* c, const rene_denoise_params* params, const rene_robust_params* robust) {
  return guarded([&] { return denoise_run("rene_denoise_robust", c, params, false, true, robust); });
}
int rene_denoise_tiles_robust(rene_ctx* c, const rene_denoise_params* params, const rene_robust_params* robust) {
  return guarded([&] { return denoise_run("rene_denoise_tiles_robust", c, params, true, true, robust); });
}

// ---- the noise estimate (kernels_noise.hip; the metric is specified in include/rene_hip.h) -----------------------------------------------
void rene_noise_params_default(rene_noise_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->luminance_floor = 0.01f;
}

// the derived figures from the additive fields (worst_tile_noise / worst_tile are the caller's)
static void noise_derive(rene_noise_estimate* e) {
  const double n = (double)e->n_pixels;
  e->noise = e->n_pixels ? std::sqrt(e->sum_weighted_q / n) : 0.0;
  e->rel_rmse = e->n_pixels ? std::sqrt(e->sum_var / n) / (e->sum_lum / n + (double)e->luminance_floor) : 0.0;
}

static int rene_estimate_noise_impl(rene_ctx* c, const rene_noise_params* params, rene_noise_estimate* out) {
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_estimate_noise: NULL context");
  if (!out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_estimate_noise: NULL output");
  rene_noise_params p;
  if (int prc = read_params("rene_noise_params", rene_noise_params_default, params, p); prc != RENE_OK) return prc;
  if (!std::isfinite(p.luminance_floor) || !(p.luminance_floor > 0.0f)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_estimate_noise: luminance_floor must be finite and positive");
  uint64_t N = 0;
  uint32_t k = 0;
  float consts[rene::NOISE_SET_FLOATS] = {};
  rene::NoiseLaunch L{};
  int rc = begin_chain_pass("rene_estimate_noise", c, false, L.grid, [&] {
    if (chain_constants(c->chain_frames, consts, &N, &k)) return (int)RENE_OK;
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_estimate_noise: the variance estimate needs frames in at least two of the eight frame chains (render two or more consecutive frames first)");
  });
  if (rc != RENE_OK) return rc;
  const uint32_t n_owned = c->n_work / rene::TILE_SLOTS;
  rc = c->noise_dev.reserve((size_t)n_owned * sizeof(rene_noise_tile), "rene_estimate_noise buffer");
  if (rc != RENE_OK) return rc;
  L.inv_n = consts[0];
  L.inv_km1 = consts[1];
  for (uint32_t g = 0; g < rene::CHAINS; ++g) {
    L.chain_share[g] = consts[2u + g];
    L.chain_inv[g] = consts[2u + rene::CHAINS + g];
  }
  if (c->uneven()) {  // one set of constants per distinct N_t; NOISE_SET_NONE for the tiles of a count that cannot be estimated
    std::vector<uint32_t> counts, tile_set;
    distinct_tile_counts(c, counts, tile_set);
    std::vector<float> sets(counts.size() * rene::NOISE_SET_FLOATS, 0.0f);
    std::vector<uint32_t> set_of(counts.size());
    for (uint32_t s = 0; s < counts.size(); ++s) {
      uint64_t cf[rene::CHAINS];
      rene_ctx::chain_counts(c->frame_base, counts[s], cf);
      set_of[s] = chain_constants(cf, &sets[(size_t)s * rene::NOISE_SET_FLOATS]) ? s : rene::NOISE_SET_NONE;
    }
    for (uint32_t& t : tile_set) t = set_of[t];
    rc = upload_tile_sets(c, sets, tile_set, &L.sets, &L.tile_set);
    if (rc != RENE_OK) return rc;
  }
  c->noise_valid = false;
  std::vector<rene_noise_tile> owned(n_owned);
  if (n_owned) {
    rc = timed_launch("rene_estimate_noise", c, [&] { return rene::launch_noise_tiles(c->chains, c->noise_dev.as<float>(), L, c->stream); }, [&](float ms) {
      std::fprintf(stderr, "[rene] noise estimate %u x %u, %llu frames in %u chains, %u tiles, ms: kernel %.4f\n", c->width, c->height, (unsigned long long)N, k, n_owned, ms);
    });
    if (rc != RENE_OK) return rc;
    HIP_TRY(hipMemcpy(owned.data(), c->noise_dev.p, (size_t)n_owned * sizeof(rene_noise_tile), hipMemcpyDeviceToHost));
  }
  scatter_owned_tiles(c, owned, c->noise_tiles);
  rene_noise_estimate est{};
  est.struct_size = sizeof(est);
  est.n_frames = N;
  est.n_chains = k;
  est.luminance_floor = p.luminance_floor;
  bool have_worst = false;
  for (uint32_t i = 0; i < n_owned; ++i) {  // fp64, in tile order
    const rene_noise_tile& t = owned[i];
    if (t.n_pixels == 0) continue;
    const double nt = (double)t.n_pixels, m = (double)t.sum_lum / nt + (double)p.luminance_floor;
    const double q = ((double)t.sum_var / nt) / (m * m);
    est.n_tiles += 1u;
    est.n_pixels += t.n_pixels;
    est.sum_var += (double)t.sum_var;
    est.sum_lum += (double)t.sum_lum;
    est.sum_weighted_q += nt * q;
    const double tn = std::sqrt(q);
    if (!have_worst || tn > est.worst_tile_noise) {
      est.worst_tile_noise = tn;
      est.worst_tile = c->owned_tile(i);
      have_worst = true;
    }
  }
  noise_derive(&est);
  c->noise_valid = true;
  *out = est;
  return RENE_OK;
}

static int rene_download_noise_tiles_impl(rene_ctx* c, rene_noise_tile* dst, size_t n) {
  if (!c || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_noise_tiles: NULL argument");
  if (!c->noise_valid) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_noise_tiles: no rene_estimate_noise since the context was created or reset");
  if (n < c->noise_tiles.size()) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_noise_tiles: destination too small for the tiles_y x tiles_x grid");
  std::memcpy(dst, c->noise_tiles.data(), c->noise_tiles.size() * sizeof(rene_noise_tile));
  return RENE_OK;
}

// ---- the firefly-robust resolve (kernels_robust.hip; the rule is specified in include/rene_hip.h) ---------------------------------------------------
void rene_robust_params_default(rene_robust_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->max_trim = 3u;
  out->gain = 1.0f;
}

static void robust_derive(rene_robust_summary* s) { s->kept_energy = s->sum_lum_plain != 0.0 ? s->sum_lum_robust / s->sum_lum_plain : 1.0; }

static int rene_resolve_robust_impl(rene_ctx* c, const rene_robust_params* params, rene_robust_summary* out) {
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_resolve_robust: NULL context");
  if (!out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_resolve_robust: NULL output");
  rene_robust_params p;
  if (int prc = read_params("rene_robust_params", rene_robust_params_default, params, p); prc != RENE_OK) return prc;
  if (int prc = check_robust_params("rene_resolve_robust", p); prc != RENE_OK) return prc;
  rene::RobustLaunch L{};
  int rc = begin_chain_pass("rene_resolve_robust", c, true, L.grid, [&] {
    return c->frames ? (int)RENE_OK : fail(RENE_ERR_INVALID_ARGUMENT, "rene_resolve_robust: no frames have been rendered since the context was created or reset");
  });
  if (rc != RENE_OK) return rc;
  const uint32_t n_owned = c->n_owned();
  const size_t n_px = (size_t)c->width * c->height;
  if (!c->robust_img.p) {
    rc = c->robust_img.reserve(std::max<size_t>(16, n_px * 4 * sizeof(float)), "rene_resolve_robust buffer");
    if (rc != RENE_OK) return rc;
    // tiles the context does not own stay zero.  On the context's stream, ahead of the kernel: the stream is non-blocking, so a memset on the
    // null stream is not ordered with it and could clear pixels the first resolve has already written
    const hipError_t e = hipMemsetAsync(c->robust_img.p, 0, c->robust_img.cap, c->stream);
    if (e != hipSuccess) {
      c->robust_img.release();  // (not zeroed: the next call starts again)
      return fail(RENE_ERR_DEVICE, std::string("rene_resolve_robust buffer: ") + hipGetErrorString(e));
    }
  }
  rc = c->robust_dev.reserve(std::max<size_t>(16, (size_t)n_owned * sizeof(rene_robust_tile)), "rene_resolve_robust buffer");
  if (rc != RENE_OK) return rc;
  L.max_trim = p.max_trim;
  L.gain = p.gain;
  rc = fill_chain_counts(c, L.counts);
  if (rc != RENE_OK) return rc;
  uint64_t n_frames = 0;
  for (uint32_t i = 0; i < n_owned; ++i) n_frames = std::max<uint64_t>(n_frames, c->tile_n(i));
  if (n_owned == 0) n_frames = c->frames;
  c->robust_valid = false;
  std::vector<rene_robust_tile> owned(n_owned);
  if (n_owned) {
    rc = timed_launch("rene_resolve_robust", c, [&] { return rene::launch_robust_tiles(c->chains, c->robust_img.as<float>(), c->robust_dev.as<float>(), L, c->stream); }, [&](float ms) {
      std::fprintf(stderr, "[rene] robust resolve %u x %u, %llu frames, %u tiles, ms: kernel %.4f\n", c->width, c->height, (unsigned long long)n_frames, n_owned, ms);
    });
    if (rc != RENE_OK) return rc;
    HIP_TRY(hipMemcpy(owned.data(), c->robust_dev.p, (size_t)n_owned * sizeof(rene_robust_tile), hipMemcpyDeviceToHost));
  }
  scatter_owned_tiles(c, owned, c->robust_tiles);
  rene_robust_summary sum{};
  sum.struct_size = sizeof(sum);
  sum.n_frames = n_frames;
  sum.max_trim = p.max_trim;
  sum.gain = p.gain;
  for (uint32_t i = 0; i < n_owned; ++i) {  // fp64, in tile order
    const rene_robust_tile& t = owned[i];
    if (t.n_pixels == 0) continue;  // (an owned slot block past the image's last tile)
    sum.n_tiles += 1u;
    sum.n_pixels += t.n_pixels;
    sum.n_trimmed += t.n_trimmed;
    sum.sum_lum_plain += (double)t.sum_lum_plain;
    sum.sum_lum_robust += (double)t.sum_lum_robust;
  }
  robust_derive(&sum);
  c->robust_valid = true;
  *out = sum;
  return RENE_OK;
}

static int rene_download_robust_impl(rene_ctx* c, int what, int channels, float* dst, size_t dst_floats) {
  if (!c || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_robust: NULL argument");
  if (what != RENE_ROBUST_IMAGE && what != RENE_ROBUST_TRIM) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_robust: `what` must be RENE_ROBUST_IMAGE or RENE_ROBUST_TRIM");
  const bool image = what == RENE_ROBUST_IMAGE;
  if (image ? (channels != 3 && channels != 4) : channels != 1)
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_robust: channels must be 3 or 4 for the image, 1 for the trim plane");
  const size_t n = (size_t)c->width * c->height;
  if (dst_floats < n * (size_t)channels) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_robust: destination too small");
  if (!c->robust_valid) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_robust: no rene_resolve_robust since the context was created or reset");
  HIP_TRY(hipSetDevice(c->device));
  return staged_download(c, c->robust_img.as<float>(), 4, channels, dst, true, 3);  // (the device record's fourth lane is j: the trim plane; the image's alpha is 0)
}

static int rene_download_robust_tiles_impl(rene_ctx* c, rene_robust_tile* dst, size_t n) {
  if (!c || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_robust_tiles: NULL argument");
  if (!c->robust_valid) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_robust_tiles: no rene_resolve_robust since the context was created or reset");
  if (n < c->robust_tiles.size()) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_robust_tiles: destination too small for the tiles_y x tiles_x grid");
  std::memcpy(dst, c->robust_tiles.data(), c->robust_tiles.size() * sizeof(rene_robust_tile));
  return RENE_OK;
}

int rene_robust_combine(const rene_robust_summary* parts, size_t n, rene_robust_summary* out) {
  if (!parts || !out || n == 0) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_robust_combine: NULL argument or no parts");
  rene_robust_summary s{};
  s.struct_size = sizeof(s);
  for (size_t i = 0; i < n; ++i) {
    const rene_robust_summary& p = parts[i];
    if (p.struct_size != sizeof(rene_robust_summary)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_robust_summary.struct_size mismatch (ABI skew)");
    if (i == 0) {
      s.max_trim = p.max_trim;
      s.gain = p.gain;
    } else if (p.max_trim != s.max_trim || !(p.gain == s.gain)) {
      return fail(RENE_ERR_INVALID_ARGUMENT, "rene_robust_combine: the parts differ in max_trim or gain: they are not shards of one resolve");
    }
    s.n_tiles += p.n_tiles;
    s.n_pixels += p.n_pixels;
    s.n_trimmed += p.n_trimmed;
    s.sum_lum_plain += p.sum_lum_plain;
    s.sum_lum_robust += p.sum_lum_robust;
    s.n_frames = std::max(s.n_frames, p.n_frames);
  }
  robust_derive(&s);
  *out = s;
  return RENE_OK;
}

// ---- the denoiser hand-off (kernels_features.hip; the tensor is specified in include/rene_hip.h) ---------------------------------------------------
static constexpr uint32_t kFeatureAll = RENE_FEATURE_COLOR | RENE_FEATURE_ALBEDO | RENE_FEATURE_NORMAL | RENE_FEATURE_VARIANCE | RENE_FEATURE_HALF_A |
                                        RENE_FEATURE_HALF_B | RENE_FEATURE_FRAMES;

void rene_feature_params_default(rene_feature_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->features = RENE_FEATURE_COLOR | RENE_FEATURE_ALBEDO | RENE_FEATURE_NORMAL;
  out->format = RENE_FEATURES_F32;
  out->layout = RENE_FEATURES_HWC;
}

uint32_t rene_feature_channels(uint32_t features) {
  if (features == 0 || (features & ~kFeatureAll)) return 0;
  uint32_t n = 0;
  for (uint32_t three : {RENE_FEATURE_COLOR, RENE_FEATURE_ALBEDO, RENE_FEATURE_NORMAL, RENE_FEATURE_HALF_A, RENE_FEATURE_HALF_B})
    if (features & three) n += 3;
  for (uint32_t one : {RENE_FEATURE_VARIANCE, RENE_FEATURE_FRAMES})
    if (features & one) n += 1;
  return n;
}

static int rene_export_features_impl(rene_ctx* c, const rene_feature_params* params, void* device_dst, size_t dst_bytes) {
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_export_features: NULL context");
  rene_feature_params p;
  if (int prc = read_params("rene_feature_params", rene_feature_params_default, params, p); prc != RENE_OK) return prc;
  const uint32_t channels = rene_feature_channels(p.features);
  if (channels == 0) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_export_features: the feature mask is empty or has unknown bits");
  if (p.format != RENE_FEATURES_F32 && p.format != RENE_FEATURES_F16) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_export_features: format must be RENE_FEATURES_F32 or RENE_FEATURES_F16");
  if (p.layout != RENE_FEATURES_CHW && p.layout != RENE_FEATURES_HWC) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_export_features: layout must be RENE_FEATURES_CHW or RENE_FEATURES_HWC");
  const size_t elem = p.format == RENE_FEATURES_F16 ? 2 : 4;
  const size_t need = (size_t)channels * c->width * c->height * elem;
  rene::FeatureLaunch L{};
  int rc = begin_chain_pass("rene_export_features", c, true, L.grid, [&] {
    return device_dst ? check_device_destination("rene_export_features", c->device, device_dst, dst_bytes, need, "channels x height x width x element size", elem,
                                                 "aligned to its element size")
                      : (int)RENE_OK;
  });
  if (rc != RENE_OK) return rc;
  void* dst = device_dst;
  if (!device_dst)
    if (rc = c->features.begin(need, {p.features, p.format, p.layout}, c->stream, "rene_export_features buffer", dst); rc != RENE_OK) return rc;
  const uint32_t n_owned = c->n_owned();
  L.features = p.features;
  L.channels = channels;
  rc = fill_chain_counts(c, L.counts);
  if (rc != RENE_OK) return rc;
  rc = timed_launch("rene_export_features", c, [&] { return rene::launch_features(c->chains, c->fb, dst, (int)p.format, (int)p.layout, L, c->stream); }, [&](float ms) {
    std::fprintf(stderr, "[rene] feature export %u x %u x %u, %s %s, %u tiles, ms: kernel %.4f\n", channels, c->height, c->width, p.format == RENE_FEATURES_F16 ? "f16" : "f32",
                 p.layout == RENE_FEATURES_HWC ? "hwc" : "chw", n_owned, ms);
  });
  if (rc != RENE_OK) return rc;
  if (!device_dst) c->features.commit(need);
  return RENE_OK;
}

// ---- the output transform on the device (kernels_output.hip; the bytes are specified in include/rene_hip.h) ----------------------------------------
static const float* output_threshold_table();  // (below, beside rene_to_rgb8, from which it is derived)

void rene_output_params_default(rene_output_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->source = RENE_OUTPUT_RADIANCE;
  out->format = RENE_OUTPUT_RGB8;
}

// What every call that reads one of the images a context hands out (rene_output_8bit, rene_output_tonemapped, rene_luminance_histogram,
// rene_output_exr) shares, in three steps.  First the refusals of a source, before anything waits or launches:
static int check_output_source(const std::string& me, rene_ctx* c, uint32_t source) {
  const bool denoised = source == RENE_OUTPUT_DENOISED || source == RENE_OUTPUT_DENOISED_MEAN;
  if (denoised && c->opts.shard_count > 1)
    return fail(RENE_ERR_UNSUPPORTED, me + ": the denoised image is a whole image; a context with shard_count > 1 writes only the tiles it owns");
  if (denoised && !c->dn_valid) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": no rene_denoise since the context was created or reset");
  if (source == RENE_OUTPUT_DENOISED && c->uneven())
    return fail(RENE_ERR_UNSUPPORTED, me + ": the context's tiles differ in their frame counts (rene_set_active_tiles) and RENE_OUTPUT_DENOISED divides by one count; "
                                           "RENE_OUTPUT_DENOISED_MEAN is the source for such a job");
  if (source == RENE_OUTPUT_ROBUST && !c->robust_valid) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": no rene_resolve_robust since the context was created or reset");
  return RENE_OK;
}
// ... then, behind the drain, the image of a source as a kernel reads it: its [H][W][4] layer, and in row[0 .. n_tiles) its divisors, one per tile
// of the image's full grid (RENE_OUTPUT_DENOISED_MEAN launches the mean into the free ping-pong buffer)
static int output_source_layer(const std::string& me, rene_ctx* c, uint32_t source, const float*& layer, uint32_t* row) {
  const size_t n_px = (size_t)c->width * c->height;
  std::fill(row, row + c->n_tiles, 1u);
  if (source <= RENE_OUTPUT_ALBEDO) {
    layer = c->fb + (size_t)source * n_px * 4;
    std::fill(row, row + c->n_tiles, 0u);
    for (uint32_t k = 0; k < c->n_owned(); ++k)
      if (c->owned_tile(k) < c->n_tiles) row[c->owned_tile(k)] = c->tile_n(k);
  } else if (source == RENE_OUTPUT_DENOISED) {
    layer = c->dn_out.as<float>();
    std::fill(row, row + c->n_tiles, (uint32_t)std::min<uint64_t>(c->frames, 0xffffffffull));
  } else if (source == RENE_OUTPUT_ROBUST) {
    layer = c->robust_img.as<float>();  // a mean already
  } else {  // RENE_DENOISED_MEAN as rene_download_denoised makes it: col * den into the free ping-pong buffer; the invalid tiles hold unfiltered sums
    float* mean = c->dn_rec[c->dn_cur ^ 1u].as<float>();
    const hipError_t e = rene::launch_denoise_mean(c->dn_rec[c->dn_cur].as<float>(), c->dn_guides.as<float>(), mean, c->width, c->height, c->dn_albedo_floor, c->dn_masked, c->stream);
    if (e != hipSuccess) return launch_failed(me, c, e);
    layer = mean;
    if (c->dn_masked && c->dn_invalid_frames.size() == c->n_tiles)
      for (uint32_t t = 0; t < c->n_tiles; ++t)
        if (c->dn_invalid_frames[t] != rene_ctx::DN_TILE_VALID) row[t] = c->dn_invalid_frames[t];
  }
  return RENE_OK;
}
// ... and the divisor rows on the device, in the context's buffer
static int upload_tile_divisors(const std::string& me, rene_ctx* c, const std::vector<uint32_t>& frames, const uint32_t*& device) {
  int rc = c->tile_frames_dev.reserve(std::max<size_t>(16, frames.size() * sizeof(uint32_t)), me + " buffer");
  if (rc != RENE_OK) return rc;
  HIP_TRY(hipMemcpyAsync(c->tile_frames_dev.p, frames.data(), frames.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(wait_stream(c->stream));  // (`frames` is pageable memory of the caller's scope)
  device = c->tile_frames_dev.as<uint32_t>();
  return RENE_OK;
}

// The three for one source: its refusals and `more` (the caller's remaining checks), the drain, then L's layer, the divisors of the full tile grid
// (uploaded), the film and the shard.  L.dst and L.thresholds are the caller's to fill.
static int output_source(const std::string& me, rene_ctx* c, uint32_t source, rene::OutputLaunch& L, const std::function<int()>& more) {
  rene::TileGrid G{};
  int rc = begin_chain_pass(me.c_str(), c, false, G, [&] {
    if (int r = check_output_source(me, c, source); r != RENE_OK) return r;
    return more();
  });  // (... and the drain: waits for the launches issued so far and resolves the image)
  if (rc != RENE_OK) return rc;
  std::vector<uint32_t> frames(c->n_tiles, 1u);
  if (rc = output_source_layer(me, c, source, L.layer, frames.data()); rc != RENE_OK) return rc;
  L.width = c->width;
  L.height = c->height;
  L.tiles_x = c->tiles_x;
  L.n_tiles = c->n_tiles;
  L.shard_rank = G.shard_rank;
  L.shard_count = G.shard_count;
  L.shard_inv = G.shard_count > 1u ? (uint32_t)(0x100000000ull / G.shard_count) : 0u;
  if ((size_t)c->width * c->height == 0) return RENE_OK;  // (an empty film: nothing to read)
  return upload_tile_divisors(me, c, frames, L.tile_frames);
}

// the sRGB thresholds on the device, uploaded by the context's first call that needs them
static int upload_output_thresholds(const std::string& me, rene_ctx* c) {
  if (c->out_thresholds.p) return RENE_OK;
  if (int rc = c->out_thresholds.reserve(256 * sizeof(float), me + " thresholds"); rc != RENE_OK) return rc;
  const hipError_t e = hipMemcpy(c->out_thresholds.p, output_threshold_table(), 255 * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    c->out_thresholds.release();
    return fail(RENE_ERR_DEVICE, me + " thresholds: " + hipGetErrorString(e));
  }
  return RENE_OK;
}

// The body of rene_output_8bit and rene_output_tonemapped behind the checks of their own parameters: `source` through launch(L) into the caller's
// destination or the library's buffer, [H][W][3 or 4] bytes.  `what` goes into the RENE_DEBUG line behind the format.
static int output_image(const std::string& me, rene_ctx* c, uint32_t source, uint32_t format, bool srgb, void* device_dst, size_t dst_bytes, const std::string& what,
                        const std::function<hipError_t(const rene::OutputLaunch&)>& launch) {
  const size_t n_px = (size_t)c->width * c->height, need = n_px * (format == RENE_OUTPUT_RGBA8 ? 4u : 3u);
  rene::OutputLaunch L{};
  int rc = output_source(me, c, source, L, [&] { return device_dst ? check_device_destination(me, c->device, device_dst, dst_bytes, need, kImageBytes, 4, "4-byte aligned") : (int)RENE_OK; });
  if (rc != RENE_OK) return rc;
  if (srgb)
    if (rc = upload_output_thresholds(me, c); rc != RENE_OK) return rc;
  if (n_px == 0) return RENE_OK;  // (an empty film: nothing to transform)
  void* dst = device_dst;
  if (!device_dst)
    if (rc = c->out.begin(need, {format}, c->stream, me + " buffer", dst); rc != RENE_OK) return rc;
  L.dst = dst;
  L.thresholds = c->out_thresholds.as<float>();
  rc = timed_launch(me.c_str(), c, [&] { return launch(L); }, [&](float ms) {
    std::fprintf(stderr, "[rene] output %u x %u, source %u, %s%s, ms: kernel %.4f\n", c->width, c->height, source, format == RENE_OUTPUT_RGBA8 ? "rgba8" : "rgb8", what.c_str(), ms);
  });
  if (rc != RENE_OK) return rc;
  if (!device_dst) c->out.commit(need);
  return RENE_OK;
}

static int rene_output_8bit_impl(rene_ctx* c, const rene_output_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_output_8bit";
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  rene_output_params p;
  if (int prc = read_params("rene_output_params", rene_output_params_default, params, p); prc != RENE_OK) return prc;
  if (p.source > RENE_OUTPUT_ROBUST) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": source must be RENE_OUTPUT_RADIANCE .. RENE_OUTPUT_ROBUST");
  if (p.format != RENE_OUTPUT_RGB8 && p.format != RENE_OUTPUT_RGBA8) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": format must be RENE_OUTPUT_RGB8 or RENE_OUTPUT_RGBA8");
  int transform = RENE_OUTPUT_SRGB;
  if (p.source == RENE_OUTPUT_NORMAL) transform = RENE_OUTPUT_AOV_NORMAL;
  if (p.source == RENE_OUTPUT_ALBEDO) transform = RENE_OUTPUT_AOV;
  return output_image(me, c, p.source, p.format, transform == RENE_OUTPUT_SRGB, device_dst, dst_bytes, "",
                      [&](const rene::OutputLaunch& L) { return rene::launch_output(L, transform, (int)p.format, c->stream); });
}

// ---- tone-mapped output and the luminance histogram (kernels_tonemap.hip, kernels_luminance.hip; specified in include/rene_hip.h) --------------------
void rene_tonemap_params_default(rene_tonemap_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->source = RENE_OUTPUT_RADIANCE;
  out->format = RENE_OUTPUT_RGB8;
  out->op = RENE_TONEMAP_CLAMP;
  out->scale = 1.0f;
  out->white = 4.0f;
}

static bool finite_positive(float v) { return std::isfinite(v) && v > 0.0f; }
static const char* const TONEMAP_NAMES[] = {"clamp", "reinhard", "aces"};
// the refusals rene_output_tonemapped, rene_tonemap_rgb8 and rene_tonemap_probe share
static int check_tonemap(const std::string& me, uint32_t op, float scale, float white) {
  if (op > RENE_TONEMAP_ACES) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": op must be RENE_TONEMAP_CLAMP, RENE_TONEMAP_REINHARD or RENE_TONEMAP_ACES");
  if (!finite_positive(scale)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": scale must be finite and greater than 0");
  if (!finite_positive(white)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": white must be finite and greater than 0");
  return RENE_OK;
}
static int check_tonemap_source(const std::string& me, uint32_t source) {
  if (source > RENE_OUTPUT_ROBUST) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": source must be RENE_OUTPUT_RADIANCE, _DENOISED, _DENOISED_MEAN or _ROBUST");
  if (source == RENE_OUTPUT_NORMAL || source == RENE_OUTPUT_ALBEDO)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": RENE_OUTPUT_NORMAL and RENE_OUTPUT_ALBEDO are not radiance; rene_output_8bit transforms them");
  return RENE_OK;
}

static int rene_output_tonemapped_impl(rene_ctx* c, const rene_tonemap_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_output_tonemapped";
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  rene_tonemap_params p;
  if (int prc = read_params("rene_tonemap_params", rene_tonemap_params_default, params, p); prc != RENE_OK) return prc;
  if (int rc = check_tonemap_source(me, p.source); rc != RENE_OK) return rc;
  if (p.format != RENE_OUTPUT_RGB8 && p.format != RENE_OUTPUT_RGBA8) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": format must be RENE_OUTPUT_RGB8 or RENE_OUTPUT_RGBA8");
  if (int rc = check_tonemap(me, p.op, p.scale, p.white); rc != RENE_OK) return rc;
  char what[96];
  std::snprintf(what, sizeof(what), ", %s, scale %.9g, white %.9g", TONEMAP_NAMES[p.op], (double)p.scale, (double)p.white);
  return output_image(me, c, p.source, p.format, true, device_dst, dst_bytes, what, [&](const rene::OutputLaunch& L) {
    return rene::launch_tonemap(rene::TonemapLaunch{L, p.scale, p.white * p.white}, (int)p.op, (int)p.format, c->stream);
  });
}

static int rene_luminance_histogram_impl(rene_ctx* c, uint32_t source, rene_luminance_stats* out) {
  const std::string me = "rene_luminance_histogram";
  if (!c || !out) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (int rc = check_tonemap_source(me, source); rc != RENE_OK) return rc;
  rene::OutputLaunch O{};
  if (int rc = output_source(me, c, source, O, [] { return (int)RENE_OK; }); rc != RENE_OK) return rc;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  const size_t n_px = (size_t)c->width * c->height;
  if (n_px == 0) return RENE_OK;
  // the pixels the launch looks at: those of the owned tiles inside the image
  uint64_t looked_at = 0;
  for (uint32_t k = 0; k < c->n_owned(); ++k) {
    const uint32_t t = c->owned_tile(k);
    if (t >= c->n_tiles) continue;
    const uint32_t tx = t % c->tiles_x, ty = t / c->tiles_x;
    looked_at += (uint64_t)std::min<uint32_t>(RENE_TILE_SIZE, c->width - tx * RENE_TILE_SIZE) * std::min<uint32_t>(RENE_TILE_SIZE, c->height - ty * RENE_TILE_SIZE);
  }
  rene::LuminanceLaunch L{};
  // a grid sized to the chip, every workgroup striding over the image: four workgroups of 256 threads per CU (every one is a row the second launch
  // adds), and no more than the image has runs of 1024 pixels
  L.groups = (uint32_t)std::min<size_t>((n_px + 4u * rene::LUM_BLOCK - 1) / (4u * rene::LUM_BLOCK), (size_t)std::max(1u, c->cfg.cus) * 4u);
  if (int rc = c->lum_rows.reserve(((size_t)L.groups + 1) * rene::LUM_ROW * sizeof(uint32_t), me + " buffer"); rc != RENE_OK) return rc;
  L.layer = O.layer;
  L.tile_frames = O.tile_frames;
  L.rows = c->lum_rows.as<uint32_t>();
  L.out = L.rows + (size_t)L.groups * rene::LUM_ROW;  // the sum, behind the rows
  L.width = O.width, L.height = O.height, L.tiles_x = O.tiles_x, L.n_tiles = O.n_tiles;
  L.shard_rank = O.shard_rank, L.shard_count = O.shard_count, L.shard_inv = O.shard_inv;
  int rc = timed_launch(me.c_str(), c, [&] { return rene::launch_luminance(L, c->stream); }, [&](float ms) {
    std::fprintf(stderr, "[rene] luminance histogram %u x %u, source %u, %u workgroups, ms: kernels %.4f\n", c->width, c->height, source, L.groups, ms);
  });
  if (rc != RENE_OK) return rc;
  uint32_t sums[rene::LUM_ROW];
  HIP_TRY(hipMemcpy(sums, L.out, sizeof(sums), hipMemcpyDeviceToHost));
  std::memcpy(out->counts, sums, sizeof(out->counts));
  out->n_dark = sums[rene::LUM_BINS];
  out->n_pixels = (uint32_t)looked_at;  // (a film has at most 2^28 pixels)
  return RENE_OK;
}

static int rene_tonemap_probe_impl(int device, uint32_t op, float scale, float white, size_t n, const float* rgb, uint8_t* out) {
  if (n && (!rgb || !out)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_tonemap_probe: NULL argument");
  if (int rc = check_tonemap("rene_tonemap_probe", op, scale, white); rc != RENE_OK) return rc;
  if (n == 0) return RENE_OK;
  int n_dev = 0;
  HIP_TRY(hipGetDeviceCount(&n_dev));
  if (device < 0 || device >= n_dev) return fail(n_dev <= 0 ? RENE_ERR_DEVICE : RENE_ERR_INVALID_ARGUMENT, "rene_tonemap_probe: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  return run_probe("rene_tonemap_probe", nullptr, {{rgb, 3 * n * sizeof(float)}, {output_threshold_table(), 255 * sizeof(float)}}, {{out, 3 * n}}, [&](void** d) {
    return rene::launch_tonemap_probe((int)op, scale, white * white, n, (const float*)d[0], (uint8_t*)d[2], (const float*)d[1], nullptr);
  });
}

static int rene_output_probe_impl(int device, int transform, size_t n, const float* v, uint8_t* out) {
  if (n && (!v || !out)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_output_probe: NULL argument");
  if (transform != RENE_OUTPUT_SRGB && transform != RENE_OUTPUT_AOV && transform != RENE_OUTPUT_AOV_NORMAL)
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_output_probe: transform must be RENE_OUTPUT_SRGB, RENE_OUTPUT_AOV or RENE_OUTPUT_AOV_NORMAL");
  if (n == 0) return RENE_OK;
  int n_dev = 0;
  HIP_TRY(hipGetDeviceCount(&n_dev));
  if (device < 0 || device >= n_dev) return fail(n_dev <= 0 ? RENE_ERR_DEVICE : RENE_ERR_INVALID_ARGUMENT, "rene_output_probe: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  return run_probe("rene_output_probe", nullptr, {{v, n * sizeof(float)}, {output_threshold_table(), 255 * sizeof(float)}}, {{out, n}}, [&](void** d) {
    return rene::launch_output_probe(transform, n, (const float*)d[0], (uint8_t*)d[2], (const float*)d[1], nullptr);
  });
}

// ---- the geometry pass (kernels_gbuffer.hip; specified in include/rene_hip.h) ------------------------------------------------------------------------
void rene_gbuffer_params_default(rene_gbuffer_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->first_frame = 0;
  out->n_frames = 16;
  out->id_source = RENE_GBUFFER_ID_INSTANCE;
}
size_t rene_gbuffer_bytes(uint32_t width, uint32_t height) { return (size_t)width * height * sizeof(rene_gbuffer_pixel); }

static int rene_gbuffer_impl(rene_ctx* c, const rene_gbuffer_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_gbuffer";
  rene_gbuffer_params p;
  if (int prc = read_params("rene_gbuffer_params", rene_gbuffer_params_default, params, p); prc != RENE_OK) return prc;
  if (p.n_frames < 1u || p.n_frames > RENE_GBUFFER_MAX_FRAMES) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n_frames must be 1 .. 65536");
  if (p.id_source > RENE_GBUFFER_ID_PRIMITIVE) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": id_source must be RENE_GBUFFER_ID_INSTANCE, _MATERIAL or _PRIMITIVE");
  if (p.flags != 0u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": flags must be 0");
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");  // (behind the parameters, which are checked without a GPU)
  const int rc = run_pixel_pass(me, c, p.first_frame, p.n_frames, sizeof(rene_gbuffer_pixel), &rene_ctx::gbuf, device_dst, dst_bytes, [&](const uint32_t* seeds, void* dst) {
    return rene::launch_gbuffer(c->cfg, c->view, rene::GbufferLaunch{tile_grid(c), seeds, p.n_frames, p.id_source, dst}, false, c->stream);
  }, [&](float ms) {
    std::fprintf(stderr, "[rene] gbuffer %u x %u, frames %u + %u, ids %u, ms: kernel %.4f\n", c->width, c->height, p.first_frame, p.n_frames, p.id_source, ms);
  });
  if (rc == RENE_OK && !device_dst) c->gbuf_id_source = p.id_source;  // (what rene_output_cryptomatte asks of the library-owned records)
  return rc;
}

static int rene_primary_hits_impl(rene_ctx* c, uint32_t first_frame, uint32_t n_frames, rene_primary_hit* host_dst, size_t n) {
  const std::string me = "rene_primary_hits";
  if (n_frames < 1u || n_frames > RENE_GBUFFER_MAX_FRAMES) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n_frames must be 1 .. 65536");
  if (!c || !host_dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  return run_pixel_pass_samples(me, c, first_frame, n_frames, 1, sizeof(rene_primary_hit), 24, "samples", "n_frames x width x height", host_dst, n, [&](const uint32_t* seeds, void* dst) {
    return rene::launch_gbuffer(c->cfg, c->view, rene::GbufferLaunch{tile_grid(c), seeds, n_frames, RENE_GBUFFER_ID_INSTANCE, dst}, true, c->stream);
  });
}

// ---- the occlusion pass (kernels_occlusion.hip; specified in include/rene_hip.h) ----------------------------------------------------------------------
void rene_occlusion_params_default(rene_occlusion_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->first_frame = 0;
  out->n_frames = 16;
  out->rays = 1;
  out->radius = 1.0f;
}
size_t rene_occlusion_bytes(uint32_t width, uint32_t height) { return (size_t)width * height * sizeof(rene_occlusion_pixel); }

// the parameters of either call, checked without a GPU
static int occlusion_read_params(const std::string& me, const rene_occlusion_params* params, rene_occlusion_params& p) {
  if (int prc = read_params("rene_occlusion_params", rene_occlusion_params_default, params, p); prc != RENE_OK) return prc;
  if (p.n_frames < 1u || p.n_frames > RENE_OCCLUSION_MAX_FRAMES) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n_frames must be 1 .. 65536");
  if (p.rays < 1u || p.rays > RENE_OCCLUSION_MAX_RAYS) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": rays must be 1 .. 64");
  if (!std::isfinite(p.radius) || !(p.radius > 0.001f) || !(p.radius <= 100000.0f))
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": radius must be finite, above 0.001 and at most 100000");
  if (p.flags != 0u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": flags must be 0");
  return RENE_OK;
}

static int rene_occlusion_impl(rene_ctx* c, const rene_occlusion_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_occlusion";
  rene_occlusion_params p;
  if (int prc = occlusion_read_params(me, params, p); prc != RENE_OK) return prc;
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");  // (behind the parameters, which are checked without a GPU)
  return run_pixel_pass(me, c, p.first_frame, p.n_frames, sizeof(rene_occlusion_pixel), &rene_ctx::occl, device_dst, dst_bytes, [&](const uint32_t* seeds, void* dst) {
    return rene::launch_occlusion(c->cfg, c->view, rene::OcclusionLaunch{tile_grid(c), seeds, p.n_frames, p.rays, p.radius, dst}, false, c->stream);
  }, [&](float ms) {
    std::fprintf(stderr, "[rene] occlusion %u x %u, frames %u + %u, rays %u, radius %g, ms: kernel %.4f\n", c->width, c->height, p.first_frame, p.n_frames, p.rays,
                 (double)p.radius, ms);
  });
}

static int rene_occlusion_samples_impl(rene_ctx* c, const rene_occlusion_params* params, rene_occlusion_sample* host_dst, size_t n) {
  const std::string me = "rene_occlusion_samples";
  rene_occlusion_params p;
  if (int prc = occlusion_read_params(me, params, p); prc != RENE_OK) return prc;
  if (!c || !host_dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  return run_pixel_pass_samples(me, c, p.first_frame, p.n_frames, p.rays, sizeof(rene_occlusion_sample), 22, "records", "n_frames x rays x width x height", host_dst, n,
                                [&](const uint32_t* seeds, void* dst) {
    return rene::launch_occlusion(c->cfg, c->view, rene::OcclusionLaunch{tile_grid(c), seeds, p.n_frames, p.rays, p.radius, dst}, true, c->stream);
  });
}

// ---- the direct-light pass (kernels_direct.hip; specified in include/rene_hip.h) ----------------------------------------------------------------------
void rene_direct_params_default(rene_direct_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->first_frame = 0;
  out->n_frames = 16;
}
size_t rene_direct_bytes(uint32_t width, uint32_t height) { return (size_t)width * height * sizeof(rene_direct_pixel); }

// the parameters of either call and the context's scene, checked without a GPU
static int direct_read_params(const std::string& me, const rene_ctx* c, bool need_dst, const void* host_dst, const rene_direct_params* params, rene_direct_params& p) {
  if (int prc = read_params("rene_direct_params", rene_direct_params_default, params, p); prc != RENE_OK) return prc;
  if (p.n_frames < 1u || p.n_frames > RENE_DIRECT_MAX_FRAMES) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n_frames must be 1 .. 65536");
  if (p.flags != 0u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": flags must be 0");
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");  // (behind the parameters, which are checked without a GPU)
  if (need_dst && !host_dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (c->cfg.features & rene::FEAT_VOLPATH)
    return fail(RENE_ERR_UNSUPPORTED, me + ": the scene selects the volpath integrator, whose estimator the pass does not replay; path-integrator scenes only");
  return RENE_OK;
}
// either call's launch: the pass's records, or (samples) the probe's
static hipError_t direct_launch(rene_ctx* c, const rene_direct_params& p, bool samples, const uint32_t* seeds, void* dst) {
  const uint32_t background = (c->cfg.features & rene::FEAT_BACKGROUND) ? 1u : 0u;
  return rene::launch_direct(c->cfg, c->view, rene::DirectLaunch{tile_grid(c), seeds, p.n_frames, background, dst}, samples, c->stream);
}

static int rene_direct_impl(rene_ctx* c, const rene_direct_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_direct";
  rene_direct_params p;
  if (int prc = direct_read_params(me, c, false, nullptr, params, p); prc != RENE_OK) return prc;
  const int rc = run_pixel_pass(me, c, p.first_frame, p.n_frames, sizeof(rene_direct_pixel), &rene_ctx::direct, device_dst, dst_bytes,
                                [&](const uint32_t* seeds, void* dst) { return direct_launch(c, p, false, seeds, dst); }, [&](float ms) {
    std::fprintf(stderr, "[rene] direct %u x %u, frames %u + %u, ms: kernel %.4f\n", c->width, c->height, p.first_frame, p.n_frames, ms);
  });
  if (rc == RENE_OK && !device_dst) c->direct_first_frame = p.first_frame, c->direct_n_frames = p.n_frames;  // (what rene_output_exr_passes asks of the library-owned records)
  return rc;
}

static int rene_direct_samples_impl(rene_ctx* c, const rene_direct_params* params, rene_direct_sample* host_dst, size_t n) {
  const std::string me = "rene_direct_samples";
  rene_direct_params p;
  if (int prc = direct_read_params(me, c, true, host_dst, params, p); prc != RENE_OK) return prc;
  return run_pixel_pass_samples(me, c, p.first_frame, p.n_frames, 1, sizeof(rene_direct_sample), 22, "records", "n_frames x width x height", host_dst, n,
                                [&](const uint32_t* seeds, void* dst) { return direct_launch(c, p, true, seeds, dst); });
}

// ---- the bounce pass (kernels_bounces.hip; specified in include/rene_hip.h) ---------------------------------------------------------------------------
void rene_bounces_params_default(rene_bounces_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->first_frame = 0;
  out->n_frames = 16;
  out->max_depth = 0;
}
size_t rene_bounces_bytes(uint32_t width, uint32_t height) { return (size_t)width * height * sizeof(rene_bounces_pixel); }

// the parameters of either call and the context's scene, checked without a GPU; p.max_depth leaves as the cap itself, 1 .. 50
static int bounces_read_params(const std::string& me, const rene_ctx* c, bool need_dst, const void* host_dst, const rene_bounces_params* params, rene_bounces_params& p) {
  if (int prc = read_params("rene_bounces_params", rene_bounces_params_default, params, p); prc != RENE_OK) return prc;
  if (p.n_frames < 1u || p.n_frames > RENE_BOUNCES_MAX_FRAMES) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n_frames must be 1 .. 65536");
  if (p.max_depth > RENE_BOUNCES_MAX_DEPTH) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": max_depth must be 1 .. 50, or 0 for 50");
  if (p.flags != 0u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": flags must be 0");
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");  // (behind the parameters, which are checked without a GPU)
  if (need_dst && !host_dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (c->cfg.features & rene::FEAT_VOLPATH)
    return fail(RENE_ERR_UNSUPPORTED, me + ": the scene selects the volpath integrator, whose estimator the pass does not replay; path-integrator scenes only");
  if (p.max_depth == 0u) p.max_depth = RENE_BOUNCES_MAX_DEPTH;
  return RENE_OK;
}
// either call's launch: the pass's records, or (samples) the probe's
static hipError_t bounces_launch(rene_ctx* c, const rene_bounces_params& p, bool samples, const uint32_t* seeds, void* dst) {
  const uint32_t background = (c->cfg.features & rene::FEAT_BACKGROUND) ? 1u : 0u;
  return rene::launch_bounces(c->cfg, c->view, rene::BouncesLaunch{tile_grid(c), seeds, p.n_frames, background, p.max_depth, dst}, samples, c->stream);
}

static int rene_bounces_impl(rene_ctx* c, const rene_bounces_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_bounces";
  rene_bounces_params p;
  if (int prc = bounces_read_params(me, c, false, nullptr, params, p); prc != RENE_OK) return prc;
  return run_pixel_pass(me, c, p.first_frame, p.n_frames, sizeof(rene_bounces_pixel), &rene_ctx::bounces, device_dst, dst_bytes,
                        [&](const uint32_t* seeds, void* dst) { return bounces_launch(c, p, false, seeds, dst); }, [&](float ms) {
    std::fprintf(stderr, "[rene] bounces %u x %u, frames %u + %u, max depth %u, ms: kernel %.4f\n", c->width, c->height, p.first_frame, p.n_frames, p.max_depth, ms);
  });
}

static int rene_bounces_samples_impl(rene_ctx* c, const rene_bounces_params* params, rene_bounces_sample* host_dst, size_t n) {
  const std::string me = "rene_bounces_samples";
  rene_bounces_params p;
  if (int prc = bounces_read_params(me, c, true, host_dst, params, p); prc != RENE_OK) return prc;
  return run_pixel_pass_samples(me, c, p.first_frame, p.n_frames, 1, sizeof(rene_bounces_sample), 20, "records", "n_frames x width x height", host_dst, n,
                                [&](const uint32_t* seeds, void* dst) { return bounces_launch(c, p, true, seeds, dst); });
}

// ---- the light-group pass (kernels_lights.hip; specified in include/rene_hip.h) ----------------------------------------------------------------------
void rene_lights_params_default(rene_lights_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->first_frame = 0;
  out->n_frames = 16;
}
size_t rene_lights_bytes(uint32_t width, uint32_t height) { return (size_t)width * height * sizeof(rene_lights_pixel); }

// the library's grouping of c's scene: the background, the distant lights, the emitting instances, the overflow in the last group; returns the
// groups it uses
static uint32_t lights_default_groups(const rene_ctx* c, uint8_t* instance_group, uint8_t* distant_group, uint8_t& background_group) {
  const uint32_t last = RENE_LIGHTS_GROUPS - 1u;
  uint32_t next = 1u;
  background_group = 0;
  for (uint32_t li = 0; li < c->view.lights_len; ++li) distant_group[li] = (uint8_t)std::min(next++, last);
  for (size_t k = 0; k < c->inst_emits.size(); ++k) instance_group[k] = c->inst_emits[k] ? (uint8_t)std::min(next++, last) : 0;
  return std::min(next, RENE_LIGHTS_GROUPS);
}

static int rene_lights_default_groups_impl(rene_ctx* c, uint8_t* instance_group, uint32_t n_instances, uint8_t* distant_group, uint32_t n_distant,
                                           uint8_t* background_group, uint32_t* n_used) {
  const std::string me = "rene_lights_default_groups";
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  if (n_instances != c->inst_emits.size() || n_distant != c->view.lights_len)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n_instances / n_distant are not the scene's " + std::to_string(c->inst_emits.size()) + " instances and " +
                                               std::to_string(c->view.lights_len) + " distant lights");
  if ((n_instances && !instance_group) || (n_distant && !distant_group)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL table");
  uint8_t bg = 0;
  const uint32_t used = lights_default_groups(c, instance_group, distant_group, bg);
  if (background_group) *background_group = bg;
  if (n_used) *n_used = used;
  return RENE_OK;
}

// the parameters of either call and the context's scene, checked without a GPU; `tables` leaves as the call's grouping -- the caller's, or the
// library's where the params name none -- instance_group, then distant_group
static int lights_read_params(const std::string& me, const rene_ctx* c, bool need_dst, const void* host_dst, const rene_lights_params* params, rene_lights_params& p,
                              std::vector<uint8_t>& tables) {
  if (int prc = read_params("rene_lights_params", rene_lights_params_default, params, p); prc != RENE_OK) return prc;
  if (p.n_frames < 1u || p.n_frames > RENE_LIGHTS_MAX_FRAMES) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n_frames must be 1 .. 65536");
  if (p.flags != 0u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": flags must be 0");
  const bool own = !p.instance_group && !p.distant_group && p.n_instances == 0u && p.n_distant == 0u;  // the library's grouping
  if ((p.n_instances && !p.instance_group) || (p.n_distant && !p.distant_group)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a NULL table with a count above 0");
  for (uint32_t k = 0; k < p.n_instances; ++k)
    if (p.instance_group[k] >= RENE_LIGHTS_GROUPS) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": instance_group[" + std::to_string(k) + "] must be below 8");
  for (uint32_t k = 0; k < p.n_distant; ++k)
    if (p.distant_group[k] >= RENE_LIGHTS_GROUPS) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": distant_group[" + std::to_string(k) + "] must be below 8");
  if (!own && p.background_group >= RENE_LIGHTS_GROUPS) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": background_group must be below 8");
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");  // (behind the parameters, which are checked without a GPU)
  if (need_dst && !host_dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (c->cfg.features & rene::FEAT_VOLPATH)
    return fail(RENE_ERR_UNSUPPORTED, me + ": the scene selects the volpath integrator, whose estimator the pass does not replay; path-integrator scenes only");
  const size_t n_inst = c->inst_emits.size(), n_dist = c->view.lights_len;
  if (!own && (p.n_instances != n_inst || p.n_distant != n_dist))
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n_instances / n_distant are not the scene's " + std::to_string(n_inst) + " instances and " + std::to_string(n_dist) +
                                               " distant lights");
  tables.assign(n_inst + n_dist, 0);
  if (own) {
    lights_default_groups(c, tables.data(), tables.data() + n_inst, p.background_group);
  } else {
    if (n_inst) std::memcpy(tables.data(), p.instance_group, n_inst);
    if (n_dist) std::memcpy(tables.data() + n_inst, p.distant_group, n_dist);
  }
  return RENE_OK;
}
// the call's tables to the device, ahead of the destination's checks (a call refused there has launched nothing; the next one uploads its own).  A
// pass in flight reads the ones this call overwrites: the stream is drained first, and again behind the copy (`tables` is pageable memory of the
// caller's scope)
static int lights_upload_tables(const std::string& me, rene_ctx* c, const std::vector<uint8_t>& tables) {
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(wait_stream(c->stream));
  if (int rc = c->lights_tables.reserve(std::max<size_t>(16, tables.size()), me + " tables"); rc != RENE_OK) return rc;
  if (!tables.empty()) HIP_TRY(hipMemcpyAsync(c->lights_tables.p, tables.data(), tables.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(wait_stream(c->stream));
  return RENE_OK;
}
// either call's launch: the pass's records, or (samples) the probe's
static hipError_t lights_launch(rene_ctx* c, const rene_lights_params& p, bool samples, const uint32_t* seeds, void* dst) {
  const uint32_t background = (c->cfg.features & rene::FEAT_BACKGROUND) ? 1u : 0u;
  const uint8_t* t = c->lights_tables.as<uint8_t>();
  return rene::launch_lights(c->cfg, c->view, rene::LightsLaunch{tile_grid(c), seeds, p.n_frames, background, t, t + c->inst_emits.size(), p.background_group, dst}, samples,
                             c->stream);
}

static int rene_lights_impl(rene_ctx* c, const rene_lights_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_lights";
  rene_lights_params p;
  std::vector<uint8_t> tables;
  if (int prc = lights_read_params(me, c, false, nullptr, params, p, tables); prc != RENE_OK) return prc;
  if (int rc = lights_upload_tables(me, c, tables); rc != RENE_OK) return rc;
  return run_pixel_pass(me, c, p.first_frame, p.n_frames, sizeof(rene_lights_pixel), &rene_ctx::lights, device_dst, dst_bytes,
                        [&](const uint32_t* seeds, void* dst) { return lights_launch(c, p, false, seeds, dst); }, [&](float ms) {
    std::fprintf(stderr, "[rene] lights %u x %u, frames %u + %u, ms: kernel %.4f\n", c->width, c->height, p.first_frame, p.n_frames, ms);
  });
}

static int rene_lights_samples_impl(rene_ctx* c, const rene_lights_params* params, rene_lights_sample* host_dst, size_t n) {
  const std::string me = "rene_lights_samples";
  rene_lights_params p;
  std::vector<uint8_t> tables;
  if (int prc = lights_read_params(me, c, true, host_dst, params, p, tables); prc != RENE_OK) return prc;
  if (int rc = lights_upload_tables(me, c, tables); rc != RENE_OK) return rc;
  return run_pixel_pass_samples(me, c, p.first_frame, p.n_frames, 1, sizeof(rene_lights_sample), 20, "records", "n_frames x width x height", host_dst, n,
                                [&](const uint32_t* seeds, void* dst) { return lights_launch(c, p, true, seeds, dst); });
}

// ---- multi-channel OpenEXR output (kernels_exr.hip; the file and its values are specified in include/rene_hip.h) -------------------------------------
namespace {
enum { EXR_UINT = 0, EXR_HALF = 1, EXR_FLOAT = 2 };
enum ExrPlane { EXR_P_BEAUTY, EXR_P_ALBEDO, EXR_P_NORMAL, EXR_P_DENOISED, EXR_P_ALPHA, EXR_P_DEPTH, EXR_P_POSITION, EXR_P_IDS, EXR_P_COVERAGE };
struct ExrChannel {
  const char* name;
  uint32_t layer, type;
  ExrPlane plane;
  uint32_t component, stride;  // of rene_exr_planes' plane
};
// every channel a file can hold, in the order of their names' bytes -- the order of the header's channel list and of a chunk's rows, and the order
// in which kernels_exr.hip emits them
const ExrChannel kExrChannels[] = {
    {"A", RENE_EXR_ALPHA, EXR_HALF, EXR_P_ALPHA, 0, 1},
    {"B", RENE_EXR_BEAUTY, EXR_HALF, EXR_P_BEAUTY, 2, 3},
    {"G", RENE_EXR_BEAUTY, EXR_HALF, EXR_P_BEAUTY, 1, 3},
    {"P.X", RENE_EXR_POSITION, EXR_FLOAT, EXR_P_POSITION, 0, 3},
    {"P.Y", RENE_EXR_POSITION, EXR_FLOAT, EXR_P_POSITION, 1, 3},
    {"P.Z", RENE_EXR_POSITION, EXR_FLOAT, EXR_P_POSITION, 2, 3},
    {"R", RENE_EXR_BEAUTY, EXR_HALF, EXR_P_BEAUTY, 0, 3},
    {"Z", RENE_EXR_DEPTH, EXR_FLOAT, EXR_P_DEPTH, 0, 1},
    {"albedo.B", RENE_EXR_ALBEDO, EXR_HALF, EXR_P_ALBEDO, 2, 3},
    {"albedo.G", RENE_EXR_ALBEDO, EXR_HALF, EXR_P_ALBEDO, 1, 3},
    {"albedo.R", RENE_EXR_ALBEDO, EXR_HALF, EXR_P_ALBEDO, 0, 3},
    {"cov0", RENE_EXR_IDS, EXR_HALF, EXR_P_COVERAGE, 0, 4},
    {"cov1", RENE_EXR_IDS, EXR_HALF, EXR_P_COVERAGE, 1, 4},
    {"cov2", RENE_EXR_IDS, EXR_HALF, EXR_P_COVERAGE, 2, 4},
    {"cov3", RENE_EXR_IDS, EXR_HALF, EXR_P_COVERAGE, 3, 4},
    {"denoised.B", RENE_EXR_DENOISED, EXR_HALF, EXR_P_DENOISED, 2, 3},
    {"denoised.G", RENE_EXR_DENOISED, EXR_HALF, EXR_P_DENOISED, 1, 3},
    {"denoised.R", RENE_EXR_DENOISED, EXR_HALF, EXR_P_DENOISED, 0, 3},
    {"id0", RENE_EXR_IDS, EXR_UINT, EXR_P_IDS, 0, 4},
    {"id1", RENE_EXR_IDS, EXR_UINT, EXR_P_IDS, 1, 4},
    {"id2", RENE_EXR_IDS, EXR_UINT, EXR_P_IDS, 2, 4},
    {"id3", RENE_EXR_IDS, EXR_UINT, EXR_P_IDS, 3, 4},
    {"normal.X", RENE_EXR_NORMAL, EXR_HALF, EXR_P_NORMAL, 0, 3},
    {"normal.Y", RENE_EXR_NORMAL, EXR_HALF, EXR_P_NORMAL, 1, 3},
    {"normal.Z", RENE_EXR_NORMAL, EXR_HALF, EXR_P_NORMAL, 2, 3},
};
constexpr uint32_t kExrGeometry = RENE_EXR_ALPHA | RENE_EXR_DEPTH | RENE_EXR_POSITION | RENE_EXR_IDS;

uint32_t exr_bytes_per_pixel(uint32_t layers) {
  uint32_t bpp = 0;
  for (const ExrChannel& ch : kExrChannels)
    if (layers & ch.layer) bpp += ch.type == EXR_HALF ? 2u : 4u;
  return bpp;
}
// the fp32 -> fp16 rule of half_element.h on the host: clamped to the finite halves, round to nearest even, subnormals kept, a NaN stays one
uint16_t exr_half_bits(float v) {
  v = v > 65504.0f ? 65504.0f : (v < -65504.0f ? -65504.0f : v);
  uint32_t x;
  std::memcpy(&x, &v, sizeof(x));
  const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x1ffu));  // NaN: quiet, the payload's top bits
  if (a >= 0x38800000u) {  // a normal half, 2^-14 and up (at most 65504 after the clamp: the carry of the rounding cannot reach infinity)
    const uint32_t h = a - 0x38000000u, rem = h & 0x1fffu;
    uint32_t r = h >> 13;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
  }
  if (a <= 0x33000000u) return (uint16_t)sign;  // up to 2^-25, the tie included: zero
  const uint32_t e = a >> 23, m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;  // a subnormal half: m x 2^(e - 150) in units of 2^-24; shift 14 .. 24
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  uint32_t r = m >> shift;
  if (rem > half || (rem == half && (r & 1u))) ++r;
  return (uint16_t)(sign | r);
}
int exr_check_film(const std::string& me, uint32_t width, uint32_t height, uint32_t layers) {
  if (layers == 0u || (layers & ~RENE_EXR_ALL)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": layers must be a non-empty mask of RENE_EXR_* bits");
  if (width < 1u || width > RENE_EXR_MAX_SIZE || height < 1u || height > RENE_EXR_MAX_SIZE)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": width and height must be 1 .. 16384");
  return RENE_OK;
}
void exr_put(std::vector<uint8_t>& v, const void* p, size_t n) { v.insert(v.end(), static_cast<const uint8_t*>(p), static_cast<const uint8_t*>(p) + n); }
void exr_attr(std::vector<uint8_t>& v, const char* name, const char* type, const void* value, uint32_t n) {
  exr_put(v, name, std::strlen(name) + 1);
  exr_put(v, type, std::strlen(type) + 1);
  exr_put(v, &n, 4);  // (little-endian hosts only, like every file this library writes)
  exr_put(v, value, n);
}
// one entry of a channel list
void exr_channel(std::vector<uint8_t>& chlist, const char* name, int32_t type) {
  exr_put(chlist, name, std::strlen(name) + 1);
  const int32_t rec[4] = {type, 0, 1, 1};  // pixel type, pLinear + 3 reserved bytes, x and y sampling
  exr_put(chlist, rec, 16);
}
// the magic, the version and the eight attributes of every file this library writes, without the header's terminating 0: `chlist` is the channel
// list without its own terminating 0
void exr_common_attributes(uint32_t width, uint32_t height, std::vector<uint8_t> chlist, uint8_t compression, std::vector<uint8_t>& v) {
  v.clear();
  const uint32_t magic[2] = {20000630u, 2u};
  exr_put(v, magic, 8);
  chlist.push_back(0);
  exr_attr(v, "channels", "chlist", chlist.data(), (uint32_t)chlist.size());
  const uint8_t zero = 0;
  exr_attr(v, "compression", "compression", &compression, 1);
  const int32_t box[4] = {0, 0, (int32_t)width - 1, (int32_t)height - 1};
  exr_attr(v, "dataWindow", "box2i", box, 16);
  exr_attr(v, "displayWindow", "box2i", box, 16);
  exr_attr(v, "lineOrder", "lineOrder", &zero, 1);
  const float one = 1.0f, centre[2] = {0.0f, 0.0f};
  exr_attr(v, "pixelAspectRatio", "float", &one, 4);
  exr_attr(v, "screenWindowCenter", "v2f", centre, 8);
  exr_attr(v, "screenWindowWidth", "float", &one, 4);
}
// the header and the offset table of a width x height file of `layers`; table == false: the attributes alone, with `compression` as the attribute's byte
void exr_header_bytes(uint32_t width, uint32_t height, uint32_t layers, std::vector<uint8_t>& v, uint8_t compression = 0, bool table = true) {
  std::vector<uint8_t> chlist;
  for (const ExrChannel& ch : kExrChannels)
    if (layers & ch.layer) exr_channel(chlist, ch.name, (int32_t)ch.type);
  exr_common_attributes(width, height, std::move(chlist), compression, v);
  v.push_back(0);
  if (!table) return;
  const uint64_t chunk = 8u + (uint64_t)width * exr_bytes_per_pixel(layers), first = v.size() + 8u * (uint64_t)height;
  for (uint32_t y = 0; y < height; ++y) {
    const uint64_t at = first + y * chunk;
    exr_put(v, &at, 8);
  }
}
}  // namespace

void rene_exr_params_default(rene_exr_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->layers = RENE_EXR_BEAUTY | RENE_EXR_ALBEDO | RENE_EXR_NORMAL;
  out->beauty_source = RENE_OUTPUT_RADIANCE;
}

static int rene_exr_layout_impl(uint32_t width, uint32_t height, uint32_t layers, size_t* header_bytes, size_t* body_bytes, uint32_t* bytes_per_pixel) {
  if (int rc = exr_check_film("rene_exr_layout", width, height, layers); rc != RENE_OK) return rc;
  const uint32_t bpp = exr_bytes_per_pixel(layers);
  std::vector<uint8_t> h;
  exr_header_bytes(width, height, layers, h);
  if (header_bytes) *header_bytes = h.size();
  if (body_bytes) *body_bytes = (size_t)height * (8u + (size_t)width * bpp);
  if (bytes_per_pixel) *bytes_per_pixel = bpp;
  return RENE_OK;
}

static int rene_exr_header_impl(uint32_t width, uint32_t height, uint32_t layers, void* dst, size_t dst_bytes) {
  const std::string me = "rene_exr_header";
  if (int rc = exr_check_film(me, width, height, layers); rc != RENE_OK) return rc;
  if (!dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL destination");
  std::vector<uint8_t> h;
  exr_header_bytes(width, height, layers, h);
  if (dst_bytes < h.size()) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than the header and its offset table (rene_exr_layout)");
  std::memcpy(dst, h.data(), h.size());
  return RENE_OK;
}

static int rene_exr_body_host_impl(uint32_t width, uint32_t height, uint32_t layers, const rene_exr_planes* planes, void* dst, size_t dst_bytes) {
  const std::string me = "rene_exr_body_host";
  if (int rc = exr_check_film(me, width, height, layers); rc != RENE_OK) return rc;
  if (!planes || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (planes->struct_size != sizeof(rene_exr_planes)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_exr_planes.struct_size mismatch (ABI skew)");
  const void* const plane[] = {planes->beauty, planes->albedo, planes->normal, planes->denoised, planes->alpha, planes->depth, planes->position, planes->ids, planes->coverage};
  for (const ExrChannel& ch : kExrChannels)
    if ((layers & ch.layer) && !plane[ch.plane]) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the plane of channel " + ch.name + " is NULL");
  const uint32_t row_data = width * exr_bytes_per_pixel(layers);
  if (dst_bytes < (size_t)height * (8u + (size_t)row_data)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than the body (rene_exr_layout)");
  uint8_t* at = static_cast<uint8_t*>(dst);
  for (uint32_t y = 0; y < height; ++y) {
    const uint32_t prefix[2] = {y, row_data};
    std::memcpy(at, prefix, 8);
    at += 8;
    for (const ExrChannel& ch : kExrChannels) {
      if (!(layers & ch.layer)) continue;
      const size_t first = (size_t)y * width * ch.stride + ch.component;
      if (ch.type == EXR_HALF) {
        const float* src = static_cast<const float*>(plane[ch.plane]) + first;
        for (uint32_t x = 0; x < width; ++x, at += 2) {
          const uint16_t h = exr_half_bits(src[(size_t)x * ch.stride]);
          std::memcpy(at, &h, 2);
        }
      } else {  // FLOAT and UINT: the plane's bits
        const uint32_t* src = static_cast<const uint32_t*>(plane[ch.plane]) + first;
        for (uint32_t x = 0; x < width; ++x, at += 4) std::memcpy(at, src + (size_t)x * ch.stride, 4);
      }
    }
  }
  return RENE_OK;
}

static const char kNoExr[] = "no rene_output_exr into the library's buffer since the context was created or reset";

static int rene_output_exr_impl(rene_ctx* c, const rene_exr_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_output_exr";
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  rene_exr_params p;
  if (int prc = read_params("rene_exr_params", rene_exr_params_default, params, p); prc != RENE_OK) return prc;
  if (p.beauty_source != RENE_OUTPUT_RADIANCE && p.beauty_source != RENE_OUTPUT_DENOISED_MEAN && p.beauty_source != RENE_OUTPUT_ROBUST)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": beauty_source must be RENE_OUTPUT_RADIANCE, RENE_OUTPUT_DENOISED_MEAN or RENE_OUTPUT_ROBUST");
  if (p.reserved != 0u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": reserved must be 0");
  if (int rc = exr_check_film(me, c->width, c->height, p.layers); rc != RENE_OK) return rc;
  const uint32_t bpp = exr_bytes_per_pixel(p.layers);
  const size_t n_px = (size_t)c->width * c->height, need = (size_t)c->height * (8u + (size_t)c->width * bpp);
  const bool beauty = (p.layers & RENE_EXR_BEAUTY) != 0u, geometry = (p.layers & kExrGeometry) != 0u;
  // the images the chosen layers read, as the sources of rene_output_8bit: a row of divisors each
  struct Source {
    bool used;
    uint32_t source;
    const float* rene::ExrLaunch::*layer;
    const uint32_t* rene::ExrLaunch::*frames;
  };
  const Source sources[] = {{beauty, p.beauty_source, &rene::ExrLaunch::beauty, &rene::ExrLaunch::beauty_frames},
                            {(p.layers & (RENE_EXR_ALBEDO | RENE_EXR_NORMAL)) != 0u, RENE_OUTPUT_ALBEDO, &rene::ExrLaunch::albedo, &rene::ExrLaunch::image_frames},
                            {(p.layers & RENE_EXR_DENOISED) != 0u, RENE_OUTPUT_DENOISED_MEAN, &rene::ExrLaunch::denoised, &rene::ExrLaunch::denoised_frames}};
  rene::TileGrid G{};
  int rc = begin_chain_pass(me.c_str(), c, false, G, [&] {
    for (const Source& s : sources)
      if (s.used)
        if (int r = check_output_source(me, c, s.source); r != RENE_OK) return r;
    if (geometry && (!c->gbuf.valid || c->gbuf.bytes != n_px * sizeof(rene_gbuffer_pixel)))
      return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the alpha, depth, position and id layers read the records of a rene_gbuffer with device_dst == NULL, and this context has none");
    return device_dst ? check_device_destination(me, c->device, device_dst, dst_bytes, need, "the body (rene_exr_layout)", 4, "4-byte aligned") : (int)RENE_OK;
  });  // (... and the drain: waits for the launches issued so far and resolves the image)
  if (rc != RENE_OK) return rc;
  const uint32_t nt = c->n_tiles;
  std::vector<uint32_t> frames(3u * (size_t)nt, 1u);
  rene::ExrLaunch L{};
  for (size_t k = 0; k < 3; ++k)
    if (sources[k].used)
      if (rc = output_source_layer(me, c, sources[k].source, L.*sources[k].layer, frames.data() + k * nt); rc != RENE_OK) return rc;
  const uint32_t* d_frames = nullptr;
  if (rc = upload_tile_divisors(me, c, frames, d_frames); rc != RENE_OK) return rc;
  for (size_t k = 0; k < 3; ++k) L.*sources[k].frames = d_frames + k * nt;
  L.normal = c->fb + n_px * 4;  // (layer 1 shares layer 2's divisors: both are the resolved image)
  L.records = geometry ? c->gbuf.buf.as<rene_gbuffer_pixel>() : nullptr;
  L.width = c->width, L.height = c->height, L.tiles_x = c->tiles_x, L.n_tiles = nt;
  L.shard_rank = G.shard_rank, L.shard_count = G.shard_count;
  L.shard_inv = G.shard_count > 1u ? (uint32_t)(0x100000000ull / G.shard_count) : 0u;
  L.layers = p.layers;
  L.bytes_per_pixel = bpp;
  void* dst = device_dst;
  if (!device_dst)
    if (rc = c->exr.begin(need, {p.layers}, c->stream, me + " buffer", dst); rc != RENE_OK) return rc;
  L.dst = dst;
  rc = timed_launch(me.c_str(), c, [&] { return rene::launch_exr(L, c->stream); }, [&](float ms) {
    std::fprintf(stderr, "[rene] exr body %u x %u, layers 0x%02x, beauty source %u, %u bytes per pixel, ms: kernel %.4f\n", c->width, c->height, p.layers, p.beauty_source, bpp, ms);
  });
  if (rc != RENE_OK) return rc;
  if (!device_dst) c->exr.commit(need);
  return RENE_OK;
}

// a file's bytes into `path`
static int exr_write_file(const std::string& me, const char* path, const std::vector<uint8_t>& file) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(RENE_ERR_IO, me + ": cannot open " + path + " for writing");
  const bool ok = std::fwrite(file.data(), 1, file.size(), f) == file.size();
  if (std::fclose(f) != 0 || !ok) return fail(RENE_ERR_IO, me + ": cannot write " + path);
  return RENE_OK;
}

static int rene_write_exr_impl(rene_ctx* c, const rene_exr_params* params, const char* path) {
  const std::string me = "rene_write_exr";
  if (!c || !path) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (int rc = rene_output_exr_impl(c, params, nullptr, 0); rc != RENE_OK) return rc;
  rene_exr_params p;
  read_params("rene_exr_params", rene_exr_params_default, params, p);  // (checked by the call above)
  std::vector<uint8_t> file;
  exr_header_bytes(c->width, c->height, p.layers, file);
  const size_t head = file.size();
  file.resize(head + c->exr.bytes);
  if (int rc = result_download(me.c_str(), c, &rene_ctx::exr, kNoExr, "destination too small", false, file.data() + head, c->exr.bytes); rc != RENE_OK) return rc;
  return exr_write_file(me, path, file);
}

// ---- compressed OpenEXR output: ZIPS chunks (kernels_exr_zips.hip, exr_deflate.h; the stream is specified in include/rene_hip.h) -----------------------
namespace {
int exr_check_compression(const std::string& me, uint32_t compression) {
  if (compression != RENE_EXR_COMPRESSION_NONE && compression != RENE_EXR_COMPRESSION_ZIPS)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": compression must be RENE_EXR_COMPRESSION_NONE or RENE_EXR_COMPRESSION_ZIPS");
  return RENE_OK;
}
// the sizes of a file's parts: the attributes, the uncompressed body, a row's data
struct ExrSizes {
  size_t attr_bytes, body_bytes, tail_bound;
  uint32_t row_bytes;
  const char* body_is;  // where the caller learns body_bytes, for the refusals
};
// ... of `height` rows of row_bytes behind attr_bytes of attributes
ExrSizes exr_row_sizes(uint32_t row_bytes, uint32_t height, size_t attr_bytes, const char* body_is = "height x (8 + row_bytes)") {
  const size_t body = (size_t)height * (8u + (size_t)row_bytes);
  return ExrSizes{attr_bytes, body, 8u * (size_t)height + body, row_bytes, body_is};
}
ExrSizes exr_sizes(uint32_t width, uint32_t height, uint32_t layers) {
  std::vector<uint8_t> a;
  exr_header_bytes(width, height, layers, a, 0, false);
  return exr_row_sizes(width * exr_bytes_per_pixel(layers), height, a.size(), "rene_exr_layout");
}
// the rows rene_exr_compress_rows takes: the kernels pair the bytes of a row (an even length), and a Cryptomatte row of three layers is the longest
constexpr uint32_t kExrMaxRowBytes = RENE_EXR_MAX_SIZE * 32u * RENE_CRYPTOMATTE_MAX_LAYERS;
int exr_check_rows(const std::string& me, uint32_t row_bytes, uint32_t height) {
  if (row_bytes < 2u || (row_bytes & 1u) || row_bytes > kExrMaxRowBytes) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": row_bytes must be even and 2 .. 16384 x 96");
  if (height < 1u || height > RENE_EXR_MAX_SIZE) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": height must be 1 .. 16384");
  return RENE_OK;
}
// an LSB-first bit writer into a vector of bytes
struct ZipsBits {
  std::vector<uint8_t>& z;
  uint64_t acc = 0;
  uint32_t cnt = 0;
  void put(uint32_t v, uint32_t n) {
    acc |= (uint64_t)v << cnt;
    for (cnt += n; cnt >= 8u; cnt -= 8u, acc >>= 8) z.push_back((uint8_t)acc);
  }
  void to_byte() {
    if (cnt) put(0u, 8u - cnt);
  }
};
// the zlib stream of one row: d is scratch for the pre-processed row
void zips_row_host(const uint8_t* raw, uint32_t n, std::vector<uint8_t>& d, std::vector<uint8_t>& z) {
  d.resize(n);
  uint8_t prev = 0;
  uint32_t s1 = 1u, s2 = 0u;
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t t = raw[rene::zips_raw_index(i, n)];
    d[i] = i ? (uint8_t)(t - prev + 128u) : t;
    prev = t;
    s1 = (s1 + d[i]) % rene::ZIPS_ADLER_MOD;
    s2 = (s2 + s1) % rene::ZIPS_ADLER_MOD;
  }
  z.clear();
  ZipsBits bits{z};
  bits.put(rene::ZIPS_HEAD, rene::ZIPS_HEAD_BITS);
  uint32_t nb = 0;
  for (uint32_t i = 0; i < n;) {
    if (i < 2u || d[i] != d[i - 2u]) {
      const uint32_t code = rene::zips_token(d[i], false, 0u, 0u, &nb);
      bits.put(code, nb);
      ++i;
      continue;
    }
    uint32_t end = i;  // the maximal interval of e == 1 is [i, end)
    while (end < n && d[end] == d[end - 2u]) ++end;
    for (uint32_t p = i; p < end; ++p) {
      const uint32_t code = rene::zips_token(d[p], true, (p - i) % rene::ZIPS_MAX_MATCH, end - p, &nb);
      if (nb) bits.put(code, nb);
    }
    i = end;
  }
  bits.put(0u, rene::ZIPS_EOB_BITS);
  bits.to_byte();
  for (int k = 3; k >= 0; --k) z.push_back((uint8_t)((((s2 << 16) | s1) >> (8 * k)) & 255u));
}
// the uncompressed file's table, as offsets behind attr_bytes of attributes
void exr_plain_table(const ExrSizes& S, uint32_t height, std::vector<uint64_t>& table) {
  table.resize(height);
  for (uint32_t y = 0; y < height; ++y) table[y] = S.attr_bytes + 8u * (uint64_t)height + (uint64_t)y * (8u + (uint64_t)S.row_bytes);
}
}  // namespace

static size_t rene_exr_tail_bound_impl(uint32_t width, uint32_t height, uint32_t layers) {
  if (layers == 0u || (layers & ~RENE_EXR_ALL) || width < 1u || width > RENE_EXR_MAX_SIZE || height < 1u || height > RENE_EXR_MAX_SIZE) return 0;
  return exr_sizes(width, height, layers).tail_bound;
}

static int rene_exr_attributes_impl(uint32_t width, uint32_t height, uint32_t layers, uint32_t compression, void* dst, size_t dst_bytes) {
  const std::string me = "rene_exr_attributes";
  if (int rc = exr_check_film(me, width, height, layers); rc != RENE_OK) return rc;
  if (int rc = exr_check_compression(me, compression); rc != RENE_OK) return rc;
  if (!dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL destination");
  std::vector<uint8_t> a;
  exr_header_bytes(width, height, layers, a, (uint8_t)compression, false);
  if (dst_bytes < a.size()) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than the attributes (rene_exr_layout's header_bytes - 8 x height)");
  std::memcpy(dst, a.data(), a.size());
  return RENE_OK;
}

// What rene_exr_compress_host and rene_exr_compress_rows_host share behind the checks of the film or the row: `S` says what the rows are
static int exr_compress_host_rows(const std::string& me, const ExrSizes& S, uint32_t height, uint32_t compression, const void* body, size_t body_bytes, void* dst,
                                  size_t dst_bytes, size_t* written) {
  if (int rc = exr_check_compression(me, compression); rc != RENE_OK) return rc;
  if (!body || !dst || !written) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (body_bytes != S.body_bytes) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": body_bytes is not the body's size (" + S.body_is + ")");
  if (dst_bytes < S.tail_bound) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than rene_exr_tail_bound");
  const uint8_t* src = static_cast<const uint8_t*>(body);
  uint8_t* out = static_cast<uint8_t*>(dst);
  if (compression == RENE_EXR_COMPRESSION_NONE) {
    std::vector<uint64_t> table;
    exr_plain_table(S, height, table);
    std::memcpy(out, table.data(), 8u * (size_t)height);
    std::memcpy(out + 8u * (size_t)height, src, S.body_bytes);
    *written = S.tail_bound;
    return RENE_OK;
  }
  std::vector<uint8_t> d, z;
  size_t at = 8u * (size_t)height;
  for (uint32_t y = 0; y < height; ++y) {
    const uint8_t* raw = src + (size_t)y * (8u + (size_t)S.row_bytes) + 8u;
    zips_row_host(raw, S.row_bytes, d, z);
    const bool stored = z.size() >= S.row_bytes;
    const uint64_t offset = S.attr_bytes + at;
    const uint32_t prefix[2] = {y, stored ? S.row_bytes : (uint32_t)z.size()};
    std::memcpy(out + 8u * (size_t)y, &offset, 8);
    std::memcpy(out + at, prefix, 8);
    std::memcpy(out + at + 8u, stored ? raw : z.data(), prefix[1]);
    at += 8u + prefix[1];
  }
  *written = at;
  return RENE_OK;
}

static int rene_exr_compress_host_impl(uint32_t width, uint32_t height, uint32_t layers, uint32_t compression, const void* body, size_t body_bytes, void* dst,
                                       size_t dst_bytes, size_t* written) {
  const std::string me = "rene_exr_compress_host";
  if (int rc = exr_check_film(me, width, height, layers); rc != RENE_OK) return rc;
  return exr_compress_host_rows(me, exr_sizes(width, height, layers), height, compression, body, body_bytes, dst, dst_bytes, written);
}

static int rene_exr_compress_rows_host_impl(uint32_t row_bytes, uint32_t height, size_t attributes_bytes, uint32_t compression, const void* body, size_t body_bytes,
                                            void* dst, size_t dst_bytes, size_t* written) {
  const std::string me = "rene_exr_compress_rows_host";
  if (int rc = exr_check_rows(me, row_bytes, height); rc != RENE_OK) return rc;
  return exr_compress_host_rows(me, exr_row_sizes(row_bytes, height, attributes_bytes), height, compression, body, body_bytes, dst, dst_bytes, written);
}

static const char kNoExrTail[] = "no rene_exr_compress into the library's buffer since the context was created or reset";

// What rene_exr_compress and rene_exr_compress_rows share behind the checks of the context and of the film or the row (`what`: the rows in the
// words of the RENE_DEBUG line)
static int exr_compress_rows(const std::string& me, rene_ctx* c, const ExrSizes& S, uint32_t height, const std::string& what, uint32_t compression,
                             const void* device_body, size_t body_bytes, void* device_dst, size_t dst_bytes, size_t* written) {
  if (int rc = exr_check_compression(me, compression); rc != RENE_OK) return rc;
  if (!device_body || !written) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (body_bytes != S.body_bytes) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": body_bytes is not the body's size (" + S.body_is + ")");
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = check_device_destination(me + " (the body)", c->device, device_body, body_bytes, S.body_bytes, ("the body (" + std::string(S.body_is) + ")").c_str(), 4, "4-byte aligned"); rc != RENE_OK)
    return rc;
  if (device_dst) {
    if (int rc = check_device_destination(me, c->device, device_dst, dst_bytes, S.tail_bound, "rene_exr_tail_bound", 8, "8-byte aligned"); rc != RENE_OK) return rc;
    const char *b0 = static_cast<const char*>(device_body), *d0 = static_cast<const char*>(device_dst);
    if (b0 < d0 + S.tail_bound && d0 < b0 + S.body_bytes) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the destination overlaps the body");
  }
  void* dst = device_dst;
  if (!device_dst) {  // (the library's buffer may be freed and allocated again here: the body must not lie in it)
    const char *b0 = static_cast<const char*>(device_body), *t0 = c->exr_tail.buf.as<char>();
    if (t0 && b0 < t0 + c->exr_tail.buf.cap && t0 < b0 + S.body_bytes) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the body lies in the library's tail buffer, which this call overwrites");
    if (int rc = c->exr_tail.begin(S.tail_bound, {}, c->stream, me + " buffer", dst); rc != RENE_OK) return rc;
  }
  unsigned long long n_written = S.tail_bound;
  if (compression == RENE_EXR_COMPRESSION_NONE) {  // the present table and the present body: two copies, no kernel
    std::vector<uint64_t> table;
    exr_plain_table(S, height, table);
    HIP_TRY(hipMemcpyAsync(dst, table.data(), 8u * (size_t)height, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + 8u * (size_t)height, device_body, S.body_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(wait_stream(c->stream));
  } else {
    if (int rc = c->zips_scratch.reserve(8u + 4u * (size_t)height, me + " scratch"); rc != RENE_OK) return rc;
    rene::ZipsLaunch L{};
    L.body = static_cast<const uint8_t*>(device_body);
    L.tail = static_cast<uint8_t*>(dst);
    L.written = c->zips_scratch.as<unsigned long long>();
    L.sizes = reinterpret_cast<uint32_t*>(c->zips_scratch.as<char>() + 8);
    L.attr_bytes = S.attr_bytes;
    L.height = height, L.row_bytes = S.row_bytes;
    Marks M(c->stream);
    M.mark();
    hipError_t e = rene::launch_exr_zips_size(L, c->stream);
    M.mark();
    if (e == hipSuccess) e = rene::launch_exr_zips_scan(L, c->stream);
    M.mark();
    if (e == hipSuccess) e = rene::launch_exr_zips_encode(L, c->stream);
    M.mark();
    if (e != hipSuccess) return launch_failed(me, c, e);
    HIP_TRY(hipMemcpyAsync(&n_written, L.written, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(wait_stream(c->stream));
    if (n_written < 16u * (unsigned long long)height || n_written > S.tail_bound) return fail(RENE_ERR_DEVICE, me + ": the kernels left a length outside the tail's bounds");
    if (M.complete)
      std::fprintf(stderr, "[rene] exr zips %s, %zu -> %llu bytes, ms: size %.4f scan %.4f encode %.4f\n", what.c_str(), S.tail_bound, n_written, M.ms(0, 1), M.ms(1, 2),
                   M.ms(2, 3));
  }
  if (!device_dst) c->exr_tail.commit((size_t)n_written);
  *written = (size_t)n_written;
  return RENE_OK;
}

static int rene_exr_compress_impl(rene_ctx* c, uint32_t width, uint32_t height, uint32_t layers, uint32_t compression, const void* device_body, size_t body_bytes,
                                  void* device_dst, size_t dst_bytes, size_t* written) {
  const std::string me = "rene_exr_compress";
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  if (int rc = exr_check_film(me, width, height, layers); rc != RENE_OK) return rc;
  char what[64];
  std::snprintf(what, sizeof what, "%u x %u, layers 0x%02x", width, height, layers);
  return exr_compress_rows(me, c, exr_sizes(width, height, layers), height, what, compression, device_body, body_bytes, device_dst, dst_bytes, written);
}

static int rene_exr_compress_rows_impl(rene_ctx* c, uint32_t row_bytes, uint32_t height, size_t attributes_bytes, uint32_t compression, const void* device_body,
                                       size_t body_bytes, void* device_dst, size_t dst_bytes, size_t* written) {
  const std::string me = "rene_exr_compress_rows";
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  if (int rc = exr_check_rows(me, row_bytes, height); rc != RENE_OK) return rc;
  char what[64];
  std::snprintf(what, sizeof what, "%u rows of %u bytes", height, row_bytes);
  return exr_compress_rows(me, c, exr_row_sizes(row_bytes, height, attributes_bytes), height, what, compression, device_body, body_bytes, device_dst, dst_bytes, written);
}

static int rene_output_exr_compressed_impl(rene_ctx* c, const rene_exr_params* params, uint32_t compression, void* device_dst, size_t dst_bytes, size_t* written) {
  const std::string me = "rene_output_exr_compressed";
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL context");
  if (!written) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (int rc = exr_check_compression(me, compression); rc != RENE_OK) return rc;
  rene_exr_params p;
  if (int prc = read_params("rene_exr_params", rene_exr_params_default, params, p); prc != RENE_OK) return prc;
  if (int rc = exr_check_film(me, c->width, c->height, p.layers); rc != RENE_OK) return rc;
  if (c->opts.shard_count > 1)
    return fail(RENE_ERR_UNSUPPORTED, me + ": a row spans tiles of several shards; let the shards fill one body with rene_output_exr and compress it with rene_exr_compress on one context");
  if (device_dst) {  // (checked again by rene_exr_compress; here so that a bad destination is refused before the body's kernel is launched)
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = check_device_destination(me, c->device, device_dst, dst_bytes, rene_exr_tail_bound_impl(c->width, c->height, p.layers), "rene_exr_tail_bound", 8, "8-byte aligned"); rc != RENE_OK)
      return rc;
  }
  if (int rc = rene_output_exr_impl(c, params, nullptr, 0); rc != RENE_OK) return rc;
  return rene_exr_compress_impl(c, c->width, c->height, p.layers, compression, c->exr.buf.p, c->exr.bytes, device_dst, dst_bytes, written);
}

static int rene_write_exr_compressed_impl(rene_ctx* c, const rene_exr_params* params, uint32_t compression, const char* path) {
  const std::string me = "rene_write_exr_compressed";
  if (!c || !path) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  size_t written = 0;
  if (int rc = rene_output_exr_compressed_impl(c, params, compression, nullptr, 0, &written); rc != RENE_OK) return rc;
  rene_exr_params p;
  read_params("rene_exr_params", rene_exr_params_default, params, p);  // (checked by the call above)
  std::vector<uint8_t> file;
  exr_header_bytes(c->width, c->height, p.layers, file, (uint8_t)compression, false);
  const size_t head = file.size();
  file.resize(head + written);
  if (int rc = result_download(me.c_str(), c, &rene_ctx::exr_tail, kNoExrTail, "destination too small", false, file.data() + head, written); rc != RENE_OK) return rc;
  return exr_write_file(me, path, file);
}

// ---- Cryptomatte output (kernels_cryptomatte.hip; the hash, the manifest, the file and its values are specified in include/rene_hip.h) --------------
namespace {
uint32_t murmur3_x86_32(const uint8_t* data, size_t n, uint32_t seed) {
  auto rotl = [](uint32_t v, int r) { return (v << r) | (v >> (32 - r)); };
  const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
  uint32_t h = seed;
  const size_t blocks = n / 4;
  for (size_t i = 0; i < blocks; ++i) {
    uint32_t k = (uint32_t)data[4 * i] | (uint32_t)data[4 * i + 1] << 8 | (uint32_t)data[4 * i + 2] << 16 | (uint32_t)data[4 * i + 3] << 24;
    k = rotl(k * c1, 15) * c2;
    h = rotl(h ^ k, 13) * 5u + 0xe6546b64u;
  }
  uint32_t k = 0;
  const uint8_t* tail = data + 4 * blocks;
  switch (n & 3u) {
    case 3: k ^= (uint32_t)tail[2] << 16; [[fallthrough]];
    case 2: k ^= (uint32_t)tail[1] << 8; [[fallthrough]];
    case 1: k ^= tail[0], h ^= rotl(k * c1, 15) * c2;
  }
  h ^= (uint32_t)n;
  h ^= h >> 16, h *= 0x85ebca6bu, h ^= h >> 13, h *= 0xc2b2ae35u, h ^= h >> 16;
  return h;
}
uint32_t cryptomatte_hash(const char* s, size_t n) {
  uint32_t h = murmur3_x86_32(reinterpret_cast<const uint8_t*>(s), n, 0u);
  const uint32_t e = (h >> 23) & 255u;
  if (e == 0u || e == 255u) h ^= 1u << 23;
  return h;
}
// the first `digits` of %08x of h, behind what `out` holds
void put_hex(std::string& out, uint32_t h, size_t digits = 8) {
  char b[12];
  std::snprintf(b, sizeof b, "%08x", h);
  out.append(b, digits);
}
void cryptomatte_manifest(const char* const* names, uint32_t n_names, std::string& m) {
  std::vector<std::string> sorted(names, names + n_names);
  std::sort(sorted.begin(), sorted.end());  // (char_traits<char> compares bytes as unsigned)
  sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
  m = "{";
  for (const std::string& name : sorted) {
    if (m.size() > 1) m += ',';
    m += '"';
    for (const char ch : name) {
      const uint8_t b = (uint8_t)ch;
      if (b == '"' || b == '\\') m += '\\', m += ch;
      else if (b < 0x20u) m += "\\u00", m += "0123456789abcdef"[b >> 4], m += "0123456789abcdef"[b & 15u];
      else m += ch;
    }
    m += "\":\"";
    put_hex(m, cryptomatte_hash(name.data(), name.size()));
    m += '"';
  }
  m += '}';
}

// What the layers of a call come to, once checked: the layers in the order of their names' bytes, their keys, and the chunk's channel rows
struct CryptomattePlan {
  uint32_t n_layers = 0;
  uint32_t by_name[RENE_CRYPTOMATTE_MAX_LAYERS] = {};     // the caller's index of the k-th layer in name order
  std::string key[RENE_CRYPTOMATTE_MAX_LAYERS];           // by the caller's index
  std::vector<std::string> channels;                      // the channel names in the order of their bytes
  uint8_t row_index[RENE_CRYPTOMATTE_MAX_LAYERS][8] = {}; // by the caller's index: where the level 00's A B G R and the level 01's lie in `channels`
  uint32_t bytes_per_pixel() const { return 32u * n_layers; }
};
int cryptomatte_plan(const std::string& me, uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers, CryptomattePlan& P) {
  if (width < 1u || width > RENE_EXR_MAX_SIZE || height < 1u || height > RENE_EXR_MAX_SIZE)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": width and height must be 1 .. 16384");
  if (n_layers < 1u || n_layers > RENE_CRYPTOMATTE_MAX_LAYERS) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": n_layers must be 1 .. 3");
  if (!layers) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL layers");
  P.n_layers = n_layers;
  for (uint32_t l = 0; l < n_layers; ++l) {
    const rene_cryptomatte_layer& Y = layers[l];
    const size_t len = Y.name ? std::strlen(Y.name) : 0;
    bool ok = len >= 1 && len <= RENE_CRYPTOMATTE_MAX_NAME;
    for (size_t i = 0; ok && i < len; ++i) ok = std::isalnum((unsigned char)Y.name[i]) || Y.name[i] == '_';
    if (!ok || std::isdigit((unsigned char)Y.name[len - 1]))
      return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a layer's name must be 1 .. 24 bytes of [A-Za-z0-9_] and must not end in a digit");
    if (Y.id_source != RENE_GBUFFER_ID_INSTANCE && Y.id_source != RENE_GBUFFER_ID_MATERIAL)
      return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a layer's id_source must be RENE_GBUFFER_ID_INSTANCE or RENE_GBUFFER_ID_MATERIAL (primitives have no names)");
    if (Y.n_names && !Y.names) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a NULL name list with n_names above 0");
    for (uint32_t i = 0; i < Y.n_names; ++i)
      if (!Y.names[i]) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a NULL name in a layer's list");
    put_hex(P.key[l], cryptomatte_hash(Y.name, len), 7);
    for (uint32_t k = 0; k < l; ++k) {
      if (!std::strcmp(Y.name, layers[k].name)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": two layers of one name");
      if (P.key[l] == P.key[k]) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": two layers whose names hash to one metadata key");
    }
    P.by_name[l] = l;
  }
  std::sort(P.by_name, P.by_name + n_layers, [&](uint32_t a, uint32_t b) { return std::string(layers[a].name) < std::string(layers[b].name); });
  std::vector<std::pair<std::string, uint32_t>> ch;  // (name, 8 l + its place among A B G R of 00, then of 01)
  for (uint32_t l = 0; l < n_layers; ++l)
    for (uint32_t c = 0; c < 8u; ++c) ch.emplace_back(std::string(layers[l].name) + (c < 4u ? "00." : "01.") + "ABGR"[c & 3u], 8u * l + c);
  std::sort(ch.begin(), ch.end());
  for (size_t i = 0; i < ch.size(); ++i) {
    P.channels.push_back(ch[i].first);
    P.row_index[ch[i].second / 8u][ch[i].second % 8u] = (uint8_t)i;
  }
  return RENE_OK;
}
// the file from the magic through the header's terminating 0
void cryptomatte_attribute_bytes(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, const CryptomattePlan& P, uint8_t compression,
                                 std::vector<uint8_t>& v) {
  std::vector<uint8_t> chlist;
  for (const std::string& name : P.channels) exr_channel(chlist, name.c_str(), EXR_FLOAT);
  exr_common_attributes(width, height, std::move(chlist), compression, v);
  for (uint32_t k = 0; k < P.n_layers; ++k) {
    const rene_cryptomatte_layer& Y = layers[P.by_name[k]];
    const std::string stem = "cryptomatte/" + P.key[P.by_name[k]] + "/";
    std::string manifest;
    cryptomatte_manifest(Y.names, Y.n_names, manifest);
    exr_attr(v, (stem + "conversion").c_str(), "string", "uint32_to_float32", 17);
    exr_attr(v, (stem + "hash").c_str(), "string", "MurmurHash3_32", 14);
    exr_attr(v, (stem + "manifest").c_str(), "string", manifest.data(), (uint32_t)manifest.size());
    exr_attr(v, (stem + "name").c_str(), "string", Y.name, (uint32_t)std::strlen(Y.name));
  }
  v.push_back(0);
}
// a layer's names as the table the pack looks ids up in, behind what `h` holds
void cryptomatte_hashes(const rene_cryptomatte_layer& Y, std::vector<uint32_t>& h) {
  for (uint32_t i = 0; i < Y.n_names; ++i) h.push_back(cryptomatte_hash(Y.names[i], std::strlen(Y.names[i])));
}
}  // namespace

void rene_cryptomatte_params_default(rene_cryptomatte_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
}

static int rene_cryptomatte_manifest_impl(const char* const* names, uint32_t n_names, char* dst, size_t dst_bytes, size_t* written) {
  const std::string me = "rene_cryptomatte_manifest";
  if (!written || (n_names && !names)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  for (uint32_t i = 0; i < n_names; ++i)
    if (!names[i]) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a NULL name in the list");
  std::string m;
  cryptomatte_manifest(names, n_names, m);
  *written = m.size();
  if (!dst) return RENE_OK;
  if (dst_bytes < m.size()) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than the manifest (*written)");
  std::memcpy(dst, m.data(), m.size());
  return RENE_OK;
}

static int rene_cryptomatte_layout_impl(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers, size_t* attributes_bytes,
                                        size_t* body_bytes, uint32_t* bytes_per_pixel) {
  CryptomattePlan P;
  if (int rc = cryptomatte_plan("rene_cryptomatte_layout", width, height, layers, n_layers, P); rc != RENE_OK) return rc;
  std::vector<uint8_t> a;
  cryptomatte_attribute_bytes(width, height, layers, P, 0, a);
  if (attributes_bytes) *attributes_bytes = a.size();
  if (body_bytes) *body_bytes = (size_t)height * (8u + (size_t)width * P.bytes_per_pixel());
  if (bytes_per_pixel) *bytes_per_pixel = P.bytes_per_pixel();
  return RENE_OK;
}

static int rene_cryptomatte_attributes_impl(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers, uint32_t compression, void* dst,
                                            size_t dst_bytes) {
  const std::string me = "rene_cryptomatte_attributes";
  CryptomattePlan P;
  if (int rc = cryptomatte_plan(me, width, height, layers, n_layers, P); rc != RENE_OK) return rc;
  if (int rc = exr_check_compression(me, compression); rc != RENE_OK) return rc;
  if (!dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL destination");
  std::vector<uint8_t> a;
  cryptomatte_attribute_bytes(width, height, layers, P, (uint8_t)compression, a);
  if (dst_bytes < a.size()) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than the attributes (rene_cryptomatte_layout)");
  std::memcpy(dst, a.data(), a.size());
  return RENE_OK;
}

static int rene_cryptomatte_body_host_impl(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers,
                                           const rene_gbuffer_pixel* const* host_records, void* dst, size_t dst_bytes) {
  const std::string me = "rene_cryptomatte_body_host";
  CryptomattePlan P;
  if (int rc = cryptomatte_plan(me, width, height, layers, n_layers, P); rc != RENE_OK) return rc;
  if (!host_records || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  for (uint32_t l = 0; l < n_layers; ++l)
    if (!host_records[l]) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a layer without records");
  const uint32_t row_data = width * P.bytes_per_pixel();
  if (dst_bytes < (size_t)height * (8u + (size_t)row_data)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than the body (rene_cryptomatte_layout)");
  struct Matte {
    uint32_t count, key;
  };
  for (uint32_t l = 0; l < n_layers; ++l) {
    std::vector<uint32_t> hashes;
    cryptomatte_hashes(layers[l], hashes);
    for (uint32_t y = 0; y < height; ++y) {
      uint8_t* const row = static_cast<uint8_t*>(dst) + (size_t)y * (8u + (size_t)row_data);
      if (l == 0u) {
        const uint32_t prefix[2] = {y, row_data};
        std::memcpy(row, prefix, 8);
      }
      for (uint32_t x = 0; x < width; ++x) {
        const rene_gbuffer_pixel& g = host_records[l][(size_t)y * width + x];
        Matte s[4];
        size_t used = 0;
        for (int k = 0; g.n != 0u && k < 4; ++k) {  // rules 1 to 3
          if (g.count[k] == 0u || g.id[k] >= layers[l].n_names) continue;
          const uint32_t key = hashes[g.id[k]];
          size_t j = 0;
          while (j < used && s[j].key != key) ++j;
          if (j < used) s[j].count += g.count[k];
          else s[used++] = Matte{g.count[k], key};
        }
        std::sort(s, s + used, [](const Matte& a, const Matte& b) { return a.count > b.count || (a.count == b.count && a.key < b.key); });  // rule 4
        uint32_t value[8] = {};  // A B G R of the level 00, then of 01 (rule 5)
        for (size_t r = 0; r < used; ++r) {
          const float coverage = (float)s[r].count / (float)g.n;
          const size_t level = 4u * (r / 2u);
          value[level + (r & 1u ? 1u : 3u)] = s[r].key;
          std::memcpy(&value[level + (r & 1u ? 0u : 2u)], &coverage, 4);
        }
        for (int c = 0; c < 8; ++c) std::memcpy(row + 8u + (size_t)P.row_index[l][c] * 4u * width + 4u * (size_t)x, &value[c], 4);
      }
    }
  }
  return RENE_OK;
}

static const char kNoCryptomatte[] = "no rene_output_cryptomatte into the library's buffer since the context was created or reset";

static int rene_output_cryptomatte_impl(rene_ctx* c, const rene_cryptomatte_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_output_cryptomatte";
  if (!c || !params) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (params->struct_size != sizeof(rene_cryptomatte_params)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_cryptomatte_params.struct_size mismatch (ABI skew)");
  if (params->reserved != 0u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": reserved must be 0");
  CryptomattePlan P;
  if (int rc = cryptomatte_plan(me, c->width, c->height, params->layers, params->n_layers, P); rc != RENE_OK) return rc;
  const size_t n_px = (size_t)c->width * c->height, need = (size_t)c->height * (8u + (size_t)c->width * P.bytes_per_pixel());
  HIP_TRY(hipSetDevice(c->device));
  rene::CryptomatteLaunch L{};
  std::vector<uint32_t> hashes;  // the layers' tables one behind the other
  size_t first[RENE_CRYPTOMATTE_MAX_LAYERS] = {};
  for (uint32_t l = 0; l < P.n_layers; ++l) {
    const rene_cryptomatte_layer& Y = params->layers[l];
    const bool instances = Y.id_source == RENE_GBUFFER_ID_INSTANCE;
    const size_t have = instances ? c->inst_emits.size() : (size_t)c->n_materials;
    if (Y.n_names != have)
      return fail(RENE_ERR_INVALID_ARGUMENT, me + ": layer " + Y.name + " has n_names " + std::to_string(Y.n_names) + ", the scene " + std::to_string(have) +
                                                 (instances ? " instances" : " materials"));
    if (Y.records) {
      if (int rc = check_device_destination(me + " (the records of layer " + Y.name + ")", c->device, Y.records, n_px * sizeof(rene_gbuffer_pixel),
                                            n_px * sizeof(rene_gbuffer_pixel), "the records (rene_gbuffer_bytes)", 16, "16-byte aligned");
          rc != RENE_OK)
        return rc;
      L.records[l] = static_cast<const rene_gbuffer_pixel*>(Y.records);
    } else {
      if (!c->gbuf.valid || c->gbuf.bytes != n_px * sizeof(rene_gbuffer_pixel))
        return fail(RENE_ERR_INVALID_ARGUMENT, me + ": layer " + Y.name + " reads the records of a rene_gbuffer with device_dst == NULL, and this context has none");
      if (c->gbuf_id_source != Y.id_source)
        return fail(RENE_ERR_INVALID_ARGUMENT, me + ": layer " + Y.name + " has id_source " + std::to_string(Y.id_source) + ", the context's last rene_gbuffer with device_dst == NULL ran with " +
                                                   std::to_string(c->gbuf_id_source));
      L.records[l] = c->gbuf.buf.as<rene_gbuffer_pixel>();
    }
    first[l] = hashes.size();
    cryptomatte_hashes(Y, hashes);
    L.n_names[l] = Y.n_names;
    std::memcpy(L.row_index[l], P.row_index[l], 8);
  }
  if (device_dst)
    if (int rc = check_device_destination(me, c->device, device_dst, dst_bytes, need, "the body (rene_cryptomatte_layout)", 4, "4-byte aligned"); rc != RENE_OK) return rc;
  HIP_TRY(wait_stream(c->stream));  // (the launches issued so far; a pack in flight reads the table this call overwrites)
  if (int rc = c->cryptomatte_hashes.reserve(std::max<size_t>(16, hashes.size() * sizeof(uint32_t)), me + " name hashes"); rc != RENE_OK) return rc;
  if (!hashes.empty()) HIP_TRY(hipMemcpyAsync(c->cryptomatte_hashes.p, hashes.data(), hashes.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(wait_stream(c->stream));  // (`hashes` is pageable memory of this scope)
  for (uint32_t l = 0; l < P.n_layers; ++l) L.hashes[l] = c->cryptomatte_hashes.as<uint32_t>() + first[l];
  const rene::TileGrid G = tile_grid(c);
  L.width = c->width, L.height = c->height, L.tiles_x = c->tiles_x;
  L.shard_rank = G.shard_rank, L.shard_count = G.shard_count;
  L.shard_inv = G.shard_count > 1u ? (uint32_t)(0x100000000ull / G.shard_count) : 0u;
  L.n_layers = P.n_layers;
  void* dst = device_dst;
  if (!device_dst) {  // (a shard leaves the bytes of the other shards' tiles alone: they read zero, as in rene_output_exr's buffer)
    uint32_t rows = 0;
    for (uint32_t l = 0; l < P.n_layers; ++l)
      for (int ch = 0; ch < 8; ++ch) rows = rows * 31u + P.row_index[l][ch];
    if (int rc = c->cryptomatte.begin(need, {P.n_layers, rows, 1u}, c->stream, me + " buffer", dst); rc != RENE_OK) return rc;
  }
  L.dst = dst;
  const int rc = timed_launch(me.c_str(), c, [&] { return rene::launch_cryptomatte(L, c->stream); }, [&](float ms) {
    std::fprintf(stderr, "[rene] cryptomatte body %u x %u, %u layers, %u bytes per pixel, ms: kernel %.4f\n", c->width, c->height, P.n_layers, P.bytes_per_pixel(), ms);
  });
  if (rc != RENE_OK) return rc;
  if (!device_dst) c->cryptomatte.commit(need);
  return RENE_OK;
}

// a file's bytes into path + ".tmp", which then takes the place of `path` (the checkpoint's way: a reader never sees half a file)
static int cryptomatte_write_file(const std::string& me, const char* path, const std::vector<uint8_t>& file) {
  const std::string tmp = std::string(path) + ".tmp";
  if (int rc = exr_write_file(me, tmp.c_str(), file); rc != RENE_OK) {
    std::remove(tmp.c_str());
    return rc;
  }
  if (std::rename(tmp.c_str(), path) != 0) {
    std::remove(tmp.c_str());
    return fail(RENE_ERR_IO, me + ": cannot rename " + tmp + " to " + path);
  }
  return RENE_OK;
}

static int rene_write_cryptomatte_impl(rene_ctx* c, const rene_cryptomatte_params* params, uint32_t compression, const char* path) {
  const std::string me = "rene_write_cryptomatte";
  if (!c || !params || !path) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (int rc = exr_check_compression(me, compression); rc != RENE_OK) return rc;
  if (c->opts.shard_count > 1)
    return fail(RENE_ERR_UNSUPPORTED, me + ": a row spans tiles of several shards; let the shards fill one body with rene_output_cryptomatte and compress it with rene_exr_compress_rows on one context");
  if (int rc = rene_output_cryptomatte_impl(c, params, nullptr, 0); rc != RENE_OK) return rc;
  CryptomattePlan P;
  if (int rc = cryptomatte_plan(me, c->width, c->height, params->layers, params->n_layers, P); rc != RENE_OK) return rc;  // (checked by the call above)
  std::vector<uint8_t> file;
  cryptomatte_attribute_bytes(c->width, c->height, params->layers, P, (uint8_t)compression, file);
  const size_t head = file.size();
  size_t written = 0;
  if (int rc = rene_exr_compress_rows_impl(c, c->width * P.bytes_per_pixel(), c->height, head, compression, c->cryptomatte.buf.p, c->cryptomatte.bytes, nullptr, 0, &written);
      rc != RENE_OK)
    return rc;
  file.resize(head + written);
  if (int rc = result_download(me.c_str(), c, &rene_ctx::exr_tail, kNoExrTail, "destination too small", false, file.data() + head, written); rc != RENE_OK) return rc;
  return cryptomatte_write_file(me, path, file);
}

// ---- OpenEXR pass layers (kernels_exr_passes.hip; the file and its values are specified in include/rene_hip.h) -------------------------------------
namespace {
// What a call's masks and names come to, once checked
struct ExrPassesPlan {
  uint32_t layers = 0, groups = 0;  // groups: the groups written, 0 without RENE_EXRP_LIGHTS
  uint32_t bpp = 0;
  std::string light_groups;         // the value of rene/lightGroups; empty: no attribute
  std::vector<std::string> channels;  // in file order, which is the order of the names' bytes
};
int exr_passes_plan(const std::string& me, uint32_t width, uint32_t height, const rene_exr_passes_params* p, ExrPassesPlan& P) {
  if (!p) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL params");
  if (p->struct_size != sizeof(rene_exr_passes_params)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_exr_passes_params.struct_size mismatch (ABI skew)");
  if (p->layers == 0u || (p->layers & ~RENE_EXRP_ALL)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": layers must be a non-empty mask of RENE_EXRP_* bits");
  if (p->groups > 255u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": groups must be a mask of 8 bits");
  if (p->groups && !(p->layers & RENE_EXRP_LIGHTS)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": groups must be 0 without RENE_EXRP_LIGHTS");
  if (p->reserved != 0u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": reserved must be 0");
  if (width < 1u || width > RENE_EXR_MAX_SIZE || height < 1u || height > RENE_EXR_MAX_SIZE)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": width and height must be 1 .. 16384");
  P.layers = p->layers;
  P.groups = (p->layers & RENE_EXRP_LIGHTS) ? (p->groups ? p->groups : 255u) : 0u;
  for (uint32_t g = 0; p->group_names && g < RENE_LIGHTS_GROUPS; ++g) {  // (every name is checked, a group's that is not written too)
    const char* name = p->group_names[g];
    if (!name) continue;
    const size_t len = std::strlen(name);
    bool ok = len >= 1 && len <= RENE_EXRP_MAX_NAME;
    for (size_t i = 0; ok && i < len; ++i) ok = std::isalnum((unsigned char)name[i]) || name[i] == '_' || name[i] == ' ' || name[i] == '-';
    if (!ok) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a light group's name must be 1 .. 24 bytes of [A-Za-z0-9_ -]");
    if (!(P.groups >> g & 1u)) continue;
    P.light_groups += P.light_groups.empty() ? "{" : ",";
    P.light_groups += "\"light" + std::to_string(g) + "\":\"" + name + "\"";  // (nothing in such a name needs the manifest's escapes)
  }
  if (!P.light_groups.empty()) P.light_groups += "}";
  auto rgb = [&](const std::string& stem) {
    for (const char* c : {".B", ".G", ".R"}) P.channels.push_back(stem + c);
  };
  if (P.layers & RENE_EXRP_AO) P.channels.push_back("ao");
  if (P.layers & RENE_EXRP_BENT)
    for (const char* c : {"bent.X", "bent.Y", "bent.Z"}) P.channels.push_back(c);
  if (P.layers & RENE_EXRP_BOUNCES)
    for (uint32_t d = 0; d < RENE_BOUNCES_BUCKETS; ++d) rgb("depth" + std::to_string(d));
  if (P.layers & RENE_EXRP_DIRECT) rgb("direct");
  if (P.layers & RENE_EXRP_INDIRECT) rgb("indirect");
  for (uint32_t g = 0; g < RENE_LIGHTS_GROUPS; ++g)
    if (P.groups >> g & 1u) rgb("light" + std::to_string(g));
  if (P.layers & RENE_EXRP_LENGTH) P.channels.push_back("pathlength");
  P.bpp = 2u * (uint32_t)P.channels.size();
  return RENE_OK;
}
// the file from the magic through the header's terminating 0
void exr_passes_attribute_bytes(uint32_t width, uint32_t height, const ExrPassesPlan& P, uint8_t compression, std::vector<uint8_t>& v) {
  std::vector<uint8_t> chlist;
  for (const std::string& name : P.channels) exr_channel(chlist, name.c_str(), EXR_HALF);
  exr_common_attributes(width, height, std::move(chlist), compression, v);
  if (!P.light_groups.empty()) exr_attr(v, "rene/lightGroups", "string", P.light_groups.data(), (uint32_t)P.light_groups.size());
  v.push_back(0);
}
// a value as the file's HALF: rene_output_exr's rule, and every NaN the one pattern
uint16_t exr_passes_half(float v) { return v != v ? (uint16_t)0x7e00u : exr_half_bits(v); }
}  // namespace

void rene_exr_passes_params_default(rene_exr_passes_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->layers = RENE_EXRP_ALL;
}

static int rene_exr_passes_layout_impl(uint32_t width, uint32_t height, const rene_exr_passes_params* params, size_t* attributes_bytes, size_t* body_bytes,
                                       uint32_t* bytes_per_pixel) {
  ExrPassesPlan P;
  if (int rc = exr_passes_plan("rene_exr_passes_layout", width, height, params, P); rc != RENE_OK) return rc;
  std::vector<uint8_t> a;
  exr_passes_attribute_bytes(width, height, P, 0, a);
  if (attributes_bytes) *attributes_bytes = a.size();
  if (body_bytes) *body_bytes = (size_t)height * (8u + (size_t)width * P.bpp);
  if (bytes_per_pixel) *bytes_per_pixel = P.bpp;
  return RENE_OK;
}

static int rene_exr_passes_attributes_impl(uint32_t width, uint32_t height, const rene_exr_passes_params* params, uint32_t compression, void* dst, size_t dst_bytes) {
  const std::string me = "rene_exr_passes_attributes";
  ExrPassesPlan P;
  if (int rc = exr_passes_plan(me, width, height, params, P); rc != RENE_OK) return rc;
  if (int rc = exr_check_compression(me, compression); rc != RENE_OK) return rc;
  if (!dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL destination");
  std::vector<uint8_t> a;
  exr_passes_attribute_bytes(width, height, P, (uint8_t)compression, a);
  if (dst_bytes < a.size()) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than the attributes (rene_exr_passes_layout)");
  std::memcpy(dst, a.data(), a.size());
  return RENE_OK;
}

static int rene_exr_passes_body_host_impl(uint32_t width, uint32_t height, const rene_exr_passes_params* params, const float* beauty_sum, void* dst, size_t dst_bytes) {
  const std::string me = "rene_exr_passes_body_host";
  ExrPassesPlan P;
  if (int rc = exr_passes_plan(me, width, height, params, P); rc != RENE_OK) return rc;
  const uint32_t F = P.layers;
  const auto* occlusion = static_cast<const rene_occlusion_pixel*>(params->occlusion);
  const auto* direct = static_cast<const rene_direct_pixel*>(params->direct);
  const auto* bounces = static_cast<const rene_bounces_pixel*>(params->bounces);
  const auto* lights = static_cast<const rene_lights_pixel*>(params->lights);
  if (!dst) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL destination");
  if (((F & (RENE_EXRP_AO | RENE_EXRP_BENT)) && !occlusion) || ((F & (RENE_EXRP_DIRECT | RENE_EXRP_INDIRECT)) && !direct) ||
      ((F & (RENE_EXRP_BOUNCES | RENE_EXRP_LENGTH)) && !bounces) || ((F & RENE_EXRP_LIGHTS) && !lights))
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a chosen layer's records are NULL");
  if ((F & RENE_EXRP_INDIRECT) && !beauty_sum) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": RENE_EXRP_INDIRECT without beauty_sum");
  const uint32_t row_data = width * P.bpp;
  if (dst_bytes < (size_t)height * (8u + (size_t)row_data)) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": dst_bytes is smaller than the body (rene_exr_passes_layout)");
  for (uint32_t y = 0; y < height; ++y) {
    uint8_t* const row = static_cast<uint8_t*>(dst) + (size_t)y * (8u + (size_t)row_data);
    const uint32_t prefix[2] = {y, row_data};
    std::memcpy(row, prefix, 8);
    for (uint32_t x = 0; x < width; ++x) {
      const size_t p = (size_t)y * width + x;
      uint8_t* at = row + 8u + 2u * (size_t)x;  // this pixel's place in the next channel row
      auto channel = [&](float v) {
        const uint16_t h = exr_passes_half(v);
        std::memcpy(at, &h, 2);
        at += 2u * (size_t)width;
      };
      auto mean3 = [&](const float* sum, uint32_t n) {  // B G R
        const float n_f = (float)n;
        for (int k = 2; k >= 0; --k) channel(n ? sum[k] / n_f : 0.0f);
      };
      if (F & RENE_EXRP_AO) channel(occlusion[p].rays ? 1.0f - (float)occlusion[p].occluded / (float)occlusion[p].rays : 1.0f);
      if (F & RENE_EXRP_BENT) {
        const float* b = occlusion[p].bent_sum;
        const float xx = b[0] * b[0], yy = b[1] * b[1], zz = b[2] * b[2];
        const float l = std::sqrt((xx + yy) + zz);
        for (int k = 0; k < 3; ++k) channel(l > 0.0f ? b[k] / l : 0.0f);
      }
      if (F & RENE_EXRP_BOUNCES)
        for (uint32_t d = 0; d < RENE_BOUNCES_BUCKETS; ++d) mean3(bounces[p].bucket[d].sum, bounces[p].n);
      if (F & (RENE_EXRP_DIRECT | RENE_EXRP_INDIRECT)) {
        const rene_direct_pixel& r = direct[p];
        float sum[3], rest[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < 3; ++k) {
          const float two = r.seen[k] + r.distant[k];
          sum[k] = two + r.sampled[k];
          if (F & RENE_EXRP_INDIRECT) rest[k] = beauty_sum[3u * p + (size_t)k] - sum[k];
        }
        if (F & RENE_EXRP_DIRECT) mean3(sum, r.n);
        if (F & RENE_EXRP_INDIRECT) mean3(rest, r.n);
      }
      for (uint32_t g = 0; g < RENE_LIGHTS_GROUPS; ++g)
        if (P.groups >> g & 1u) mean3(lights[p].group[g].sum, lights[p].n);
      if (F & RENE_EXRP_LENGTH) channel(bounces[p].n ? (float)bounces[p].length_sum / (float)bounces[p].n : 0.0f);
    }
  }
  return RENE_OK;
}

static const char kNoExrPasses[] = "no rene_output_exr_passes into the library's buffer since the context was created or reset";

static int rene_output_exr_passes_impl(rene_ctx* c, const rene_exr_passes_params* params, void* device_dst, size_t dst_bytes) {
  const std::string me = "rene_output_exr_passes";
  if (!c || !params) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  ExrPassesPlan P;
  if (int rc = exr_passes_plan(me, c->width, c->height, params, P); rc != RENE_OK) return rc;
  const uint32_t F = P.layers;
  const size_t n_px = (size_t)c->width * c->height, need = (size_t)c->height * (8u + (size_t)c->width * P.bpp);
  rene::ExrPassesLaunch L{};
  // the records a chosen layer reads: the caller's, or the library-owned result of the pass
  struct Source {
    uint32_t layers;
    const char* pass;
    const void* given;
    Result rene_ctx::*result;
    size_t record_bytes;
    const void** into;
  };
  const Source sources[] = {
      {RENE_EXRP_AO | RENE_EXRP_BENT, "rene_occlusion", params->occlusion, &rene_ctx::occl, sizeof(rene_occlusion_pixel), reinterpret_cast<const void**>(&L.occlusion)},
      {RENE_EXRP_DIRECT | RENE_EXRP_INDIRECT, "rene_direct", params->direct, &rene_ctx::direct, sizeof(rene_direct_pixel), reinterpret_cast<const void**>(&L.direct)},
      {RENE_EXRP_BOUNCES | RENE_EXRP_LENGTH, "rene_bounces", params->bounces, &rene_ctx::bounces, sizeof(rene_bounces_pixel), reinterpret_cast<const void**>(&L.bounces)},
      {RENE_EXRP_LIGHTS, "rene_lights", params->lights, &rene_ctx::lights, sizeof(rene_lights_pixel), reinterpret_cast<const void**>(&L.lights)}};
  auto checks = [&]() -> int {  // everything that can refuse, before anything waits or launches
    for (const Source& s : sources) {
      if (!(F & s.layers)) continue;  // (a source whose layers are not chosen is not read)
      const size_t bytes = n_px * s.record_bytes;
      if (s.given) {
        if (int rc = check_device_destination(me + " (the records of " + s.pass + ")", c->device, s.given, bytes, bytes, kImageBytes, 16, "16-byte aligned"); rc != RENE_OK)
          return rc;
        *s.into = s.given;
      } else {
        const Result& r = c->*s.result;
        if (!r.valid || r.bytes != bytes)
          return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a chosen layer reads the records of a " + s.pass + " with device_dst == NULL, and this context has none");
        *s.into = r.buf.p;
      }
    }
    if ((F & RENE_EXRP_INDIRECT) && !params->direct) {  // the radiance sums and the library-owned direct records: sums over the same frames?
      if (c->frame_base != c->direct_first_frame)
        return fail(RENE_ERR_INVALID_ARGUMENT, me + ": RENE_EXRP_INDIRECT: the context's frames start at " + std::to_string(c->frame_base) + ", the direct-light pass's at " +
                                                   std::to_string(c->direct_first_frame));
      for (uint32_t k = 0; k < c->n_owned(); ++k)
        if (c->tile_n(k) != c->direct_n_frames)
          return fail(RENE_ERR_INVALID_ARGUMENT, me + ": RENE_EXRP_INDIRECT: tile " + std::to_string(c->owned_tile(k)) + " holds " + std::to_string(c->tile_n(k)) +
                                                     " frames, the direct-light pass ran over " + std::to_string(c->direct_n_frames) +
                                                     "; beauty - direct needs sums over the same samples");
    }
    return device_dst ? check_device_destination(me, c->device, device_dst, dst_bytes, need, "the body (rene_exr_passes_layout)", 4, "4-byte aligned") : (int)RENE_OK;
  };
  rene::TileGrid G{};
  if (F & RENE_EXRP_INDIRECT) {  // rene_output_exr's refusals for RENE_OUTPUT_RADIANCE, and its drain: the launches issued so far, the image resolved
    if (int rc = begin_chain_pass(me.c_str(), c, false, G, checks); rc != RENE_OK) return rc;
    L.beauty = c->fb;
  } else {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = checks(); rc != RENE_OK) return rc;
    HIP_TRY(wait_stream(c->stream));  // (the launches issued so far)
    G = tile_grid(c);
  }
  L.width = c->width, L.height = c->height, L.tiles_x = c->tiles_x;
  L.shard_rank = G.shard_rank, L.shard_count = G.shard_count;
  L.shard_inv = G.shard_count > 1u ? (uint32_t)(0x100000000ull / G.shard_count) : 0u;
  L.layers = F, L.groups = P.groups, L.bytes_per_pixel = P.bpp;
  void* dst = device_dst;
  if (!device_dst)  // (a shard leaves the bytes of the other shards' tiles alone: they read zero, as in rene_output_exr's buffer)
    if (int rc = c->exr_passes.begin(need, {F, P.groups, 1u}, c->stream, me + " buffer", dst); rc != RENE_OK) return rc;
  L.dst = dst;
  const int rc = timed_launch(me.c_str(), c, [&] { return rene::launch_exr_passes(L, c->stream); }, [&](float ms) {
    std::fprintf(stderr, "[rene] exr passes body %u x %u, layers 0x%02x, groups 0x%02x, %u bytes per pixel, ms: kernel %.4f\n", c->width, c->height, F, P.groups, P.bpp, ms);
  });
  if (rc != RENE_OK) return rc;
  if (!device_dst) c->exr_passes.commit(need);
  return RENE_OK;
}

static int rene_write_exr_passes_impl(rene_ctx* c, const rene_exr_passes_params* params, uint32_t compression, const char* path) {
  const std::string me = "rene_write_exr_passes";
  if (!c || !params || !path) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL argument");
  if (int rc = exr_check_compression(me, compression); rc != RENE_OK) return rc;
  if (c->opts.shard_count > 1)
    return fail(RENE_ERR_UNSUPPORTED, me + ": a row spans tiles of several shards; let the shards fill one body with rene_output_exr_passes and compress it with rene_exr_compress_rows on one context");
  if (int rc = rene_output_exr_passes_impl(c, params, nullptr, 0); rc != RENE_OK) return rc;
  ExrPassesPlan P;
  if (int rc = exr_passes_plan(me, c->width, c->height, params, P); rc != RENE_OK) return rc;  // (checked by the call above)
  std::vector<uint8_t> file;
  exr_passes_attribute_bytes(c->width, c->height, P, (uint8_t)compression, file);
  const size_t head = file.size();
  size_t written = 0;
  if (int rc = rene_exr_compress_rows_impl(c, c->width * P.bpp, c->height, head, compression, c->exr_passes.buf.p, c->exr_passes.bytes, nullptr, 0, &written); rc != RENE_OK)
    return rc;
  file.resize(head + written);
  if (int rc = result_download(me.c_str(), c, &rene_ctx::exr_tail, kNoExrTail, "destination too small", false, file.data() + head, written); rc != RENE_OK) return rc;
  return cryptomatte_write_file(me, path, file);
}

// ---- adaptive sampling (include/rene_hip.h) -------------------------------------------------------------------------------------------------------
static int rene_set_active_tiles_impl(rene_ctx* c, const uint8_t* active, size_t n) {
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_set_active_tiles: NULL context");
  if (c->loaded) return fail(RENE_ERR_UNSUPPORTED, "rene_set_active_tiles: the frame chains were put there by rene_load_chains, which nothing renders onto; rene_reset first");
  if (c->opts.flags & RENE_FLAG_WAVEFRONT)
    return fail(RENE_ERR_UNSUPPORTED, "rene_set_active_tiles: a RENE_FLAG_WAVEFRONT context (the stage-separated wavefront integrator renders every slot of a launch)");
  if (c->opts.shard_mode == RENE_SHARD_FRAMES && c->opts.shard_count > 1)
    return fail(RENE_ERR_UNSUPPORTED, "rene_set_active_tiles: a frame shard (RENE_SHARD_FRAMES, shard_count > 1) holds a share of every pixel's frames; use an unsharded context or tile shards");
  if (!active) {
    if (c->n_inactive) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_set_active_tiles: a tile that has been switched off cannot be set active again (the set only shrinks until rene_reset)");
    return RENE_OK;
  }
  if (n < c->n_tiles) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_set_active_tiles: fewer entries than the tiles_y x tiles_x grid has tiles");
  const uint32_t n_owned = c->n_owned();
  std::vector<uint32_t> off;  // owned tiles this call switches off
  for (uint32_t k = 0; k < n_owned; ++k) {
    const bool was = !c->n_inactive || c->tile_active[k], want = active[c->owned_tile(k)] != 0;
    if (want && !was) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_set_active_tiles: a tile that has been switched off cannot be set active again (the set only shrinks until rene_reset)");
    if (was && !want) off.push_back(k);
  }
  if (off.empty()) return RENE_OK;
  if (!c->frames_contiguous || c->frames > 0xffffffffull)
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_set_active_tiles: the frames rendered so far are not one range (a rene_render did not continue where the one before it ended): "
                                           "a tile's frame count would not say which frames it holds; rene_reset and render consecutive frames");
  HIP_TRY(hipSetDevice(c->device));
  int rc = c->drain();  // launches in flight, and their replays, keep the set they were launched with
  if (rc != RENE_OK) return rc;
  const size_t words = (n_owned + 31u) / 32u;
  rc = c->mask_dev.reserve(words * sizeof(uint32_t), "rene_set_active_tiles mask");
  if (rc != RENE_OK) return rc;
  std::vector<uint8_t> now = c->tile_active.empty() ? std::vector<uint8_t>(n_owned, 1) : c->tile_active;
  for (uint32_t k : off) now[k] = 0;
  std::vector<uint32_t> bits(words, 0u);
  for (uint32_t k = 0; k < n_owned; ++k)
    if (now[k]) bits[k >> 5] |= 1u << (k & 31u);
  HIP_TRY(hipMemcpy(c->mask_dev.p, bits.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (c->tile_stop.empty()) c->tile_stop.assign(n_owned, 0u);
  for (uint32_t k : off) {
    c->tile_stop[k] = (uint32_t)c->frames;
    c->inactive_pixels += c->tile_pixels(c->owned_tile(k));
  }
  c->tile_active = std::move(now);
  c->n_inactive += (uint32_t)off.size();
  return RENE_OK;
}

static int rene_tile_frames_impl(rene_ctx* c, uint32_t* dst, size_t n) {
  if (!c || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_tile_frames: NULL argument");
  if (n < c->n_tiles) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_tile_frames: destination too small for the tiles_y x tiles_x grid");
  std::fill(dst, dst + c->n_tiles, 0u);
  for (uint32_t k = 0; k < c->n_owned(); ++k) dst[c->owned_tile(k)] = c->tile_n(k);
  return RENE_OK;
}

static int rene_download_mean_impl(rene_ctx* c, int layer, int channels, float* dst, size_t dst_floats) {
  if (!c || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_mean: NULL argument");
  if (layer < 0 || layer >= RENE_LAYER_COUNT) return fail(RENE_ERR_INVALID_ARGUMENT, "layer out of range");
  if (channels != 3 && channels != 4) return fail(RENE_ERR_INVALID_ARGUMENT, "channels must be 3 or 4");
  const size_t n = (size_t)c->width * c->height;
  if (dst_floats < n * (size_t)channels) return fail(RENE_ERR_INVALID_ARGUMENT, "destination too small");
  HIP_TRY(hipSetDevice(c->device));
  int rc = c->drain();  // the resolved image
  if (rc != RENE_OK) return rc;
  rc = c->mean_dev.reserve(std::max<size_t>(16, n * 4 * sizeof(float)), "rene_download_mean buffer");
  if (rc == RENE_OK) rc = c->tile_frames_dev.reserve(std::max<size_t>(16, (size_t)c->n_tiles * sizeof(uint32_t)), "rene_download_mean buffer");
  if (rc != RENE_OK) return rc;
  std::vector<uint32_t> frames(c->n_tiles, 0u);
  for (uint32_t k = 0; k < c->n_owned(); ++k) frames[c->owned_tile(k)] = c->tile_n(k);
  HIP_TRY(hipMemcpy(c->tile_frames_dev.p, frames.data(), frames.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  rc = timed_launch("rene_download_mean", c, [&] { return rene::launch_tile_mean(c->fb + (size_t)layer * n * 4, c->mean_dev.as<float>(), c->tile_frames_dev.as<uint32_t>(), c->width, c->height, c->tiles_x, c->stream); },
                    [&](float ms) { std::fprintf(stderr, "[rene] download_mean %u x %u, layer %d, ms: kernel %.4f\n", c->width, c->height, layer, ms); });
  if (rc != RENE_OK) return rc;
  return staged_download(c, c->mean_dev.as<float>(), 4, channels, dst);
}

static int rene_noise_select_tiles_impl(const rene_noise_tile* tiles, const uint8_t* active_in, uint32_t tiles_x, uint32_t tiles_y, float luminance_floor, double target,
                                        uint32_t dilate, uint8_t* active_out) {
  if (!tiles || !active_out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_noise_select_tiles: NULL argument");
  if (tiles_x == 0 || tiles_y == 0) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_noise_select_tiles: empty tile grid");
  if (dilate > 2) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_noise_select_tiles: dilate must be 0, 1 or 2");
  if (!std::isfinite(luminance_floor) || !(luminance_floor > 0.0f)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_noise_select_tiles: luminance_floor must be finite and positive");
  if (!std::isfinite(target) || !(target > 0.0)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_noise_select_tiles: target must be finite and positive");
  const size_t n = (size_t)tiles_x * tiles_y;
  std::vector<uint8_t> noisy(n, 0), alive(n, 0);
  for (size_t t = 0; t < n; ++t) {
    alive[t] = (!active_in || active_in[t]) && tiles[t].n_pixels != 0;
    if (!alive[t]) continue;
    const double nt = (double)tiles[t].n_pixels, m = (double)tiles[t].sum_lum / nt + (double)luminance_floor;  // q_t as rene_estimate_noise takes it
    const double q = ((double)tiles[t].sum_var / nt) / (m * m);
    noisy[t] = std::sqrt(q) > target;
  }
  const int d = (int)dilate;
  for (uint32_t y = 0; y < tiles_y; ++y)
    for (uint32_t x = 0; x < tiles_x; ++x) {
      const size_t t = (size_t)y * tiles_x + x;
      bool keep = false;
      for (int dy = -d; dy <= d && alive[t] && !keep; ++dy)
        for (int dx = -d; dx <= d && !keep; ++dx) {
          const int64_t yy = (int64_t)y + dy, xx = (int64_t)x + dx;
          if (yy < 0 || xx < 0 || yy >= (int64_t)tiles_y || xx >= (int64_t)tiles_x) continue;
          keep = noisy[(size_t)yy * tiles_x + (size_t)xx] != 0;
        }
      active_out[t] = keep ? 1 : 0;
    }
  return RENE_OK;
}

int rene_noise_combine(const rene_noise_estimate* parts, size_t n, rene_noise_estimate* out) {
  if (!parts || !out || n == 0) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_noise_combine: NULL argument or no parts");
  rene_noise_estimate e{};
  e.struct_size = sizeof(e);
  bool have_worst = false;
  for (size_t i = 0; i < n; ++i) {
    const rene_noise_estimate& p = parts[i];
    if (p.struct_size != sizeof(rene_noise_estimate)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_noise_estimate.struct_size mismatch (ABI skew)");
    if (i == 0) {
      e.n_frames = p.n_frames;
      e.n_chains = p.n_chains;
      e.luminance_floor = p.luminance_floor;
    } else if (p.n_frames != e.n_frames || !(p.luminance_floor == e.luminance_floor)) {
      return fail(RENE_ERR_INVALID_ARGUMENT, "rene_noise_combine: the parts differ in n_frames or luminance_floor: they are not shards of one job and one estimate");
    }
    e.n_tiles += p.n_tiles;
    e.n_pixels += p.n_pixels;
    e.sum_var += p.sum_var;
    e.sum_lum += p.sum_lum;
    e.sum_weighted_q += p.sum_weighted_q;
    if (p.n_tiles && (!have_worst || p.worst_tile_noise > e.worst_tile_noise || (p.worst_tile_noise == e.worst_tile_noise && p.worst_tile < e.worst_tile))) {
      e.worst_tile_noise = p.worst_tile_noise;
      e.worst_tile = p.worst_tile;
      have_worst = true;
    }
  }
  noise_derive(&e);
  *out = e;
  return RENE_OK;
}

uint32_t rene_noise_frames_needed(const rene_noise_estimate* est, double target) {
  if (!est) return 0xffffffffu;
  const uint32_t have = est->n_frames > 0xffffffffull ? 0xffffffffu : (uint32_t)est->n_frames;
  if (!(target > 0.0) || !std::isfinite(est->noise)) return 0xffffffffu;  // (also a NaN target)
  const double r = est->noise / target, need = std::ceil((double)est->n_frames * r * r);
  if (!(need < 4294967295.0)) return 0xffffffffu;
  return std::max(have, (uint32_t)need);
}

int rene_denoised_buffer(rene_ctx* c, void** device_ptr, size_t* n_floats) {
  if (!c || !device_ptr) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_denoised_buffer: NULL argument");
  if (!c->dn_valid) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_denoised_buffer: no rene_denoise since the context was created or reset");
  *device_ptr = c->dn_out.p;
  if (n_floats) *n_floats = (size_t)c->width * c->height * 4;
  return RENE_OK;
}

static int rene_download_denoised_impl(rene_ctx* c, int what, int channels, float* dst, size_t dst_floats) {
  if (!c || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_denoised: NULL argument");
  if (what != RENE_DENOISED_RADIANCE && what != RENE_DENOISED_VARIANCE && what != RENE_DENOISED_MEAN && what != RENE_DENOISED_TRIM)
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_denoised: `what` must be RENE_DENOISED_RADIANCE, RENE_DENOISED_VARIANCE, RENE_DENOISED_MEAN or RENE_DENOISED_TRIM");
  const bool plane = what == RENE_DENOISED_VARIANCE || what == RENE_DENOISED_TRIM;
  if (plane ? channels != 1 : (channels != 3 && channels != 4))
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_denoised: channels must be 3 or 4 for the radiance and the mean, 1 for the variance plane and the trim counts");
  const size_t n = (size_t)c->width * c->height;
  if (dst_floats < n * (size_t)channels) return fail(RENE_ERR_INVALID_ARGUMENT, "destination too small");
  if (!c->dn_valid) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download_denoised: no rene_denoise since the context was created or reset");
  HIP_TRY(hipSetDevice(c->device));
  if (what == RENE_DENOISED_TRIM) {  // (float)j of the last call's trim words; a call that trims nothing: zeros
    if (!c->dn_robust) {
      std::fill(dst, dst + n, 0.0f);
      return RENE_OK;
    }
    std::vector<uint32_t> words(n);
    HIP_TRY(hipMemcpy(words.data(), c->dn_trim.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) dst[i] = (float)(words[i] & 0xffu);
    return RENE_OK;
  }
  const float* src = plane ? c->dn_var.as<float>() : c->dn_out.as<float>();
  if (what == RENE_DENOISED_MEAN) {  // col * den of the call's filtered records, into the ping-pong buffer the call left free
    float* mean = c->dn_rec[c->dn_cur ^ 1u].as<float>();
    const hipError_t e = rene::launch_denoise_mean(c->dn_rec[c->dn_cur].as<float>(), c->dn_guides.as<float>(), mean, c->width, c->height, c->dn_albedo_floor, c->dn_masked, c->stream);
    if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("rene_download_denoised launch: ") + hipGetErrorString(e));
    HIP_TRY(wait_stream(c->stream));
    src = mean;
  }
  std::function<void(float*)> fix;
  if (what == RENE_DENOISED_MEAN && c->dn_masked)
    // the invalid tiles hold their unfiltered SUMS: divided here by the tile's N_t, the IEEE division of rene_download_mean (the denoiser's units
    // are built with the approximate one); N_t == 0: 0
    fix = [c](float* tmp) {
      for (uint32_t t = 0; t < c->dn_invalid_frames.size(); ++t) {
        const uint32_t nt = c->dn_invalid_frames[t];
        if (nt == rene_ctx::DN_TILE_VALID) continue;
        const uint32_t x0 = (t % c->tiles_x) * RENE_TILE_SIZE, y0 = (t / c->tiles_x) * RENE_TILE_SIZE;
        const float d = (float)nt;
        for (uint32_t y = y0; y < std::min<uint32_t>(y0 + RENE_TILE_SIZE, c->height); ++y)
          for (uint32_t x = x0; x < std::min<uint32_t>(x0 + RENE_TILE_SIZE, c->width); ++x) {
            float* v = tmp + ((size_t)y * c->width + x) * 4;
            for (int ch = 0; ch < 3; ++ch) v[ch] = nt ? v[ch] / d : 0.0f;
          }
      }
    };
  return staged_download(c, src, plane ? 1 : 4, channels, dst, false, 0, fix);
}

static int rene_download_impl(rene_ctx* c, int layer, int channels, float* dst, size_t dst_floats) {
  if (!c || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_download: NULL argument");
  if (layer < 0 || layer >= RENE_LAYER_COUNT) return fail(RENE_ERR_INVALID_ARGUMENT, "layer out of range");
  if (channels != 3 && channels != 4) return fail(RENE_ERR_INVALID_ARGUMENT, "channels must be 3 or 4");
  size_t n = (size_t)c->width * c->height;
  if (dst_floats < n * (size_t)channels) return fail(RENE_ERR_INVALID_ARGUMENT, "destination too small");
  HIP_TRY(hipSetDevice(c->device));
  int rc = c->drain();
  if (rc != RENE_OK) return rc;
  // (the device keeps a record's version in the fourth lane; rene's alpha stays 0, lib.rs:170)
  return staged_download(c, c->fb + (size_t)layer * n * 4, 4, channels, dst, true);
}

int rene_get_stats(rene_ctx* c, rene_stats* out) {
  if (!c || !out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_get_stats: NULL argument");
  HIP_TRY(hipSetDevice(c->device));
  int rc = c->drain();
  if (rc != RENE_OK) return rc;
  unsigned long long h[32];
  HIP_TRY(hipMemcpy(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost));
  if (std::getenv("RENE_DEBUG") && h[23] && h[19])  // the same kernels where path starts are prepared ahead (RENE_START_SLOT), how often and how densely
    std::fprintf(stderr, "[rene] passes with a path-start refill %llu (%.4f of the passes), lanes per refill %.3f of 64 (%.4f)\n", h[19], (double)h[19] / (double)h[12],
                 (double)h[20] / (double)h[19], (double)h[20] / (64.0 * (double)h[19]));
  if (std::getenv("RENE_DEBUG") && h[23])  // RENE_FLAG_COUNTERS on the megakernels of device_code.inc: where the lanes of a pass were
    std::fprintf(stderr, "[rene] passes %llu (wave executions of the loop); lanes per pass: on a path %.3f, waiting for a hand-off %.3f, out of work %.3f, starting a path %.3f; "
                         "passes with an item switch %.4f, with a poll %.4f\n", h[12], (double)h[13] / (64.0 * (double)h[12]), (double)h[14] / (64.0 * (double)h[12]),
                 (double)h[15] / (64.0 * (double)h[12]), (double)h[16] / (64.0 * (double)h[12]), (double)h[17] / (double)h[12], (double)h[18] / (double)h[12]);
  else if (std::getenv("RENE_DEBUG") && h[12])  // RENE_FLAG_COUNTERS on the traversal-restart kernel: lanes active per step kind
    std::fprintf(stderr, "[rene] steps (wave executions, lanes, lanes / 64 per execution): node %llu %llu %.3f | leaf %llu %llu %.3f | logic %llu %llu %.3f | iterations %llu\n",
                 h[12], h[6], (double)h[6] / (64.0 * (double)h[12]), h[13], h[16], (double)h[16] / (64.0 * (double)std::max(1ull, h[13])), h[14], h[15],
                 (double)h[15] / (64.0 * (double)std::max(1ull, h[14])), h[17]);
  if (std::getenv("RENE_DEBUG") && h[12] && !h[23] && h[17])  // ... and by the node step's position in its iteration: a wave's density decays from step to step
    std::fprintf(stderr, "[rene] lanes at an inner node per iteration, at its first / second / third node step: %.3f %.3f %.3f of 64\n",
                 (double)h[28] / (64.0 * (double)h[17]), (double)h[29] / (64.0 * (double)h[17]), (double)h[30] / (64.0 * (double)h[17]));
  if (std::getenv("RENE_DEBUG") && h[12] && !h[23])
    std::fprintf(stderr, "[rene] node visits %llu: nothing hit %llu (%.3f), reached by a pop %llu (%.3f), both %llu (%.3f); in the top levels %llu (%.3f); deepest stack %llu entries\n", h[6], h[18],
                 (double)h[18] / (double)h[6], h[19], (double)h[19] / (double)h[6], h[20], (double)h[20] / (double)h[6], h[22], (double)h[22] / (double)h[6], h[21]);
  std::memset(out, 0, sizeof(*out));
  out->rays_closest = h[0];
  out->rays_shadow = h[1];
  out->rays_emitter = h[2];
  out->paths = c->paths;  // frames rendered x pixels owned
  out->hits = h[4];
  out->bounces = h[4];
  out->adds = h[5];
  out->node_visits = h[6];
  out->prim_tests = h[7];
  out->frames = c->frames;
  out->launches = c->launches + c->replays;  // launches that had to be launched again (drain) count twice
  out->kernel_ms = c->kernel_ms;
  out->last_launch_ms = c->last_ms;
  // the engine clock while the launches ran: shader-clock ticks (s_memtime) per tick of the constant 100 MHz clock
  // (s_memrealtime) over the lifetime of one wave of each launch (device_code.inc, clock_probe)
  out->sclk_mhz = h[25] ? 100.0 * (double)h[24] / (double)h[25] : 0.0;
  return RENE_OK;
}

int rene_trace(rene_ctx* c, int which, size_t n, const float* origins, const float* directions, float tmin,
               float tmax, rene_hit* out) {
  if (!c || (n && (!origins || !directions || !out))) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_trace: NULL argument");
  if (which != 0 && which != 1) return fail(RENE_ERR_INVALID_ARGUMENT, "which must be 0 (main) or 1 (emitters)");
  // the traversal orders children by the bit pattern of their (non-negative) entry distance
  if (!(tmin >= 0.0f) || !(tmax >= tmin)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_trace: need 0 <= tmin <= tmax");
  if (n == 0) return RENE_OK;
  if (n > 0x7fffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, "too many rays in one batch");
  HIP_TRY(hipSetDevice(c->device));
  return run_probe("rene_trace", c->stream, {{origins, n * 12}, {directions, n * 12}}, {{out, n * sizeof(rene_hit)}}, [&](void* const* d) {
    return rene::launch_trace(c->cfg, c->view, which, (uint32_t)n, (const float*)d[0], (const float*)d[1], tmin, tmax, (rene_hit*)d[2], c->stream);
  });
}

// ---- the J1 gate (probes; DESIGN.md section 9, tools/j1_gate.py) ---------------------------------------------------------------------------------
int rene_ray_dump(rene_ctx* c, uint32_t first_frame, uint32_t n_frames, size_t capacity, float* rays8, uint64_t* n_issued) {
  if (!c || !rays8 || !n_issued || capacity == 0 || capacity > 0x7fffffffull / 8) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_ray_dump: bad argument");
  if (!(c->opts.flags & RENE_FLAG_COUNTERS) || c->wavefront || (c->cfg.features & rene::FEAT_VOLPATH) ||
      rene::select_kernel(c->cfg, c->view, c->opts.flags).family != rene::KernelFamily::Restart)
    return fail(RENE_ERR_UNSUPPORTED, "rene_ray_dump: a context with RENE_FLAG_COUNTERS whose scene the traversal-restart kernel renders (path integrator, more than 512 BVH nodes)");
  HIP_TRY(hipSetDevice(c->device));
  int rc = c->drain();
  if (rc != RENE_OK) return rc;
  DevArray<float> d;
  if (rc = d.reserve((capacity + 1) * 8 * sizeof(float), "rene_ray_dump"); rc != RENE_OK) return rc;
  hipError_t e = c->zero_now(d, 8 * sizeof(float));
  if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("rene_ray_dump: ") + hipGetErrorString(e));
  c->ray_dump = d;
  c->ray_dump_cap = (uint32_t)capacity;
  rc = rene_render(c, first_frame, n_frames);
  if (rc == RENE_OK) rc = c->drain();
  c->ray_dump = nullptr;
  c->ray_dump_cap = 0;
  uint32_t issued = 0;
  if (rc == RENE_OK) {
    e = hipMemcpy(&issued, d, sizeof(issued), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rays8, d + 8, std::min<size_t>(issued, capacity) * 8 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(RENE_ERR_DEVICE, std::string("rene_ray_dump: ") + hipGetErrorString(e));
  }
  *n_issued = issued;
  return rc;
}

int rene_trace_queue(rene_ctx* c, size_t n, const float* o_tmax4, const void* d_flags, int fp16, uint32_t refill_min, uint32_t leaf_min, uint32_t blocks_per_cu,
                     uint32_t repeats, float* hits4, float* ms_out, uint64_t* steps5) {
  if (!c || !n || !o_tmax4 || !d_flags || n > 0x7fffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_trace_queue: bad argument");
  if (c->cfg.features & rene::FEAT_SMALL) return fail(RENE_ERR_UNSUPPORTED, "rene_trace_queue: BVH scenes only");
  HIP_TRY(hipSetDevice(c->device));
  int rc = c->drain();
  if (rc != RENE_OK) return rc;
  DevArray<float> d_o, d_h;
  DevArray<uint32_t> d_d, d_cnt;
  DevArray<unsigned long long> d_steps;
  Event ev0, ev1;
  const size_t dbytes = n * (fp16 ? 8 : 16);
  hipError_t e = d_o.grow(n * 16);
  if (e == hipSuccess) e = d_d.grow(dbytes);
  if (e == hipSuccess) e = d_h.grow(n * 16);
  if (e == hipSuccess) e = d_cnt.grow(64 * sizeof(uint32_t));
  if (e == hipSuccess) e = d_steps.grow(8 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemcpy(d_o, o_tmax4, n * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_d, d_flags, dbytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = ev0.create();
  if (e == hipSuccess) e = ev1.create();
  float best_ms = 0.0f;
  for (uint32_t k = 0; e == hipSuccess && k < std::max(1u, repeats); ++k) {
    e = c->zero_now(d_cnt, 64 * sizeof(uint32_t));
    if (e == hipSuccess) e = c->zero_now(d_steps, 8 * sizeof(unsigned long long));
    rene::TraceQueue Q{};
    Q.o_tmax = d_o; Q.d_flags = d_d; Q.hits = d_h; Q.counter = d_cnt; Q.n = (uint32_t)n;
    Q.refill_min = std::max(1u, std::min(64u, refill_min)); Q.leaf_min = std::max(1u, leaf_min); Q.fp16 = fp16 ? 1u : 0u;
    Q.stack_entries = c->cfg.stack_depth;
    Q.passes = 1;
    if (const char* ev = std::getenv("RENE_GATE_PASSES")) Q.passes = (uint32_t)std::max(1, std::min((int)(0x7fffffffull / n), std::atoi(ev)));  // (probe knob: a longer launch)
    if (e == hipSuccess) e = hipEventRecord(ev0, c->stream);
    if (e == hipSuccess) e = rene::launch_trace_queue(c->cfg, c->view, Q, blocks_per_cu, steps5 ? d_steps : nullptr, c->stream);
    if (e == hipSuccess) e = hipEventRecord(ev1, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    if (k == 0 || ms < best_ms) best_ms = ms;
  }
  if (e == hipSuccess && hits4) e = hipMemcpy(hits4, d_h, n * 16, hipMemcpyDeviceToHost);
  if (e == hipSuccess && steps5) e = hipMemcpy(steps5, d_steps, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("rene_trace_queue: ") + hipGetErrorString(e));
  if (ms_out) *ms_out = best_ms;
  return RENE_OK;
}

int rene_bsdf_eval(rene_ctx* c, uint32_t material_index, size_t n, const float* normals3, const float* uvs2,
                   const float* wo3, const float* wi3, const uint32_t* seeds, float* out12) {
  if (!c || (n && (!normals3 || !uvs2 || !wo3 || !wi3 || !seeds || !out12)))
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_bsdf_eval: NULL argument");
  if (material_index >= c->n_materials) return fail(RENE_ERR_INVALID_ARGUMENT, "material_index out of range");
  if (n == 0) return RENE_OK;
  if (n > (1u << 24)) return fail(RENE_ERR_INVALID_ARGUMENT, "too many items in one batch");
  HIP_TRY(hipSetDevice(c->device));
  // the first instance that uses the material lends its record, so that the probe runs what a render runs (the material
  // resolved at upload, Inst::res_*); a material no instance uses goes through the material / texture tables
  int inst_index = -1;
  for (size_t k = 0; k < c->inst_material.size() && inst_index < 0; ++k)
    if (c->inst_material[k] == material_index) inst_index = (int)k;
  return run_probe("rene_bsdf_eval", c->stream, {{normals3, n * 12}, {uvs2, n * 8}, {wo3, n * 12}, {wi3, n * 12}, {seeds, n * 4}}, {{out12, n * 48}}, [&](void* const* d) {
    return rene::launch_bsdf_eval(c->view, material_index, inst_index, (uint32_t)n, (const float*)d[0], (const float*)d[1],
                                  (const float*)d[2], (const float*)d[3], (const uint32_t*)d[4], (float*)d[5], c->stream);
  });
}

int rene_medium_eval(rene_ctx* c, uint32_t medium_index, size_t n, const float* rd3, const float* t_max,
                     const float* wo3, const float* wi3, const uint32_t* seeds, float* out16) {
  if (!c || (n && (!rd3 || !t_max || !wo3 || !wi3 || !seeds || !out16)))
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_medium_eval: NULL argument");
  if (medium_index >= c->n_mediums) return fail(RENE_ERR_INVALID_ARGUMENT, "medium_index out of range (media exist only under the volpath integrator)");
  if (n == 0) return RENE_OK;
  if (n > (1u << 24)) return fail(RENE_ERR_INVALID_ARGUMENT, "too many items in one batch");
  HIP_TRY(hipSetDevice(c->device));
  return run_probe("rene_medium_eval", c->stream, {{rd3, n * 12}, {t_max, n * 4}, {wo3, n * 12}, {wi3, n * 12}, {seeds, n * 4}}, {{out16, n * 64}}, [&](void* const* d) {
    return rene::launch_medium_eval(c->view, medium_index, (uint32_t)n, (const float*)d[0], (const float*)d[1],
                                    (const float*)d[2], (const float*)d[3], (const uint32_t*)d[4], (float*)d[5], c->stream);
  });
}

int rene_transmittance(rene_ctx* c, int emit, uint32_t medium_index, size_t n, const float* origins, const float* directions, float* out4) {
  if (!c || (n && (!origins || !directions || !out4))) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_transmittance: NULL argument");
  if (medium_index >= c->n_mediums) return fail(RENE_ERR_INVALID_ARGUMENT, "medium_index out of range (media exist only under the volpath integrator)");
  if (n == 0) return RENE_OK;
  if (n > (1u << 24)) return fail(RENE_ERR_INVALID_ARGUMENT, "too many rays in one batch");
  HIP_TRY(hipSetDevice(c->device));
  return run_probe("rene_transmittance", c->stream, {{origins, n * 12}, {directions, n * 12}}, {{out4, n * 16}}, [&](void* const* d) {
    return rene::launch_transmittance(c->cfg, c->view, emit != 0, medium_index, (uint32_t)n, (const float*)d[0], (const float*)d[1], (float*)d[2], c->stream);
  });
}

int rene_emitter_pdf(rene_ctx* c, size_t n, const float* origins, const float* directions, float* out) {
  if (!c || (n && (!origins || !directions || !out))) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_emitter_pdf: NULL argument");
  if (n == 0) return RENE_OK;
  if (n > 0x7fffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, "too many rays in one batch");
  HIP_TRY(hipSetDevice(c->device));
  return run_probe("rene_emitter_pdf", c->stream, {{origins, n * 12}, {directions, n * 12}}, {{out, n * 4}}, [&](void* const* d) {
    return rene::launch_emitter_pdf(c->cfg, c->view, (uint32_t)n, (const float*)d[0], (const float*)d[1], (float*)d[2], c->stream);
  });
}

int rene_emitter_pdf_form(rene_ctx* c, int form, size_t n, const float* origins, const float* directions, float* out) {
  if (form == 0) return rene_emitter_pdf(c, n, origins, directions, out);
  if (!c || (n && (!origins || !directions || !out))) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_emitter_pdf_form: NULL argument");
  if (form != 1 && form != 2) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_emitter_pdf_form: form is 0, 1 or 2");
  if (!(c->cfg.features & rene::FEAT_SMALL) || c->view.small_bytes == 0)
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_emitter_pdf_form: forms 1 and 2 read the LDS image of a small-scene context (FEAT_SMALL)");
  if (n == 0) return RENE_OK;
  if (n > 0x7fffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, "too many rays in one batch");
  HIP_TRY(hipSetDevice(c->device));
  return run_probe("rene_emitter_pdf_form", c->stream, {{origins, n * 12}, {directions, n * 12}}, {{out, n * 4}}, [&](void* const* d) {
    return rene::launch_emitter_pdf_lds(c->view, form == 2, (uint32_t)n, (const float*)d[0], (const float*)d[1], (float*)d[2], c->stream);
  });
}

int rene_emit_sample(rene_ctx* c, int form, size_t n, const uint32_t* seeds, float* out8) {
  if (!c || (n && (!seeds || !out8))) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_emit_sample: NULL argument");
  if (form != 0 && form != 1) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_emit_sample: form is 0 or 1");
  if (c->view.emit_object_len == 0) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_emit_sample: the scene has no emitters");
  if (form == 1 && (!(c->cfg.features & rene::FEAT_SMALL) || c->view.small_bytes == 0))
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_emit_sample: form 1 reads the LDS image of a small-scene context (FEAT_SMALL)");
  if (n == 0) return RENE_OK;
  if (n > (1u << 24)) return fail(RENE_ERR_INVALID_ARGUMENT, "too many items in one batch");
  HIP_TRY(hipSetDevice(c->device));
  return run_probe("rene_emit_sample", c->stream, {{seeds, n * 4}}, {{out8, n * 32}}, [&](void* const* d) {
    return rene::launch_emit_sample(c->view, form == 1, (uint32_t)n, (const uint32_t*)d[0], (float*)d[1], c->stream);
  });
}

int rene_pcg_probe(int device, uint32_t seed, uint32_t n, uint32_t* out) {
  if (n && !out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_pcg_probe: NULL argument");
  if (n == 0) return RENE_OK;
  int n_dev = 0;
  HIP_TRY(hipGetDeviceCount(&n_dev));
  if (device < 0 || device >= n_dev) return fail(n_dev <= 0 ? RENE_ERR_DEVICE : RENE_ERR_INVALID_ARGUMENT, "rene_pcg_probe: no such HIP device");
  HIP_TRY(hipSetDevice(device));
  DevArray<uint32_t> d;
  if (int rc = d.reserve((size_t)n * 4, "rene_pcg_probe"); rc != RENE_OK) return rc;
  hipError_t e = rene::launch_pcg_probe(seed, n, d, nullptr);
  if (e == hipSuccess) e = hipMemcpy(out, d, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("rene_pcg_probe: ") + hipGetErrorString(e));
  return RENE_OK;
}

int rene_frame_stream_probe(rene_ctx* c, uint32_t first_frame, uint32_t n_frames, float* out) {
  if (!c || (n_frames && !out)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_frame_stream_probe: NULL argument");
  if (n_frames == 0) return RENE_OK;
  if (n_frames > rene::MAX_LAUNCH_FRAMES || (uint64_t)first_frame + n_frames > 0xffffffffull)
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_frame_stream_probe: frame range too long");
  if (!rene::select_kernel(c->cfg, c->view, c->opts.flags).reads_frame_stream)
    return fail(RENE_ERR_INVALID_ARGUMENT, "rene_frame_stream_probe: the kernel of this scene draws the frame-wide stream per lane (no table)");
  HIP_TRY(hipSetDevice(c->device));
  // a table of its own: the context's belongs to the launches in flight
  const size_t row = (size_t)rene::FRAME_STREAM_STRIDE * 4, floats = (size_t)n_frames * row;
  DevArray<float> d;
  if (int rc = d.reserve(floats * sizeof(float), "rene_frame_stream_probe"); rc != RENE_OK) return rc;
  std::vector<float> h(floats);
  hipError_t e = hipMemsetAsync(d, 0, floats * sizeof(float), c->stream);
  if (e == hipSuccess) e = rene::launch_frame_stream_fill(c->view, HostPcg(c->opts.seed).s, first_frame, 1u, n_frames, d, c->stream);
  if (e == hipSuccess) e = wait_stream(c->stream);
  if (e == hipSuccess) e = hipMemcpy(h.data(), d, floats * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("rene_frame_stream_probe: ") + hipGetErrorString(e));
  for (uint32_t i = 0; i < n_frames; ++i)
    std::memcpy(out + (size_t)i * rene::FRAME_STREAM_DEPTHS * 4, h.data() + i * row, (size_t)rene::FRAME_STREAM_DEPTHS * 4 * sizeof(float));
  return RENE_OK;
}

// Probe: the caller's frame chains instead of rendered ones (include/rene_hip.h).  No kernel: the owned tiles' pixels are scattered into slot order
// on the host (tile_slot, the inverse of what resolve_chains_kernel does) and copied through the pinned staging of the scene upload on the
// context's stream; the bookkeeping is then what rene_render(first_frame, n_frames) -- under tile_frames, an adaptive job -- leaves on a fresh context.
static int rene_load_chains_impl(rene_ctx* c, const float* chains, size_t n_floats, uint32_t first_frame, uint32_t n_frames, const uint32_t* tile_frames, size_t n_tiles) {
  if (!c || !chains) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_load_chains: NULL argument");
  if (c->opts.shard_mode != RENE_SHARD_TILES && c->opts.shard_count > 1)
    return fail(RENE_ERR_UNSUPPORTED, "rene_load_chains: a frame shard (RENE_SHARD_FRAMES, shard_count > 1) holds only its share of every pixel's frames; use an unsharded context or tile shards");
  if (c->exchanged)
    return fail(RENE_ERR_UNSUPPORTED, "rene_load_chains: the image has been through rene_reduce / rene_gather_tiles, which consumed the frame chains; rene_reset first");
  const size_t W = c->width, H = c->height, layer_floats = H * W * 3;
  if (n_floats < (size_t)rene::CHAINS * 3u * layer_floats) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_load_chains: fewer floats than [8][3][yres][xres][3]");
  if (n_frames == 0) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_load_chains: n_frames is 0");
  if ((uint64_t)first_frame + n_frames > 0xffffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_load_chains: frame range overflows u32");
  if (c->frames != 0 || c->loaded || !c->pending.empty()) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_load_chains: the context already holds frames; rene_reset first");
  if (tile_frames) {
    if (n_tiles != c->n_tiles) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_load_chains: n_tiles is not the tiles_y x tiles_x grid's");
    bool full = false;
    for (size_t t = 0; t < n_tiles; ++t) {
      if (tile_frames[t] > n_frames) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_load_chains: a tile with more than n_frames frames");
      full = full || tile_frames[t] == n_frames;
    }
    if (!full) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_load_chains: no tile holds n_frames frames");
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc = c->drain();
  if (rc != RENE_OK) return rc;
  // [CHAINS][3][n_slots][4] in slot order: the slots of ragged tiles outside the image and every record's version word stay 0, as rene_reset leaves them
  const uint32_t n_owned = c->n_owned();
  const size_t n_slots = c->n_work;
  std::vector<float> slots((size_t)rene::CHAINS * 3u * n_slots * 4u, 0.0f);
  for (uint32_t gl = 0; gl < rene::CHAINS * 3u; ++gl) {
    const float* src = chains + (size_t)gl * layer_floats;
    float* dst = slots.data() + (size_t)gl * n_slots * 4u;
    for (uint32_t k = 0; k < n_owned; ++k) {
      const uint32_t tile = c->owned_tile(k);
      const size_t x0 = (size_t)(tile % c->tiles_x) * RENE_TILE_SIZE, y0 = (size_t)(tile / c->tiles_x) * RENE_TILE_SIZE;
      for (uint32_t dy = 0; dy < RENE_TILE_SIZE && y0 + dy < H; ++dy)
        for (uint32_t dx = 0; dx < RENE_TILE_SIZE && x0 + dx < W; ++dx)
          std::memcpy(dst + ((size_t)k * rene::TILE_SLOTS + rene::tile_slot(dx, dy)) * 4u, src + ((y0 + dy) * W + x0 + dx) * 3u, 3 * sizeof(float));  // bit for bit
    }
  }
  if (!slots.empty()) {
    rc = c->staged_upload(c->chains, slots.data(), slots.size() * sizeof(float), c->stream);
    c->h_upload.release();
    if (rc != RENE_OK) return rc;
  }
  // the frames: N_t of the most-sampled owned tile, as rene_get_stats reports them; the owned tiles with fewer were switched off at theirs
  uint32_t frames = tile_frames ? 0u : n_frames;
  if (tile_frames)
    for (uint32_t k = 0; k < n_owned; ++k) frames = std::max(frames, tile_frames[c->owned_tile(k)]);
  c->clear_active_tiles();
  if (tile_frames) {
    std::vector<uint8_t> active(n_owned, 1);
    std::vector<uint32_t> stop(n_owned, 0u);
    for (uint32_t k = 0; k < n_owned; ++k) {
      const uint32_t nt = tile_frames[c->owned_tile(k)];
      if (nt == frames) continue;
      active[k] = 0;
      stop[k] = nt;
      ++c->n_inactive;
      c->inactive_pixels += c->tile_pixels(c->owned_tile(k));
    }
    if (c->n_inactive) {
      c->tile_active = std::move(active);
      c->tile_stop = std::move(stop);
    }
  }
  c->frames = frames;
  c->frame_base = first_frame;
  for (uint64_t& f : c->chain_frames) f = 0;
  c->count_chain_frames(first_frame & (rene::CHAINS - 1u), frames);
  c->fb_stale = true;  // the next hand-out resolves the loaded chains
  c->loaded = true;
  return RENE_OK;
}

// ---- checkpoint: save, restore and resume a job (include/rene_hip.h; kernels_state.hip packs and unpacks the chains) ---------------------------------
void rene_state_params_default(rene_state_params* out) {
  if (!out) return;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
}

int rene_scene_fingerprint(const rene_scene_desc* scene, uint64_t out[2]) { return scene_fingerprint(scene, out); }

static constexpr uint32_t kStateChunkDefault = 128, kStateChunkMax = 1024, kStateMaxRes = 16384;
static constexpr size_t kStateTile = RENE_STATE_TILE_BYTES;
static_assert(sizeof(rene_state_header) == 256 && sizeof(rene_state_tile) == 32, "the state format's header and table entry");

size_t rene_state_bytes(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count) {
  if (!width || !height || width > kStateMaxRes || height > kStateMaxRes || !shard_count || shard_rank >= shard_count) return 0;
  const uint32_t n_tiles = ((width + RENE_TILE_SIZE - 1u) / RENE_TILE_SIZE) * ((height + RENE_TILE_SIZE - 1u) / RENE_TILE_SIZE);
  return sizeof(rene_state_header) + (size_t)owned_tiles(n_tiles, shard_rank, shard_count) * (sizeof(rene_state_tile) + kStateTile);
}

// A part's header: `head` holds `avail` bytes of the part's beginning, `bytes` is the whole part's size (of the blob, of the file)
static int state_read_header(const std::string& me, const void* head, size_t avail, size_t bytes, rene_state_header& h) {
  if (!head) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL part");
  if (avail < sizeof(h) || bytes < sizeof(h))
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": truncated inside the header (" + std::to_string(std::min(avail, bytes)) + " bytes; the header has 256)");
  std::memcpy(&h, head, sizeof(h));
  if (h.magic != RENE_STATE_MAGIC) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": bad magic (not a render state)");
  if (h.version != RENE_STATE_VERSION) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": format version " + std::to_string(h.version) + ", this build reads version " + std::to_string(RENE_STATE_VERSION));
  if (h.header_bytes != sizeof(h) || h.tile_size != RENE_TILE_SIZE) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": header_bytes must be 256 and tile_size 32");
  if (!h.width || !h.height || h.width > kStateMaxRes || h.height > kStateMaxRes) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": film size out of range");
  if (h.tiles_x != (h.width + RENE_TILE_SIZE - 1u) / RENE_TILE_SIZE || h.tiles_y != (h.height + RENE_TILE_SIZE - 1u) / RENE_TILE_SIZE)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": tiles_x, tiles_y are not the film's tile grid");
  if (h.n_tiles > h.tiles_x * h.tiles_y) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": more tiles than the film's grid has");
  if (h.frames_contiguous > 1u || h.loaded > 1u) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": frames_contiguous and loaded must be 0 or 1");
  if (h.n_frames == 0) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a state without frames");
  if ((uint64_t)h.frame_base + h.n_frames > 0xffffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": frame range overflows u32");
  uint64_t in_chains = 0;
  for (uint64_t f : h.chain_frames) in_chains += std::min<uint64_t>(f, 0xffffffffull);
  if (in_chains != h.n_frames) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": chain_frames do not add up to n_frames");
  for (uint8_t r : h.reserved)
    if (r) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": a reserved header byte is not zero");
  if (h.payload_offset != sizeof(h) + (uint64_t)h.n_tiles * sizeof(rene_state_tile) || h.total_bytes != h.payload_offset + (uint64_t)h.n_tiles * kStateTile)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": payload_offset / total_bytes do not follow from n_tiles");
  if (bytes < h.payload_offset) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": truncated inside the tile table (" + std::to_string(bytes) + " of " + std::to_string(h.total_bytes) + " bytes)");
  if (bytes < h.total_bytes)
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": truncated inside the payload of the part's tile #" + std::to_string((bytes - h.payload_offset) / kStateTile) + " (" + std::to_string(bytes) + " of " +
                                               std::to_string(h.total_bytes) + " bytes)");
  if (bytes > h.total_bytes) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": " + std::to_string(bytes - h.total_bytes) + " bytes follow the part's " + std::to_string(h.total_bytes));
  return RENE_OK;
}

static int state_check_table(const std::string& me, const rene_state_header& h, const rene_state_tile* t) {
  bool full = h.n_tiles == 0;
  for (uint32_t i = 0; i < h.n_tiles; ++i) {
    const std::string tile = "tile " + std::to_string(t[i].tile);
    if (t[i].tile >= h.tiles_x * h.tiles_y) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": " + tile + " is outside the film's grid");
    if (i && t[i].tile == t[i - 1].tile) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": duplicate " + tile + " in the tile table");
    if (i && t[i].tile < t[i - 1].tile) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": tiles out of order in the tile table (" + tile + " after tile " + std::to_string(t[i - 1].tile) + ")");
    if (t[i].flags & ~RENE_STATE_TILE_ACTIVE) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": " + tile + " has unknown flags");
    if (t[i].reserved[0] | t[i].reserved[1] | t[i].reserved[2]) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": " + tile + " has a reserved word that is not zero");
    if (t[i].n_frames > h.n_frames) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": " + tile + " holds " + std::to_string(t[i].n_frames) + " frames, more than the part's N = " + std::to_string(h.n_frames));
    if ((t[i].flags & RENE_STATE_TILE_ACTIVE) && t[i].n_frames != h.n_frames)
      return fail(RENE_ERR_INVALID_ARGUMENT, me + ": active " + tile + " holds " + std::to_string(t[i].n_frames) + " frames, below the part's N = " + std::to_string(h.n_frames));
    full = full || t[i].n_frames == h.n_frames;
  }
  if (!full) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": no tile holds the part's N = " + std::to_string(h.n_frames) + " frames");
  return RENE_OK;
}

// header and table of a part in memory
static int state_read_blob(const std::string& me, const void* blob, size_t bytes, rene_state_header& h, std::vector<rene_state_tile>& tiles) {
  if (int rc = state_read_header(me, blob, bytes, bytes, h); rc != RENE_OK) return rc;
  tiles.resize(h.n_tiles);
  if (h.n_tiles) std::memcpy(tiles.data(), static_cast<const uint8_t*>(blob) + sizeof(h), (size_t)h.n_tiles * sizeof(rene_state_tile));
  return state_check_table(me, h, tiles.data());
}

static void state_info_of(const rene_state_header& h, rene_state_info* out) {
  rene_state_info o{};
  o.struct_size = sizeof(o);
  o.version = h.version, o.width = h.width, o.height = h.height, o.tile_size = h.tile_size, o.tiles_x = h.tiles_x, o.tiles_y = h.tiles_y;
  o.seed = h.seed, o.frame_base = h.frame_base, o.n_frames = h.n_frames, o.frames_contiguous = h.frames_contiguous, o.loaded = h.loaded, o.n_tiles = h.n_tiles;
  o.paths = h.paths;
  std::memcpy(o.chain_frames, h.chain_frames, sizeof(o.chain_frames));
  std::memcpy(o.fingerprint, h.fingerprint, sizeof(o.fingerprint));
  o.payload_offset = h.payload_offset, o.total_bytes = h.total_bytes;
  *out = o;
}

static int rene_state_inspect_impl(const void* blob, size_t bytes, rene_state_info* out) {
  if (!out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_state_inspect: NULL argument");
  if (out->struct_size != sizeof(*out)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_state_info.struct_size mismatch (ABI skew)");
  rene_state_header h;
  std::vector<rene_state_tile> tiles;
  if (int rc = state_read_blob("rene_state_inspect", blob, bytes, h, tiles); rc != RENE_OK) return rc;
  state_info_of(h, out);
  return RENE_OK;
}

static int rene_state_tiles_impl(const void* blob, size_t bytes, rene_state_tile* dst, size_t n) {
  rene_state_header h;
  std::vector<rene_state_tile> tiles;
  if (int rc = state_read_blob("rene_state_tiles", blob, bytes, h, tiles); rc != RENE_OK) return rc;
  if (tiles.empty()) return RENE_OK;
  if (!dst || n < tiles.size()) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_state_tiles: room for fewer entries than the part has tiles");
  std::memcpy(dst, tiles.data(), tiles.size() * sizeof(rene_state_tile));
  return RENE_OK;
}

// c0, c1 of one tile's payload on the host (the device's are kernels_state.hip's)
static void state_checksum(const uint8_t* payload, uint32_t& c0, uint32_t& c1) {
  c0 = c1 = 0;
  for (uint32_t i = 0; i < rene::STATE_TILE_DWORDS; ++i) {
    uint32_t w;
    std::memcpy(&w, payload + 4u * (size_t)i, 4);
    c0 += w;
    c1 += (i + 1u) * w;
  }
}
static std::string state_mismatch(const rene_state_tile& t, uint32_t c0, uint32_t c1) {
  char buf[160];
  std::snprintf(buf, sizeof buf, "checksum mismatch in tile %u: the payload gives c0 %08x c1 %08x, the table says c0 %08x c1 %08x", t.tile, c0, c1, t.c0, t.c1);
  return buf;
}

static int rene_state_verify_impl(const void* blob, size_t bytes) {
  rene_state_header h;
  std::vector<rene_state_tile> tiles;
  if (int rc = state_read_blob("rene_state_verify", blob, bytes, h, tiles); rc != RENE_OK) return rc;
  for (uint32_t i = 0; i < h.n_tiles; ++i) {
    uint32_t c0, c1;
    state_checksum(static_cast<const uint8_t*>(blob) + h.payload_offset + (size_t)i * kStateTile, c0, c1);
    if (c0 != tiles[i].c0 || c1 != tiles[i].c1) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_state_verify: " + state_mismatch(tiles[i], c0, c1));
  }
  return RENE_OK;
}

// is `p` host memory the HIP runtime has pinned (hipHostMalloc, hipHostRegister)?  Then a copy engine reads and writes it without a staging
static bool state_is_pinned(const void* p) {
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

// the files of the streamed calls: closed, and the unfinished one removed, whichever way the call ends
struct StateFile {
  int fd = -1;
  std::string unlink_path;
  StateFile() = default;
  StateFile(StateFile&& o) noexcept : fd(o.fd), unlink_path(std::move(o.unlink_path)) { o.fd = -1, o.unlink_path.clear(); }
  ~StateFile() {
    if (fd >= 0) ::close(fd);
    if (!unlink_path.empty()) ::unlink(unlink_path.c_str());
  }
  int write_at(size_t off, const void* p, size_t n) const {
    const char* q = static_cast<const char*>(p);
    while (n) {
      const ssize_t w = ::pwrite(fd, q, n, (off_t)off);
      if (w < 0 && errno == EINTR) continue;
      if (w <= 0) return -1;
      q += w, off += (size_t)w, n -= (size_t)w;
    }
    return 0;
  }
  int read_at(size_t off, void* p, size_t n) const {
    char* q = static_cast<char*>(p);
    while (n) {
      const ssize_t r = ::pread(fd, q, n, (off_t)off);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) return -1;
      q += r, off += (size_t)r, n -= (size_t)r;
    }
    return 0;
  }
};

// what both directions allocate on their first call, for chunks of `chunk` tiles: the two device chunk buffers, the two pinned stagings, the checksums
// of the owned tiles, the copies' stream and the events
static int state_prepare(const std::string& me, rene_ctx* c, const rene_state_params* params, uint32_t& chunk) {
  rene_state_params p;
  if (int rc = read_params("rene_state_params", rene_state_params_default, params, p); rc != RENE_OK) return rc;
  if (p.reserved[0] | p.reserved[1]) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": rene_state_params.reserved must be zero");
  if (p.chunk_tiles > kStateChunkMax) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": chunk_tiles must be at most " + std::to_string(kStateChunkMax));
  chunk = std::max(1u, std::min(p.chunk_tiles ? p.chunk_tiles : kStateChunkDefault, c->n_owned()));
  return RENE_OK;
}
static int state_alloc(const std::string& me, rene_ctx* c, uint32_t chunk) {
  for (int b = 0; b < 2; ++b) {
    if (int rc = c->state_dev[b].reserve((size_t)chunk * kStateTile, me + ": chunk buffer"); rc != RENE_OK) return rc;
    if (int rc = c->state_host[b].reserve((size_t)chunk * kStateTile, me + ": pinned staging"); rc != RENE_OK) return rc;
    if (!c->state_kernel_done[b].ev) HIP_TRY(c->state_kernel_done[b].create());
    if (!c->state_copy_done[b].ev) HIP_TRY(c->state_copy_done[b].create());
  }
  if (int rc = c->state_sums.reserve(std::max<size_t>(16, (size_t)c->n_owned() * 8u), me + ": checksums"); rc != RENE_OK) return rc;
  if (!c->state_stream) HIP_TRY(hipStreamCreateWithFlags(&c->state_stream, hipStreamNonBlocking));
  return RENE_OK;
}
static int state_refusals(const std::string& me, const rene_ctx* c) {
  if (c->opts.shard_mode != RENE_SHARD_TILES && c->opts.shard_count > 1)
    return fail(RENE_ERR_UNSUPPORTED, me + ": a frame shard (RENE_SHARD_FRAMES, shard_count > 1) holds only its share of every pixel's frames; use an unsharded context or tile shards");
  if (c->exchanged) return fail(RENE_ERR_UNSUPPORTED, me + ": the image has been through rene_reduce / rene_gather_tiles, which consumed the frame chains; rene_reset first");
  return RENE_OK;
}

// RENE_DEBUG: what the chunks' kernels took, by the events around them, and the pipeline's wall time
static void state_log(const std::string& me, const rene_ctx* c, const Marks& M, uint32_t n_owned, uint32_t chunk, bool direct, std::chrono::steady_clock::time_point t0) {
  if (!M.complete) return;
  double kernels = 0.0;
  for (size_t i = 0; i + 1 < M.size(); i += 2) kernels += M.ms(i, i + 1);
  std::fprintf(stderr, "[rene] %s %u x %u, %u tiles in chunks of %u, %s, ms: kernels %.4f, pipeline %.4f\n", me.c_str(), c->width, c->height, n_owned, chunk,
               direct ? "pinned memory" : "through the stagings", kernels, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// rene_save_state and rene_save_state_file: `direct`, where the destination is pinned memory, receives the payload straight from the device;
// else every chunk comes through a staging and `put(offset, bytes, n)` takes it from there.  `put` also takes header and table, last.
static int state_save(const std::string& me, rene_ctx* c, const rene_state_params* params, uint8_t* direct, const std::function<int(size_t, const void*, size_t)>& put) {
  if (int rc = state_refusals(me, c); rc != RENE_OK) return rc;
  if (c->frames == 0) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the context holds no frames");
  if (c->frames > 0xffffffffull || (uint64_t)c->frame_base + c->frames > 0xffffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": more than 2^32 - 1 frames");
  uint32_t chunk = 0;
  if (int rc = state_prepare(me, c, params, chunk); rc != RENE_OK) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = c->drain(); rc != RENE_OK) return rc;
  if (int rc = state_alloc(me, c, chunk); rc != RENE_OK) return rc;
  const uint32_t n_owned = c->n_owned();
  rene_state_header h{};
  h.magic = RENE_STATE_MAGIC, h.version = RENE_STATE_VERSION, h.header_bytes = sizeof(h), h.tile_size = RENE_TILE_SIZE;
  h.width = c->width, h.height = c->height, h.tiles_x = c->tiles_x, h.tiles_y = c->n_tiles / std::max(1u, c->tiles_x);
  // N is the largest N_t of the part, as the format says (of a context that owns no tile: its frames).  That is the context's frame count -- a tile
  // that is active holds every frame, and a context whose tiles have all stopped counts no further frame -- but the part is written from the tiles
  uint32_t n_part = n_owned ? 0u : (uint32_t)c->frames;
  for (uint32_t k = 0; k < n_owned; ++k) n_part = std::max(n_part, c->tile_n(k));
  if (n_part == 0) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": no tile of the context holds a frame");
  h.seed = c->opts.seed, h.frame_base = c->frame_base, h.n_frames = n_part;
  h.frames_contiguous = c->frames_contiguous ? 1u : 0u, h.loaded = c->loaded ? 1u : 0u, h.n_tiles = n_owned;
  h.paths = c->paths;
  for (uint32_t g = 0; g < rene::CHAINS; ++g) h.chain_frames[g] = c->chain_frames[g];
  if (n_part != c->frames) {  // the chains' counts of the frames [F, F + N), by the chain rule
    uint64_t cf[rene::CHAINS];
    rene_ctx::chain_counts(c->frame_base, n_part, cf);
    for (uint32_t g = 0; g < rene::CHAINS; ++g) h.chain_frames[g] = cf[g];
  }
  h.fingerprint[0] = c->fingerprint[0], h.fingerprint[1] = c->fingerprint[1];
  h.payload_offset = sizeof(h) + (uint64_t)n_owned * sizeof(rene_state_tile);
  h.total_bytes = h.payload_offset + (uint64_t)n_owned * kStateTile;
  // the pipeline: the pack kernel of chunk i on the context's stream, its copy on the copies' stream behind it; the kernel of chunk i waits ON THE
  // DEVICE for the copy of chunk i - 2, which frees chunk buffer i & 1.  Into pinned memory the host therefore enqueues every chunk ahead and waits
  // once; through the stagings it takes chunk i - 1 from its staging while chunk i is packed and copied
  const rene::TileGrid G = tile_grid(c);
  const uint32_t n_chunks = (n_owned + chunk - 1u) / chunk;
  const auto tiles_of = [&](uint32_t i) { return std::min(chunk, n_owned - i * chunk); };
  hipError_t e = hipSuccess;
  const auto take = [&](uint32_t i) -> int {
    if (direct) return RENE_OK;
    e = wait_event(c->state_copy_done[i & 1u]);
    if (e != hipSuccess) return RENE_ERR_DEVICE;
    return put(h.payload_offset + (size_t)i * chunk * kStateTile, c->state_host[i & 1u].p, (size_t)tiles_of(i) * kStateTile);
  };
  int rc = RENE_OK;
  Marks M(c->stream);  // RENE_DEBUG: an event on either side of every chunk's kernel
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 0; i < n_chunks && rc == RENE_OK; ++i) {
    const uint32_t b = i & 1u;
    const size_t bytes = (size_t)tiles_of(i) * kStateTile;
    if (i >= 2u) e = hipStreamWaitEvent(c->stream, c->state_copy_done[b], 0);  // (as recorded for chunk i - 2)
    M.mark();
    if (e == hipSuccess) e = rene::launch_state(c->chains, c->state_dev[b].p, c->state_sums.p, rene::StateLaunch{G, i * chunk, tiles_of(i)}, false, c->stream);
    M.mark();
    void* to = direct ? static_cast<void*>(direct + h.payload_offset + (size_t)i * chunk * kStateTile) : c->state_host[b].p;
    if (e == hipSuccess) e = hipEventRecord(c->state_kernel_done[b], c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->state_stream, c->state_kernel_done[b], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(to, c->state_dev[b].p, bytes, hipMemcpyDeviceToHost, c->state_stream);
    if (e == hipSuccess) e = hipEventRecord(c->state_copy_done[b], c->state_stream);
    if (e != hipSuccess) break;
    if (i) rc = take(i - 1u);
  }
  if (e == hipSuccess && rc == RENE_OK && n_chunks) rc = take(n_chunks - 1u);
  // whichever way the pipeline ended -- a HIP error, a `put` that failed -- nothing of the call stays in flight: no copy into a staging or into the
  // caller's memory outlives it
  const hipError_t e_copy = hipStreamSynchronize(c->state_stream), e_kernel = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = e_copy != hipSuccess ? e_copy : e_kernel;
  if (e != hipSuccess) return fail(RENE_ERR_DEVICE, me + ": " + hipGetErrorString(e));
  if (rc != RENE_OK) return rc;
  state_log(me, c, M, n_owned, chunk, direct != nullptr, t0);
  std::vector<uint32_t> sums((size_t)n_owned * 2u);
  if (n_owned) HIP_TRY(hipMemcpy(sums.data(), c->state_sums.p, sums.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<uint8_t> head(h.payload_offset);
  std::memcpy(head.data(), &h, sizeof(h));
  for (uint32_t k = 0; k < n_owned; ++k) {
    rene_state_tile t{};
    t.tile = c->owned_tile(k), t.n_frames = c->tile_n(k);
    t.flags = (!c->n_inactive || c->tile_active[k]) ? RENE_STATE_TILE_ACTIVE : 0u;
    t.c0 = sums[2u * k], t.c1 = sums[2u * k + 1u];
    std::memcpy(head.data() + sizeof(h) + (size_t)k * sizeof(t), &t, sizeof(t));
  }
  return put(0, head.data(), head.size());
}

static int rene_save_state_impl(rene_ctx* c, const rene_state_params* params, void* dst, size_t dst_bytes, size_t* written) {
  if (!c || !dst) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_save_state: NULL argument");
  const size_t need = sizeof(rene_state_header) + (size_t)c->n_owned() * (sizeof(rene_state_tile) + kStateTile);
  if (dst_bytes < need) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_save_state: the destination has " + std::to_string(dst_bytes) + " bytes, the state needs " + std::to_string(need));
  uint8_t* const out = static_cast<uint8_t*>(dst);
  int rc = state_save("rene_save_state", c, params, state_is_pinned(dst) ? out : nullptr, [&](size_t off, const void* p, size_t n) {
    std::memcpy(out + off, p, n);
    return RENE_OK;
  });
  if (rc == RENE_OK && written) *written = need;
  return rc;
}

static int rene_save_state_file_impl(rene_ctx* c, const rene_state_params* params, const char* path) {
  if (!c || !path || !*path) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_save_state_file: NULL argument");
  const std::string me = "rene_save_state_file", tmp = std::string(path) + ".tmp";
  if (int rc = state_refusals(me, c); rc != RENE_OK) return rc;  // (before a file is touched)
  if (c->frames == 0) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the context holds no frames");
  StateFile f;
  f.fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (f.fd < 0) return fail(RENE_ERR_IO, me + ": cannot create " + tmp + ": " + std::strerror(errno));
  f.unlink_path = tmp;
  int rc = state_save(me, c, params, nullptr, [&](size_t off, const void* p, size_t n) {
    return f.write_at(off, p, n) == 0 ? RENE_OK : fail(RENE_ERR_IO, me + ": cannot write " + tmp + ": " + std::strerror(errno));
  });
  if (rc != RENE_OK) return rc;
  const bool synced = ::fsync(f.fd) == 0;
  const int saved_errno = errno;
  const bool closed = ::close(f.fd) == 0;  // (closed whether or not the sync failed)
  f.fd = -1;
  if (!synced || !closed) {
    if (!synced) errno = saved_errno;
    return fail(RENE_ERR_IO, me + ": cannot finish " + tmp + ": " + std::strerror(errno));
  }
  if (::rename(tmp.c_str(), path) != 0) return fail(RENE_ERR_IO, me + ": cannot rename " + tmp + " to " + path + ": " + std::strerror(errno));
  f.unlink_path.clear();
  return RENE_OK;
}

// one part of a restore: its header and table, and where its payload is -- memory (pinned or not) or a file
struct StatePart {
  rene_state_header h{};
  std::vector<rene_state_tile> tiles;
  const uint8_t* mem = nullptr;
  bool pinned = false;
  StateFile file;
};

static int state_restore(const std::string& me, rene_ctx* c, const rene_state_params* params, std::vector<StatePart>& parts) {
  // everything is checked before anything is written
  if (int rc = state_refusals(me, c); rc != RENE_OK) return rc;
  if (c->frames != 0 || c->loaded || !c->pending.empty()) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the context already holds frames; rene_reset first");
  if (parts.empty()) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": no part given");
  uint32_t chunk = 0;
  if (int rc = state_prepare(me, c, params, chunk); rc != RENE_OK) return rc;
  size_t ref = 0;  // the part with the largest N: the job's frames (a shard whose tiles all stopped earlier carries the counts of its own N)
  for (size_t p = 1; p < parts.size(); ++p)
    if (parts[p].h.n_frames > parts[ref].h.n_frames) ref = p;
  const rene_state_header& h0 = parts[ref].h;
  uint32_t n_max = 0;
  bool all_owned = true;
  uint64_t header_paths = 0;
  const uint32_t n_owned = c->n_owned();
  struct Where { uint32_t part, index; };
  std::vector<Where> where(c->n_tiles, Where{0xffffffffu, 0u});
  for (size_t p = 0; p < parts.size(); ++p) {
    const rene_state_header& h = parts[p].h;
    const std::string part = me + ": part " + std::to_string(p);
    if (h.width != c->width || h.height != c->height)
      return fail(RENE_ERR_INVALID_ARGUMENT, part + " is of a " + std::to_string(h.width) + " x " + std::to_string(h.height) + " film, the context renders " + std::to_string(c->width) + " x " + std::to_string(c->height));
    if (h.seed != c->opts.seed) return fail(RENE_ERR_INVALID_ARGUMENT, part + " was rendered with seed " + std::to_string(h.seed) + ", the context has seed " + std::to_string(c->opts.seed));
    if (h.fingerprint[0] != c->fingerprint[0] || h.fingerprint[1] != c->fingerprint[1]) return fail(RENE_ERR_INVALID_ARGUMENT, part + " is of another scene (the scene fingerprints differ)");
    if (h.frame_base != h0.frame_base || h.frames_contiguous != h0.frames_contiguous || h.loaded != h0.loaded ||
        (h.n_frames == h0.n_frames && std::memcmp(h.chain_frames, h0.chain_frames, sizeof(h.chain_frames)) != 0))
      return fail(RENE_ERR_INVALID_ARGUMENT, part + " does not agree with part " + std::to_string(ref) + " in frame_base, frames_contiguous, loaded or chain_frames: the parts are not of one job");
    header_paths += h.paths;
    for (uint32_t i = 0; i < h.n_tiles; ++i) {
      const rene_state_tile& t = parts[p].tiles[i];
      n_max = std::max(n_max, t.n_frames);
      if (where[t.tile].part != 0xffffffffu) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": tile " + std::to_string(t.tile) + " is in part " + std::to_string(where[t.tile].part) + " and in part " + std::to_string(p));
      where[t.tile] = Where{(uint32_t)p, i};
    }
  }
  bool stopped = false;
  for (const StatePart& P : parts)
    for (const rene_state_tile& t : P.tiles)
      if ((t.flags & RENE_STATE_TILE_ACTIVE) && t.n_frames != n_max)
        return fail(RENE_ERR_INVALID_ARGUMENT, me + ": active tile " + std::to_string(t.tile) + " holds " + std::to_string(t.n_frames) + " frames, below the parts' N = " + std::to_string(n_max));
  std::vector<uint8_t> owned_flag(c->n_tiles, 0);
  for (uint32_t k = 0; k < n_owned; ++k) {
    const uint32_t tile = c->owned_tile(k);
    owned_flag[tile] = 1;
    if (where[tile].part == 0xffffffffu) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": tile " + std::to_string(tile) + ", which the context owns, is missing from the parts");
    stopped = stopped || !(parts[where[tile].part].tiles[where[tile].index].flags & RENE_STATE_TILE_ACTIVE);
  }
  for (uint32_t t = 0; t < c->n_tiles; ++t) all_owned = all_owned && (where[t].part == 0xffffffffu || owned_flag[t]);
  if (stopped && !h0.loaded && (c->opts.flags & RENE_FLAG_WAVEFRONT))
    return fail(RENE_ERR_INVALID_ARGUMENT, me + ": the state has stopped tiles (rene_set_active_tiles), which a RENE_FLAG_WAVEFRONT context cannot render on");
  HIP_TRY(hipSetDevice(c->device));
  if (int rc = c->drain(); rc != RENE_OK) return rc;
  if (int rc = state_alloc(me, c, chunk); rc != RENE_OK) return rc;
  const auto tile_of = [&](uint32_t k) -> const rene_state_tile& { const Where& w = where[c->owned_tile(k)]; return parts[w.part].tiles[w.index]; };

  // the pipeline: chunk i's payloads into staging i & 1 (or straight from a pinned part), the copy on the copies' stream, the unpack kernel on the
  // context's behind it.  The copy of chunk i waits ON THE DEVICE for the kernel of chunk i - 2, which frees chunk buffer i & 1; the host waits
  // only before it writes a staging again -- for the copy of chunk i - 2 out of it -- so pinned parts are enqueued ahead without a wait
  const rene::TileGrid G = tile_grid(c);
  const uint32_t n_chunks = (n_owned + chunk - 1u) / chunk;
  const auto failed = [&](int code) {  // nothing of the call stays in flight, and the context is as rene_reset leaves it
    hipStreamSynchronize(c->state_stream);
    hipStreamSynchronize(c->stream);
    const std::string msg = g_error;
    rene_reset(c);
    return fail(code, msg);
  };
  Marks M(c->stream);
  const auto t0 = std::chrono::steady_clock::now();
  bool any_pinned = false;
  for (uint32_t i = 0; i < n_chunks; ++i) {
    const uint32_t b = i & 1u, k0 = i * chunk, n = std::min(chunk, n_owned - k0);
    bool staging_free = i < 2u;  // (is the copy of chunk i - 2 out of staging i & 1 known to be done?)
    if (i >= 2u) {
      const hipError_t e = hipStreamWaitEvent(c->state_stream, c->state_kernel_done[b], 0);  // (as recorded for chunk i - 2)
      if (e != hipSuccess) {
        fail(RENE_ERR_DEVICE, me + ": " + hipGetErrorString(e));
        return failed(RENE_ERR_DEVICE);
      }
    }
    uint8_t* const stage = c->state_host[b].as<uint8_t>();
    uint8_t* const dev = c->state_dev[b].as<uint8_t>();
    for (uint32_t j = 0; j < n;) {  // runs of tiles that follow one another in one part: one copy each
      const Where w = where[c->owned_tile(k0 + j)];
      uint32_t len = 1;
      while (j + len < n && where[c->owned_tile(k0 + j + len)].part == w.part && where[c->owned_tile(k0 + j + len)].index == w.index + len) ++len;
      const StatePart& P = parts[w.part];
      const size_t off = P.h.payload_offset + (size_t)w.index * kStateTile, bytes = (size_t)len * kStateTile;
      const void* from = stage + (size_t)j * kStateTile;
      any_pinned = any_pinned || (P.mem && P.pinned);
      if (!(P.mem && P.pinned) && !staging_free) {
        const hipError_t e = wait_event(c->state_copy_done[b]);
        if (e != hipSuccess) {
          fail(RENE_ERR_DEVICE, me + ": " + hipGetErrorString(e));
          return failed(RENE_ERR_DEVICE);
        }
        staging_free = true;
      }
      if (P.mem && P.pinned) from = P.mem + off;
      else if (P.mem) std::memcpy(stage + (size_t)j * kStateTile, P.mem + off, bytes);
      else if (P.file.read_at(off, stage + (size_t)j * kStateTile, bytes) != 0) {
        fail(RENE_ERR_IO, me + ": cannot read the payload of part " + std::to_string(w.part) + ": " + std::strerror(errno));
        return failed(RENE_ERR_IO);
      }
      const hipError_t e = hipMemcpyAsync(dev + (size_t)j * kStateTile, from, bytes, hipMemcpyHostToDevice, c->state_stream);
      if (e != hipSuccess) {
        fail(RENE_ERR_DEVICE, me + " upload: " + hipGetErrorString(e));
        return failed(RENE_ERR_DEVICE);
      }
      j += len;
    }
    hipError_t e = hipEventRecord(c->state_copy_done[b], c->state_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->state_copy_done[b], 0);
    M.mark();
    if (e == hipSuccess) e = rene::launch_state(c->chains, dev, c->state_sums.p, rene::StateLaunch{G, k0, n}, true, c->stream);
    M.mark();
    if (e == hipSuccess) e = hipEventRecord(c->state_kernel_done[b], c->stream);
    if (e != hipSuccess) {
      fail(RENE_ERR_DEVICE, me + " launch: " + hipGetErrorString(e));
      return failed(RENE_ERR_DEVICE);
    }
  }
  hipError_t e = wait_stream(c->state_stream);
  if (e == hipSuccess) e = wait_stream(c->stream);
  std::vector<uint32_t> sums((size_t)n_owned * 2u);
  if (e == hipSuccess && n_owned) e = hipMemcpy(sums.data(), c->state_sums.p, sums.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    fail(RENE_ERR_DEVICE, me + ": " + hipGetErrorString(e));
    return failed(RENE_ERR_DEVICE);
  }
  state_log(me, c, M, n_owned, chunk, any_pinned, t0);
  for (uint32_t k = 0; k < n_owned; ++k) {  // what arrived on the device against the table
    const rene_state_tile& t = tile_of(k);
    if (sums[2u * k] != t.c0 || sums[2u * k + 1u] != t.c1) {
      fail(RENE_ERR_INVALID_ARGUMENT, me + ": " + state_mismatch(t, sums[2u * k], sums[2u * k + 1u]) + "; the context has been reset");
      return failed(RENE_ERR_INVALID_ARGUMENT);
    }
  }
  // the bookkeeping rene_load_chains leaves, with the table's active flags and the headers' paths, chain counts and `loaded`
  uint32_t frames = n_owned ? 0u : n_max;
  for (uint32_t k = 0; k < n_owned; ++k) frames = std::max(frames, tile_of(k).n_frames);
  c->clear_active_tiles();
  std::vector<uint8_t> active(n_owned, 1);
  std::vector<uint32_t> stop(n_owned, 0u);
  uint64_t tile_paths = 0;
  for (uint32_t k = 0; k < n_owned; ++k) {
    const rene_state_tile& t = tile_of(k);
    tile_paths += (uint64_t)t.n_frames * c->tile_pixels(c->owned_tile(k));
    if (t.flags & RENE_STATE_TILE_ACTIVE) continue;
    active[k] = 0;
    stop[k] = t.n_frames;
    ++c->n_inactive;
    c->inactive_pixels += c->tile_pixels(c->owned_tile(k));
  }
  if (c->n_inactive) {
    const size_t words = (n_owned + 31u) / 32u;  // the launches' mask, as rene_set_active_tiles uploads it
    if (int rc_ = c->mask_dev.reserve(words * sizeof(uint32_t), me + ": active-tile mask"); rc_ != RENE_OK) return failed(rc_);
    std::vector<uint32_t> bits(words, 0u);
    for (uint32_t k = 0; k < n_owned; ++k)
      if (active[k]) bits[k >> 5] |= 1u << (k & 31u);
    if (hipMemcpy(c->mask_dev.p, bits.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
      fail(RENE_ERR_DEVICE, me + ": active-tile mask upload failed");
      return failed(RENE_ERR_DEVICE);
    }
    c->tile_active = std::move(active);
    c->tile_stop = std::move(stop);
  }
  c->frames = frames;
  c->frame_base = h0.frame_base;
  c->frames_contiguous = h0.frames_contiguous != 0;
  for (uint64_t& f : c->chain_frames) f = 0;
  if (frames == h0.n_frames)
    for (uint32_t g = 0; g < rene::CHAINS; ++g) c->chain_frames[g] = h0.chain_frames[g];
  else c->count_chain_frames(h0.frame_base & (rene::CHAINS - 1u), frames);  // (a shard whose tiles all stopped below the job's N)
  c->loaded = h0.loaded != 0;
  c->paths = c->loaded ? 0u : all_owned ? header_paths : tile_paths;
  c->fb_stale = true;  // the next hand-out resolves the restored chains
  return RENE_OK;
}

static int rene_restore_state_impl(rene_ctx* c, const rene_state_params* params, const void* const* blobs, const size_t* blob_bytes, size_t n_parts) {
  if (!c || !blobs || !blob_bytes) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_restore_state: NULL argument");
  const std::string me = "rene_restore_state";
  std::vector<StatePart> parts(n_parts);
  for (size_t p = 0; p < n_parts; ++p) {
    if (int rc = state_read_blob(me + ": part " + std::to_string(p), blobs[p], blob_bytes[p], parts[p].h, parts[p].tiles); rc != RENE_OK) return rc;
    parts[p].mem = static_cast<const uint8_t*>(blobs[p]);
  }
  if (hipSetDevice(c->device) == hipSuccess)
    for (StatePart& P : parts) P.pinned = state_is_pinned(P.mem);
  return state_restore(me, c, params, parts);
}

// header and table of a part in a file, which stays open in P.file for its payload
static int state_open_file(const std::string& part, const char* path, StatePart& P) {
  P.file.fd = ::open(path, O_RDONLY | O_CLOEXEC);
  struct stat st{};
  if (P.file.fd < 0 || ::fstat(P.file.fd, &st) != 0) return fail(RENE_ERR_IO, part + ": cannot open: " + std::strerror(errno));
  uint8_t head[sizeof(rene_state_header)];
  const size_t avail = std::min<size_t>(sizeof(head), (size_t)st.st_size);
  if (avail && P.file.read_at(0, head, avail) != 0) return fail(RENE_ERR_IO, part + ": cannot read: " + std::strerror(errno));
  if (int rc = state_read_header(part, head, avail, (size_t)st.st_size, P.h); rc != RENE_OK) return rc;
  P.tiles.resize(P.h.n_tiles);
  if (P.h.n_tiles && P.file.read_at(sizeof(head), P.tiles.data(), (size_t)P.h.n_tiles * sizeof(rene_state_tile)) != 0) return fail(RENE_ERR_IO, part + ": cannot read: " + std::strerror(errno));
  return state_check_table(part, P.h, P.tiles.data());
}

static int rene_restore_state_files_impl(rene_ctx* c, const rene_state_params* params, const char* const* paths, size_t n_paths) {
  if (!c || !paths) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_restore_state_files: NULL argument");
  const std::string me = "rene_restore_state_files";
  std::vector<StatePart> parts(n_paths);
  for (size_t p = 0; p < n_paths; ++p) {
    if (!paths[p]) return fail(RENE_ERR_INVALID_ARGUMENT, me + ": NULL path");
    if (int rc = state_open_file(me + ": " + paths[p], paths[p], parts[p]); rc != RENE_OK) return rc;
  }
  return state_restore(me, c, params, parts);
}

static int rene_state_inspect_file_impl(const char* path, rene_state_info* out, rene_state_tile* tiles, size_t n) {
  if (!path || !out) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_state_inspect_file: NULL argument");
  if (out->struct_size != sizeof(*out)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_state_info.struct_size mismatch (ABI skew)");
  StatePart P;
  if (int rc = state_open_file(std::string("rene_state_inspect_file: ") + path, path, P); rc != RENE_OK) return rc;
  if (tiles && n < P.tiles.size()) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_state_inspect_file: room for fewer entries than the part has tiles");
  state_info_of(P.h, out);
  if (tiles && !P.tiles.empty()) std::memcpy(tiles, P.tiles.data(), P.tiles.size() * sizeof(rene_state_tile));
  return RENE_OK;
}

// ---- multi-GPU exchange step: RCCL over xGMI (include/rene_hip.h) ------------------------------------------------
static_assert(RENE_COMM_ID_BYTES == sizeof(ncclUniqueId), "rene_comm_unique_id hands out an ncclUniqueId");

int rene_comm_unique_id(uint8_t id[RENE_COMM_ID_BYTES]) {
  if (!id) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_comm_unique_id: NULL argument");
  Rccl* R = rccl();
  if (!R->handle) return fail(RENE_ERR_UNSUPPORTED, R->error);
  ncclUniqueId u;
  RCCL_TRY(R->GetUniqueId(&u));
  std::memcpy(id, &u, sizeof(u));
  return RENE_OK;
}

int rene_comm_init(rene_ctx* c, int n_ranks, int rank, const uint8_t id[RENE_COMM_ID_BYTES]) {
  if (!c || !id) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_comm_init: NULL argument");
  if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_comm_init: rank out of range");
  if (c->comm) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_comm_init: the context already belongs to a communicator");
  Rccl* R = rccl();
  if (!R->handle) return fail(RENE_ERR_UNSUPPORTED, R->error);
  HIP_TRY(hipSetDevice(c->device));
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  RCCL_TRY(R->CommInitRank(&c->comm, n_ranks, u, rank));
  c->comm_ranks = n_ranks;
  c->comm_rank = rank;
  return RENE_OK;
}

int rene_comm_init_all(rene_ctx** ctxs, int n) {
  if (!ctxs || n < 1) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_comm_init_all: NULL argument");
  std::vector<int> devs(n);
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i] || ctxs[i]->comm) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_comm_init_all: NULL context or context already in a communicator");
    devs[i] = ctxs[i]->device;
  }
  Rccl* R = rccl();
  if (!R->handle) return fail(RENE_ERR_UNSUPPORTED, R->error);
  std::vector<ncclComm_t> comms(n);
  RCCL_TRY(R->CommInitAll(comms.data(), n, devs.data()));
  for (int i = 0; i < n; ++i) {
    ctxs[i]->comm = comms[i];
    ctxs[i]->comm_ranks = n;
    ctxs[i]->comm_rank = i;
  }
  return RENE_OK;
}

int rene_comm_group_begin(void) {
  Rccl* R = rccl();
  if (!R->handle) return fail(RENE_ERR_UNSUPPORTED, R->error);
  RCCL_TRY(R->GroupStart());
  return RENE_OK;
}
int rene_comm_group_end(void) {
  Rccl* R = rccl();
  if (!R->handle) return fail(RENE_ERR_UNSUPPORTED, R->error);
  RCCL_TRY(R->GroupEnd());
  return RENE_OK;
}

int rene_reduce(rene_ctx* c, int root) {
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_reduce: NULL context");
  if (!c->comm) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_reduce: rene_comm_init first");
  if (root < 0 || root >= c->comm_ranks) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_reduce: root out of range");
  Rccl* R = rccl();
  HIP_TRY(hipSetDevice(c->device));
  {  // every launch has completed (and any dropped work item has been rendered by a replay) before the image is summed
    int rc = c->drain();
    if (rc != RENE_OK) return rc;
  }
  c->exchanged = true;
  RCCL_TRY(R->Reduce(c->fb, c->fb, c->fb_floats, ncclFloat, ncclSum, root, c->comm, c->stream));
  return RENE_OK;
}

// What rene_gather_tiles and rene_gather_denoise check first: a context in a communicator, a root inside it, and the shard layout the communicator's
// ranks stand for.  of_one: an unsharded context in a communicator of one passes as a shard of one
static int gather_check(const char* fn_, const rene_ctx* c, int root, bool of_one) {
  const std::string fn = fn_;
  if (!c) return fail(RENE_ERR_INVALID_ARGUMENT, fn + ": NULL context");
  if (!c->comm) return fail(RENE_ERR_INVALID_ARGUMENT, fn + ": rene_comm_init first");
  if (root < 0 || root >= c->comm_ranks) return fail(RENE_ERR_INVALID_ARGUMENT, fn + ": root out of range");
  const uint32_t n = (uint32_t)c->comm_ranks;
  if (of_one && n == 1 && c->opts.shard_count == 1) return RENE_OK;
  if (c->opts.shard_mode != RENE_SHARD_TILES || c->opts.shard_count != n || c->opts.shard_rank != (uint32_t)c->comm_rank)
    return fail(RENE_ERR_INVALID_ARGUMENT, fn + ": the context must be tile-sharded with shard_count == n_ranks and shard_rank == rank");
  return RENE_OK;
}

// The root's receives, one group: bytes_of(r) bytes from every other rank r (a multiple of 16: sent as floats; 0: that rank sends nothing), one
// after the other in rank order from the start of `buf`
static int gather_receive(Rccl* R, rene_ctx* c, int root, void* buf, const std::function<size_t(uint32_t)>& bytes_of) {
  RCCL_TRY(R->GroupStart());
  size_t off = 0;
  for (uint32_t r = 0; r < (uint32_t)c->comm_ranks; ++r) {
    const size_t bytes = (int)r == root ? 0 : bytes_of(r);
    if (bytes == 0) continue;
    ncclResult_t rr = R->Recv(static_cast<char*>(buf) + off, bytes / sizeof(float), ncclFloat, (int)r, c->comm, c->stream);
    if (rr != ncclSuccess) { R->GroupEnd(); return fail(RENE_ERR_DEVICE, std::string("ncclRecv: ") + R->GetErrorString(rr)); }
    off += bytes;
  }
  RCCL_TRY(R->GroupEnd());
  return RENE_OK;
}

int rene_gather_tiles(rene_ctx* c, int root) {
  if (int rc = gather_check("rene_gather_tiles", c, root, false); rc != RENE_OK) return rc;
  const uint32_t n = (uint32_t)c->comm_ranks;
  Rccl* R = rccl();
  HIP_TRY(hipSetDevice(c->device));
  {  // as rene_reduce: what is packed and sent is a complete image
    int rc = c->drain();
    if (rc != RENE_OK) return rc;
  }
  c->exchanged = true;
  const size_t tile_bytes = (size_t)3 * RENE_TILE_SIZE * RENE_TILE_SIZE * 4 * sizeof(float);
  auto bytes_of = [&](uint32_t r) { return owned_tiles(c->n_tiles, r, n) * tile_bytes; };
  const bool is_root = c->comm_rank == root;
  // packed staging: a sender its own tiles; the root those of every other rank, one after the other
  size_t need = 0;
  if (n == 1) need = bytes_of(0);
  else if (is_root) { for (uint32_t r = 0; r < n; ++r) if ((int)r != root) need += bytes_of(r); }
  else need = bytes_of((uint32_t)c->comm_rank);
  if (int rc = c->tile_buf.reserve(std::max<size_t>(16, need), "rene_gather_tiles staging"); rc != RENE_OK) return rc;
  float* const tile_buf = c->tile_buf.as<float>();
  if (n == 1) {
    // a communicator of one has nothing to send; it still packs its tiles, clears the image and places them again, so
    // that the two kernels of the exchange run (and are tested) wherever the library does
    hipError_t e = rene::launch_pack_tiles(c->fb, tile_buf, c->width, c->height, c->tiles_x, c->n_tiles, 0u, 1u, false, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->fb, 0, c->fb_floats * sizeof(float), c->stream);
    if (e == hipSuccess) e = rene::launch_pack_tiles(c->fb, tile_buf, c->width, c->height, c->tiles_x, c->n_tiles, 0u, 1u, true, c->stream);
    if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("rene_gather_tiles: ") + hipGetErrorString(e));
    return RENE_OK;
  }
  if (!is_root) {
    hipError_t e = rene::launch_pack_tiles(c->fb, tile_buf, c->width, c->height, c->tiles_x, c->n_tiles, (uint32_t)c->comm_rank, n, false, c->stream);
    if (e != hipSuccess) return fail(RENE_ERR_DEVICE, std::string("rene_gather_tiles pack: ") + hipGetErrorString(e));
    if (need) RCCL_TRY(R->Send(tile_buf, need / sizeof(float), ncclFloat, root, c->comm, c->stream));
    return RENE_OK;
  }
  if (int rc = gather_receive(R, c, root, tile_buf, bytes_of); rc != RENE_OK) return rc;
  // the received tiles are placed by the next call that waits for or hands out the image (rene_sync, rene_download,
  // rene_get_stats, rene_framebuffer): inside a caller's rene_comm_group_begin / _end the receives above are only
  // enqueued when the outermost group ends, and the placing kernels must come behind them on the stream
  c->unpack_root = root;
  return RENE_OK;
}

int rene_gather_denoise(rene_ctx* c, int root) {
  if (int rc = gather_check("rene_gather_denoise", c, root, true); rc != RENE_OK) return rc;  // (an unsharded context is a shard of one)
  const uint32_t n = (uint32_t)c->comm_ranks;
  if (!c->dn_shard.valid) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_gather_denoise: rene_denoise_shard_prepare first (before rene_gather_tiles consumes the chains)");
  Rccl* R = rccl();
  HIP_TRY(hipSetDevice(c->device));
  if (c->comm_rank != root) {  // (the packed buffer is a multiple of 16 bytes: sent as floats, like the tiles of rene_gather_tiles)
    RCCL_TRY(R->Send(c->dn_shard.buf.p, c->dn_shard.bytes / sizeof(float), ncclFloat, root, c->comm, c->stream));
    return RENE_OK;
  }
  auto bytes_of = [&](uint32_t r) { return rene_denoise_shard_bytes(c->width, c->height, r, n); };
  size_t need = 0;
  for (uint32_t r = 0; r < n; ++r)
    if ((int)r != root) need += bytes_of(r);
  if (int rc = c->dn_gather_buf.reserve(need, "rene_gather_denoise staging"); rc != RENE_OK) return rc;
  if (n > 1)
    if (int rc = gather_receive(R, c, root, c->dn_gather_buf.p, bytes_of); rc != RENE_OK) return rc;
  // placed by rene_denoise_placed, behind the receives on the stream (as rene_gather_tiles defers its unpack); a communicator of one has
  // nothing to receive and still goes through place and filter
  c->dn_gather_root = root;
  return RENE_OK;
}

// ---- output transform, rene/src/main.rs:1758-1810 ---------------------------------------------------------
static float gamma_correct(float v) {  // main.rs:1768-1774
  if (v <= 0.0031308f) return 12.92f * v;
  return 1.055f * std::pow(v, 1.0f / 2.4f) - 0.055f;
}
static uint8_t sat_u8(float v) {  // Rust `as u8`: saturating, NaN -> 0
  if (!(v > 0.0f)) return 0;
  if (v >= 255.0f) return 255;
  return (uint8_t)v;
}
static uint8_t rgb8_byte(float v) {  // to_rgb8 of one averaged channel, main.rs:1785-1792
  float r = std::round(255.0f * gamma_correct(v));
  return sat_u8(std::fmin(std::fmax(r, 0.0f), 255.0f));
}
void rene_to_rgb8(const float* sums, size_t n_floats, uint32_t n_samples, uint8_t* out) {
  const float denom = (float)n_samples;
  for (size_t i = 0; i < n_floats; ++i) out[i] = rgb8_byte(sums[i] / denom);  // average, main.rs:1758-1764
}
// The sRGB thresholds of the device transform (kernels_output.hip): T[k] = the smallest float rgb8_byte maps to k + 1 or more, by bisection over the
// bit patterns of the non-negative floats up to 1.0f -- the order of the patterns is the order of the floats, and rgb8_byte is monotone over them
// (selftest/output_table_check.cpp walks every one).  Once per process.
static const float* output_threshold_table() {
  static const std::array<float, 255> table = [] {
    std::array<float, 255> t{};
    auto at = [](uint32_t bits) {
      float v;
      std::memcpy(&v, &bits, sizeof(v));
      return v;
    };
    for (uint32_t k = 0; k < 255u; ++k) {
      uint32_t lo = 0u, hi = 0x3f800000u;  // rgb8_byte(+0) = 0 < k + 1 <= 255 = rgb8_byte(1)
      while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (rgb8_byte(at(mid)) >= k + 1u) hi = mid;
        else lo = mid;
      }
      t[k] = at(hi);
    }
    return t;
  }();
  return table.data();
}
void rene_output_thresholds(float out[255]) {
  if (out) std::memcpy(out, output_threshold_table(), 255 * sizeof(float));
}

// ---- tone-mapped output and the luminance histogram on the host (include/rene_hip.h): the arithmetic of kernels_tonemap.hip / output_pixel.h and
// kernels_luminance.hip, operation by operation.  Every intermediate is a named float, and nothing may be fused into a multiply-add
// (this unit's flags allow contraction: the two functions that multiply and add switch it off).
static float lum3(float r, float g, float b) {  // chain_pass.h
#pragma clang fp contract(off)
  return (0.2126f * r + 0.7152f * g) + 0.0722f * b;
}
static void tonemap_pixel(uint32_t op, const float v[3], float scale, float w2, float c[3]) {
#pragma clang fp contract(off)
  const float e[3] = {v[0] * scale, v[1] * scale, v[2] * scale};
  if (op == RENE_TONEMAP_REINHARD) {
    const float l = std::fmin(std::fmax(lum3(e[0], e[1], e[2]), 0.0f), FLT_MAX);
    const float q = l / w2;
    const float a = 1.0f + q;
    const float b = 1.0f + l;
    const float f = a / b;
    for (int k = 0; k < 3; ++k) c[k] = e[k] * f;
  } else if (op == RENE_TONEMAP_ACES) {
    for (int k = 0; k < 3; ++k) {
      const float x = std::fmin(std::fmax(e[k], 0.0f), 16777216.0f);
      const float t0 = 2.51f * x, t1 = t0 + 0.03f, n = x * t1;
      const float u0 = 2.43f * x, u1 = u0 + 0.59f, u2 = x * u1, d = u2 + 0.14f;
      c[k] = n / d;
    }
  } else {
    for (int k = 0; k < 3; ++k) c[k] = e[k];
  }
}
int rene_tonemap_rgb8(const float* means, size_t n_pixels, int channels, uint32_t op, float scale, float white, uint8_t* out) {
  if (n_pixels && (!means || !out)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_tonemap_rgb8: NULL argument");
  if (channels != 3 && channels != 4) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_tonemap_rgb8: channels must be 3 or 4");
  if (int rc = check_tonemap("rene_tonemap_rgb8", op, scale, white); rc != RENE_OK) return rc;
  const float w2 = white * white;
  const float* T = output_threshold_table();
  for (size_t i = 0; i < n_pixels; ++i) {
    float c[3];
    tonemap_pixel(op, means + (size_t)channels * i, scale, w2, c);
    // the byte: the thresholds at or below the value (a NaN is at or above none), which is rgb8_byte (selftest/output_table_check.cpp)
    for (int k = 0; k < 3; ++k) out[3 * i + k] = (uint8_t)(std::upper_bound(T, T + 255, c[k], [](float v, float t) { return !(v >= t); }) - T);
  }
  return RENE_OK;
}
static uint32_t luminance_bin(float l) {  // l > 0
  uint32_t bits;
  std::memcpy(&bits, &l, sizeof(bits));
  return (uint32_t)std::min(std::max((int)(bits >> 20) - 856, 0), RENE_LUMINANCE_BINS - 1);
}
int rene_luminance_histogram_host(const float* means, size_t n_pixels, int channels, rene_luminance_stats* out) {
  if (!out || (n_pixels && !means)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_luminance_histogram_host: NULL argument");
  if (channels != 3 && channels != 4) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_luminance_histogram_host: channels must be 3 or 4");
  if (n_pixels > 0xffffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_luminance_histogram_host: more than 2^32 - 1 pixels");
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->n_pixels = (uint32_t)n_pixels;
  for (size_t i = 0; i < n_pixels; ++i) {
    const float* v = means + (size_t)channels * i;
    const float l = lum3(v[0], v[1], v[2]);
    if (l > 0.0f) ++out->counts[luminance_bin(l)];
    else ++out->n_dark;
  }
  return RENE_OK;
}
static bool stats_ok(const rene_luminance_stats* s) { return s && s->struct_size == sizeof(*s); }
int rene_luminance_combine(const rene_luminance_stats* parts, size_t n, rene_luminance_stats* out) {
  if (!out || (n && !parts)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_luminance_combine: NULL argument");
  uint64_t sums[RENE_LUMINANCE_BINS + 2] = {};
  for (size_t i = 0; i < n; ++i) {
    if (!stats_ok(parts + i)) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_luminance_stats.struct_size mismatch (ABI skew)");
    for (int b = 0; b < RENE_LUMINANCE_BINS; ++b) sums[b] += parts[i].counts[b];
    sums[RENE_LUMINANCE_BINS] += parts[i].n_dark;
    sums[RENE_LUMINANCE_BINS + 1] += parts[i].n_pixels;
  }
  for (uint64_t s : sums)
    if (s > 0xffffffffull) return fail(RENE_ERR_INVALID_ARGUMENT, "rene_luminance_combine: a sum exceeds 2^32 - 1");
  out->struct_size = sizeof(*out);
  for (int b = 0; b < RENE_LUMINANCE_BINS; ++b) out->counts[b] = (uint32_t)sums[b];
  out->n_dark = (uint32_t)sums[RENE_LUMINANCE_BINS];
  out->n_pixels = (uint32_t)sums[RENE_LUMINANCE_BINS + 1];
  return RENE_OK;
}
static uint64_t luminance_n_lit(const rene_luminance_stats* s) {
  uint64_t n = 0;
  for (uint32_t c : s->counts) n += c;
  return n;
}
uint32_t rene_luminance_mean_bin_x256(const rene_luminance_stats* s) {
  if (!stats_ok(s)) return 0;
  const uint64_t n_lit = luminance_n_lit(s);
  if (n_lit == 0) return 0;
  uint64_t w = 0;  // (at most 2^32 x 511 per bin)
  for (uint64_t b = 0; b < RENE_LUMINANCE_BINS; ++b) w += (uint64_t)s->counts[b] * (2 * b + 1);
  return (uint32_t)(w * 128 / n_lit);
}
int rene_luminance_percentile_bin(const rene_luminance_stats* s, uint32_t per_mille) {
  if (!stats_ok(s)) return -1;
  const uint64_t n_lit = luminance_n_lit(s);
  if (n_lit == 0) return -1;
  const uint64_t need = (n_lit * std::min(per_mille, 1000u) + 999) / 1000;
  uint64_t run = 0;
  for (int b = 0; b < RENE_LUMINANCE_BINS; ++b) {
    run += s->counts[b];
    if (run >= need) return b;
  }
  return RENE_LUMINANCE_BINS - 1;
}
int rene_auto_exposure_e8(const rene_luminance_stats* s, int key_e8) {
  if (!stats_ok(s) || luminance_n_lit(s) == 0) return 0;
  const int64_t e8 = (int64_t)key_e8 + 160 - (int64_t)((rene_luminance_mean_bin_x256(s) + 128u) >> 8);
  return (int)std::min<int64_t>(std::max<int64_t>(e8, RENE_EXPOSURE_E8_MIN), RENE_EXPOSURE_E8_MAX);
}
float rene_exposure_scale(int e8) {
  static const float M[8] = RENE_EXPOSURE_MANTISSAS;
  e8 = std::min(std::max(e8, RENE_EXPOSURE_E8_MIN), RENE_EXPOSURE_E8_MAX);
  const int k = ((e8 % 8) + 8) % 8;  // e8 mod 8 and floor(e8 / 8), whatever the sign
  return std::ldexp(M[k], (e8 - k) / 8);
}
void rene_to_aov8(const float* sums, size_t n_floats, uint32_t n_samples, int is_normal, uint8_t* out) {
  const float denom = (float)n_samples;
  for (size_t i = 0; i < n_floats; ++i) {
    float v = sums[i] / denom;
    if (is_normal) v = v * 0.5f + 0.5f;                                 // to_aov_normal, main.rs:1803-1810
    out[i] = sat_u8(256.0f * std::fmin(std::fmax(v, 0.0f), 0.999f));  // to_aov, main.rs:1794-1801
  }
}

int rene_scene_pack_info(const rene_scene_desc* scene, rene_pack_info* out) { return guarded([&] { return rene_scene_pack_info_impl(scene, out); }); }
int rene_scene_small_items(const rene_scene_desc* scene, int which, float* out, uint32_t cap_items, uint32_t* n_loop, uint32_t* n_total) {
  return guarded([&] { return rene_scene_small_items_impl(scene, which, out, cap_items, n_loop, n_total); });
}
int rene_plan_memory(const rene_scene_desc* scene, const rene_opts* opts, rene_memory_plan* out) { return guarded([&] { return rene_plan_memory_impl(scene, opts, out); }); }
int rene_create(const rene_scene_desc* scene, const rene_opts* opts, rene_ctx** out) { return guarded([&] { return rene_create_impl(scene, opts, out); }); }
int rene_render(rene_ctx* c, uint32_t first_frame, uint32_t n_frames) { return guarded([&] { return rene_render_impl(c, first_frame, n_frames); }); }
int rene_download(rene_ctx* c, int layer, int channels, float* dst, size_t dst_floats) { return guarded([&] { return rene_download_impl(c, layer, channels, dst, dst_floats); }); }
int rene_estimate_noise(rene_ctx* c, const rene_noise_params* params, rene_noise_estimate* out) { return guarded([&] { return rene_estimate_noise_impl(c, params, out); }); }
int rene_set_active_tiles(rene_ctx* c, const uint8_t* active, size_t n) { return guarded([&] { return rene_set_active_tiles_impl(c, active, n); }); }
int rene_tile_frames(rene_ctx* c, uint32_t* dst, size_t n) { return guarded([&] { return rene_tile_frames_impl(c, dst, n); }); }
int rene_download_mean(rene_ctx* c, int layer, int channels, float* dst, size_t dst_floats) { return guarded([&] { return rene_download_mean_impl(c, layer, channels, dst, dst_floats); }); }
int rene_noise_select_tiles(const rene_noise_tile* tiles, const uint8_t* active_in, uint32_t tiles_x, uint32_t tiles_y, float luminance_floor, double target, uint32_t dilate,
                            uint8_t* active_out) {
  return guarded([&] { return rene_noise_select_tiles_impl(tiles, active_in, tiles_x, tiles_y, luminance_floor, target, dilate, active_out); });
}
int rene_download_noise_tiles(rene_ctx* c, rene_noise_tile* dst, size_t n) { return guarded([&] { return rene_download_noise_tiles_impl(c, dst, n); }); }
int rene_resolve_robust(rene_ctx* c, const rene_robust_params* params, rene_robust_summary* out) { return guarded([&] { return rene_resolve_robust_impl(c, params, out); }); }
int rene_download_robust(rene_ctx* c, int what, int channels, float* dst, size_t dst_floats) { return guarded([&] { return rene_download_robust_impl(c, what, channels, dst, dst_floats); }); }
int rene_export_features(rene_ctx* c, const rene_feature_params* params, void* device_dst, size_t dst_bytes) { return guarded([&] { return rene_export_features_impl(c, params, device_dst, dst_bytes); }); }
int rene_features_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) { return guarded([&] { return result_buffer("rene_features_buffer", c, &rene_ctx::features, kNoFeatures, device_ptr, n_bytes); }); }
int rene_download_features(rene_ctx* c, void* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_features", c, &rene_ctx::features, kNoFeatures, "destination too small", false, dst, dst_bytes); });
}
int rene_output_8bit(rene_ctx* c, const rene_output_params* params, void* device_dst, size_t dst_bytes) { return guarded([&] { return rene_output_8bit_impl(c, params, device_dst, dst_bytes); }); }
int rene_output_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) { return guarded([&] { return result_buffer("rene_output_buffer", c, &rene_ctx::out, kNoOutput, device_ptr, n_bytes); }); }
int rene_download_output(rene_ctx* c, uint8_t* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_output", c, &rene_ctx::out, kNoOutput, "destination too small", true, dst, dst_bytes); });
}
int rene_output_probe(int device, int transform, size_t n, const float* v, uint8_t* out) { return guarded([&] { return rene_output_probe_impl(device, transform, n, v, out); }); }
int rene_output_tonemapped(rene_ctx* c, const rene_tonemap_params* params, void* device_dst, size_t dst_bytes) { return guarded([&] { return rene_output_tonemapped_impl(c, params, device_dst, dst_bytes); }); }
int rene_luminance_histogram(rene_ctx* c, uint32_t source, rene_luminance_stats* out) { return guarded([&] { return rene_luminance_histogram_impl(c, source, out); }); }
int rene_tonemap_probe(int device, uint32_t op, float scale, float white, size_t n, const float* rgb, uint8_t* out) { return guarded([&] { return rene_tonemap_probe_impl(device, op, scale, white, n, rgb, out); }); }
int rene_gbuffer(rene_ctx* c, const rene_gbuffer_params* params, void* device_dst, size_t dst_bytes) { return guarded([&] { return rene_gbuffer_impl(c, params, device_dst, dst_bytes); }); }
int rene_gbuffer_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) { return guarded([&] { return result_buffer("rene_gbuffer_buffer", c, &rene_ctx::gbuf, kNoGbuffer, device_ptr, n_bytes); }); }
int rene_download_gbuffer(rene_ctx* c, void* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_gbuffer", c, &rene_ctx::gbuf, kNoGbuffer, "destination too small", true, dst, dst_bytes); });
}
int rene_exr_layout(uint32_t width, uint32_t height, uint32_t layers, size_t* header_bytes, size_t* body_bytes, uint32_t* bytes_per_pixel) {
  return guarded([&] { return rene_exr_layout_impl(width, height, layers, header_bytes, body_bytes, bytes_per_pixel); });
}
int rene_exr_header(uint32_t width, uint32_t height, uint32_t layers, void* dst, size_t dst_bytes) { return guarded([&] { return rene_exr_header_impl(width, height, layers, dst, dst_bytes); }); }
int rene_exr_body_host(uint32_t width, uint32_t height, uint32_t layers, const rene_exr_planes* planes, void* dst, size_t dst_bytes) {
  return guarded([&] { return rene_exr_body_host_impl(width, height, layers, planes, dst, dst_bytes); });
}
int rene_output_exr(rene_ctx* c, const rene_exr_params* params, void* device_dst, size_t dst_bytes) { return guarded([&] { return rene_output_exr_impl(c, params, device_dst, dst_bytes); }); }
int rene_exr_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) { return guarded([&] { return result_buffer("rene_exr_buffer", c, &rene_ctx::exr, kNoExr, device_ptr, n_bytes); }); }
int rene_download_exr(rene_ctx* c, void* dst, size_t dst_bytes) {
  // (straight into the caller's pages, like the feature tensor: a body is tens of megabytes)
  return guarded([&] { return result_download("rene_download_exr", c, &rene_ctx::exr, kNoExr, "destination too small", false, dst, dst_bytes); });
}
int rene_write_exr(rene_ctx* c, const rene_exr_params* params, const char* path) { return guarded([&] { return rene_write_exr_impl(c, params, path); }); }
size_t rene_exr_tail_bound(uint32_t width, uint32_t height, uint32_t layers) { return rene_exr_tail_bound_impl(width, height, layers); }
int rene_exr_attributes(uint32_t width, uint32_t height, uint32_t layers, uint32_t compression, void* dst, size_t dst_bytes) {
  return guarded([&] { return rene_exr_attributes_impl(width, height, layers, compression, dst, dst_bytes); });
}
int rene_exr_compress_host(uint32_t width, uint32_t height, uint32_t layers, uint32_t compression, const void* body, size_t body_bytes, void* dst, size_t dst_bytes,
                           size_t* written) {
  return guarded([&] { return rene_exr_compress_host_impl(width, height, layers, compression, body, body_bytes, dst, dst_bytes, written); });
}
int rene_exr_compress(rene_ctx* c, uint32_t width, uint32_t height, uint32_t layers, uint32_t compression, const void* device_body, size_t body_bytes, void* device_dst,
                      size_t dst_bytes, size_t* written) {
  return guarded([&] { return rene_exr_compress_impl(c, width, height, layers, compression, device_body, body_bytes, device_dst, dst_bytes, written); });
}
int rene_exr_tail_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) {
  return guarded([&] { return result_buffer("rene_exr_tail_buffer", c, &rene_ctx::exr_tail, kNoExrTail, device_ptr, n_bytes); });
}
int rene_download_exr_tail(rene_ctx* c, void* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_exr_tail", c, &rene_ctx::exr_tail, kNoExrTail, "destination too small", false, dst, dst_bytes); });
}
int rene_output_exr_compressed(rene_ctx* c, const rene_exr_params* params, uint32_t compression, void* device_dst, size_t dst_bytes, size_t* written) {
  return guarded([&] { return rene_output_exr_compressed_impl(c, params, compression, device_dst, dst_bytes, written); });
}
int rene_exr_compress_rows_host(uint32_t row_bytes, uint32_t height, size_t attributes_bytes, uint32_t compression, const void* body, size_t body_bytes, void* dst,
                                size_t dst_bytes, size_t* written) {
  return guarded([&] { return rene_exr_compress_rows_host_impl(row_bytes, height, attributes_bytes, compression, body, body_bytes, dst, dst_bytes, written); });
}
int rene_exr_compress_rows(rene_ctx* c, uint32_t row_bytes, uint32_t height, size_t attributes_bytes, uint32_t compression, const void* device_body, size_t body_bytes,
                           void* device_dst, size_t dst_bytes, size_t* written) {
  return guarded([&] { return rene_exr_compress_rows_impl(c, row_bytes, height, attributes_bytes, compression, device_body, body_bytes, device_dst, dst_bytes, written); });
}
uint32_t rene_cryptomatte_hash(const char* utf8, size_t n) { return utf8 || n == 0 ? cryptomatte_hash(utf8 ? utf8 : "", n) : 0u; }
int rene_cryptomatte_manifest(const char* const* names, uint32_t n_names, char* dst, size_t dst_bytes, size_t* written) {
  return guarded([&] { return rene_cryptomatte_manifest_impl(names, n_names, dst, dst_bytes, written); });
}
int rene_cryptomatte_layout(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers, size_t* attributes_bytes, size_t* body_bytes,
                            uint32_t* bytes_per_pixel) {
  return guarded([&] { return rene_cryptomatte_layout_impl(width, height, layers, n_layers, attributes_bytes, body_bytes, bytes_per_pixel); });
}
int rene_cryptomatte_attributes(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers, uint32_t compression, void* dst, size_t dst_bytes) {
  return guarded([&] { return rene_cryptomatte_attributes_impl(width, height, layers, n_layers, compression, dst, dst_bytes); });
}
int rene_cryptomatte_body_host(uint32_t width, uint32_t height, const rene_cryptomatte_layer* layers, uint32_t n_layers, const rene_gbuffer_pixel* const* host_records,
                               void* dst, size_t dst_bytes) {
  return guarded([&] { return rene_cryptomatte_body_host_impl(width, height, layers, n_layers, host_records, dst, dst_bytes); });
}
int rene_output_cryptomatte(rene_ctx* c, const rene_cryptomatte_params* params, void* device_dst, size_t dst_bytes) {
  return guarded([&] { return rene_output_cryptomatte_impl(c, params, device_dst, dst_bytes); });
}
int rene_cryptomatte_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) {
  return guarded([&] { return result_buffer("rene_cryptomatte_buffer", c, &rene_ctx::cryptomatte, kNoCryptomatte, device_ptr, n_bytes); });
}
int rene_download_cryptomatte(rene_ctx* c, void* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_cryptomatte", c, &rene_ctx::cryptomatte, kNoCryptomatte, "destination too small", false, dst, dst_bytes); });
}
int rene_write_cryptomatte(rene_ctx* c, const rene_cryptomatte_params* params, uint32_t compression, const char* path) {
  return guarded([&] { return rene_write_cryptomatte_impl(c, params, compression, path); });
}
int rene_exr_passes_layout(uint32_t width, uint32_t height, const rene_exr_passes_params* params, size_t* attributes_bytes, size_t* body_bytes, uint32_t* bytes_per_pixel) {
  return guarded([&] { return rene_exr_passes_layout_impl(width, height, params, attributes_bytes, body_bytes, bytes_per_pixel); });
}
int rene_exr_passes_attributes(uint32_t width, uint32_t height, const rene_exr_passes_params* params, uint32_t compression, void* dst, size_t dst_bytes) {
  return guarded([&] { return rene_exr_passes_attributes_impl(width, height, params, compression, dst, dst_bytes); });
}
int rene_exr_passes_body_host(uint32_t width, uint32_t height, const rene_exr_passes_params* params, const float* beauty_sum, void* dst, size_t dst_bytes) {
  return guarded([&] { return rene_exr_passes_body_host_impl(width, height, params, beauty_sum, dst, dst_bytes); });
}
int rene_output_exr_passes(rene_ctx* c, const rene_exr_passes_params* params, void* device_dst, size_t dst_bytes) {
  return guarded([&] { return rene_output_exr_passes_impl(c, params, device_dst, dst_bytes); });
}
int rene_exr_passes_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) {
  return guarded([&] { return result_buffer("rene_exr_passes_buffer", c, &rene_ctx::exr_passes, kNoExrPasses, device_ptr, n_bytes); });
}
int rene_download_exr_passes(rene_ctx* c, void* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_exr_passes", c, &rene_ctx::exr_passes, kNoExrPasses, "destination too small", false, dst, dst_bytes); });
}
int rene_write_exr_passes(rene_ctx* c, const rene_exr_passes_params* params, uint32_t compression, const char* path) {
  return guarded([&] { return rene_write_exr_passes_impl(c, params, compression, path); });
}
int rene_write_exr_compressed(rene_ctx* c, const rene_exr_params* params, uint32_t compression, const char* path) {
  return guarded([&] { return rene_write_exr_compressed_impl(c, params, compression, path); });
}
int rene_primary_hits(rene_ctx* c, uint32_t first_frame, uint32_t n_frames, rene_primary_hit* host_dst, size_t n) { return guarded([&] { return rene_primary_hits_impl(c, first_frame, n_frames, host_dst, n); }); }
int rene_occlusion(rene_ctx* c, const rene_occlusion_params* params, void* device_dst, size_t dst_bytes) { return guarded([&] { return rene_occlusion_impl(c, params, device_dst, dst_bytes); }); }
int rene_occlusion_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) { return guarded([&] { return result_buffer("rene_occlusion_buffer", c, &rene_ctx::occl, kNoOcclusion, device_ptr, n_bytes); }); }
int rene_download_occlusion(rene_ctx* c, void* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_occlusion", c, &rene_ctx::occl, kNoOcclusion, "destination too small", true, dst, dst_bytes); });
}
int rene_occlusion_samples(rene_ctx* c, const rene_occlusion_params* params, rene_occlusion_sample* host_dst, size_t n) { return guarded([&] { return rene_occlusion_samples_impl(c, params, host_dst, n); }); }
int rene_direct(rene_ctx* c, const rene_direct_params* params, void* device_dst, size_t dst_bytes) { return guarded([&] { return rene_direct_impl(c, params, device_dst, dst_bytes); }); }
int rene_direct_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) { return guarded([&] { return result_buffer("rene_direct_buffer", c, &rene_ctx::direct, kNoDirect, device_ptr, n_bytes); }); }
int rene_download_direct(rene_ctx* c, void* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_direct", c, &rene_ctx::direct, kNoDirect, "destination too small", true, dst, dst_bytes); });
}
int rene_direct_samples(rene_ctx* c, const rene_direct_params* params, rene_direct_sample* host_dst, size_t n) { return guarded([&] { return rene_direct_samples_impl(c, params, host_dst, n); }); }
int rene_bounces(rene_ctx* c, const rene_bounces_params* params, void* device_dst, size_t dst_bytes) { return guarded([&] { return rene_bounces_impl(c, params, device_dst, dst_bytes); }); }
int rene_bounces_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) { return guarded([&] { return result_buffer("rene_bounces_buffer", c, &rene_ctx::bounces, kNoBounces, device_ptr, n_bytes); }); }
int rene_download_bounces(rene_ctx* c, void* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_bounces", c, &rene_ctx::bounces, kNoBounces, "destination too small", true, dst, dst_bytes); });
}
int rene_bounces_samples(rene_ctx* c, const rene_bounces_params* params, rene_bounces_sample* host_dst, size_t n) { return guarded([&] { return rene_bounces_samples_impl(c, params, host_dst, n); }); }
int rene_lights_default_groups(rene_ctx* c, uint8_t* instance_group, uint32_t n_instances, uint8_t* distant_group, uint32_t n_distant, uint8_t* background_group,
                               uint32_t* n_used) {
  return guarded([&] { return rene_lights_default_groups_impl(c, instance_group, n_instances, distant_group, n_distant, background_group, n_used); });
}
int rene_lights(rene_ctx* c, const rene_lights_params* params, void* device_dst, size_t dst_bytes) { return guarded([&] { return rene_lights_impl(c, params, device_dst, dst_bytes); }); }
int rene_lights_buffer(rene_ctx* c, void** device_ptr, size_t* n_bytes) { return guarded([&] { return result_buffer("rene_lights_buffer", c, &rene_ctx::lights, kNoLights, device_ptr, n_bytes); }); }
int rene_download_lights(rene_ctx* c, void* dst, size_t dst_bytes) {
  return guarded([&] { return result_download("rene_download_lights", c, &rene_ctx::lights, kNoLights, "destination too small", true, dst, dst_bytes); });
}
int rene_lights_samples(rene_ctx* c, const rene_lights_params* params, rene_lights_sample* host_dst, size_t n) { return guarded([&] { return rene_lights_samples_impl(c, params, host_dst, n); }); }
int rene_download_robust_tiles(rene_ctx* c, rene_robust_tile* dst, size_t n) { return guarded([&] { return rene_download_robust_tiles_impl(c, dst, n); }); }
int rene_load_chains(rene_ctx* c, const float* chains, size_t n_floats, uint32_t first_frame, uint32_t n_frames, const uint32_t* tile_frames, size_t n_tiles) {
  return guarded([&] { return rene_load_chains_impl(c, chains, n_floats, first_frame, n_frames, tile_frames, n_tiles); });
}
int rene_save_state(rene_ctx* c, const rene_state_params* params, void* dst, size_t dst_bytes, size_t* written) { return guarded([&] { return rene_save_state_impl(c, params, dst, dst_bytes, written); }); }
int rene_restore_state(rene_ctx* c, const rene_state_params* params, const void* const* parts, const size_t* part_bytes, size_t n_parts) {
  return guarded([&] { return rene_restore_state_impl(c, params, parts, part_bytes, n_parts); });
}
int rene_state_inspect(const void* blob, size_t bytes, rene_state_info* out) { return guarded([&] { return rene_state_inspect_impl(blob, bytes, out); }); }
int rene_state_tiles(const void* blob, size_t bytes, rene_state_tile* dst, size_t n) { return guarded([&] { return rene_state_tiles_impl(blob, bytes, dst, n); }); }
int rene_state_verify(const void* blob, size_t bytes) { return guarded([&] { return rene_state_verify_impl(blob, bytes); }); }
int rene_state_inspect_file(const char* path, rene_state_info* out, rene_state_tile* tiles, size_t n) { return guarded([&] { return rene_state_inspect_file_impl(path, out, tiles, n); }); }
int rene_save_state_file(rene_ctx* c, const rene_state_params* params, const char* path) { return guarded([&] { return rene_save_state_file_impl(c, params, path); }); }
int rene_restore_state_files(rene_ctx* c, const rene_state_params* params, const char* const* paths, size_t n_paths) {
  return guarded([&] { return rene_restore_state_files_impl(c, params, paths, n_paths); });
}
int rene_denoise_shard_prepare(rene_ctx* c, const rene_denoise_params* params) { return guarded([&] { return rene_denoise_shard_prepare_impl(c, params); }); }
int rene_denoise_place_shard(rene_ctx* c, const void* src, size_t bytes) { return guarded([&] { return rene_denoise_place_shard_impl(c, src, bytes); }); }
int rene_denoise_placed(rene_ctx* c) { return guarded([&] { return rene_denoise_placed_impl(c); }); }
int rene_download_denoised(rene_ctx* c, int what, int channels, float* dst, size_t dst_floats) { return guarded([&] { return rene_download_denoised_impl(c, what, channels, dst, dst_floats); }); }
}  // extern "C"
