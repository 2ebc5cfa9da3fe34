// result_refusals_check -- host only, no GPU: the calls that hand out a library-owned result, refused before a context is looked at, with the words
// tests/test_result_buffers_host.py pins.  It exists to be built with the host code under a sanitizer (`make selftest/result_refusals_asan` links it
// with rene_hip.cpp compiled with -fsanitize=address,undefined) and run as a program of its own.  Exit status 0 and "ok ..." on success.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../../include/rene_hip.h"

namespace {
int failures = 0;
void refused(const char* fn, int rc, const char* what) {
  const std::string want = std::string(fn) + ": " + what;
  if (rc == RENE_ERR_INVALID_ARGUMENT && want == rene_last_error()) return;
  std::fprintf(stderr, "%s: status %d, \"%s\"; expected %d, \"%s\"\n", fn, rc, rene_last_error(), (int)RENE_ERR_INVALID_ARGUMENT, want.c_str());
  ++failures;
}
}  // namespace

int main() {
  void* ptr = nullptr;
  size_t n = 0;
  unsigned char dst[64];
  std::memset(dst, 0xAB, sizeof dst);
  using Getter = int (*)(rene_ctx*, void**, size_t*);
  const struct { const char* fn; Getter get; } getters[] = {{"rene_features_buffer", rene_features_buffer}, {"rene_output_buffer", rene_output_buffer},
                                                           {"rene_gbuffer_buffer", rene_gbuffer_buffer}, {"rene_denoise_shard_buffer", rene_denoise_shard_buffer}};
  for (const auto& g : getters) {
    refused(g.fn, g.get(nullptr, &ptr, &n), "NULL argument");
    refused(g.fn, g.get(nullptr, nullptr, &n), "NULL argument");
    refused(g.fn, g.get(nullptr, &ptr, nullptr), "NULL argument");
  }
  refused("rene_download_features", rene_download_features(nullptr, dst, sizeof dst), "NULL argument");
  refused("rene_download_output", rene_download_output(nullptr, dst, sizeof dst), "NULL argument");
  refused("rene_download_gbuffer", rene_download_gbuffer(nullptr, dst, sizeof dst), "NULL argument");
  refused("rene_download_denoise_shard", rene_download_denoise_shard(nullptr, dst, sizeof dst), "NULL argument");
  refused("rene_download_features", rene_download_features(nullptr, nullptr, 0), "NULL argument");
  refused("rene_download_output", rene_download_output(nullptr, nullptr, 0), "NULL argument");
  refused("rene_download_gbuffer", rene_download_gbuffer(nullptr, nullptr, 0), "NULL argument");
  refused("rene_download_denoise_shard", rene_download_denoise_shard(nullptr, nullptr, 0), "NULL argument");
  rene_feature_params fp;
  rene_feature_params_default(&fp);
  rene_output_params op;
  rene_output_params_default(&op);
  rene_tonemap_params tp;
  rene_tonemap_params_default(&tp);
  rene_gbuffer_params gp;
  rene_gbuffer_params_default(&gp);
  refused("rene_export_features", rene_export_features(nullptr, nullptr, nullptr, 0), "NULL context");
  refused("rene_export_features", rene_export_features(nullptr, &fp, dst, sizeof dst), "NULL context");
  refused("rene_output_8bit", rene_output_8bit(nullptr, nullptr, nullptr, 0), "NULL context");
  refused("rene_output_8bit", rene_output_8bit(nullptr, &op, dst, sizeof dst), "NULL context");
  refused("rene_output_tonemapped", rene_output_tonemapped(nullptr, nullptr, nullptr, 0), "NULL context");
  refused("rene_output_tonemapped", rene_output_tonemapped(nullptr, &tp, dst, sizeof dst), "NULL context");
  refused("rene_gbuffer", rene_gbuffer(nullptr, nullptr, nullptr, 0), "NULL context");
  refused("rene_gbuffer", rene_gbuffer(nullptr, &gp, dst, sizeof dst), "NULL context");
  for (unsigned char b : dst)
    if (b != 0xAB) ++failures;
  if (ptr || n) ++failures;  // a refused call writes nothing
  if (failures) return 1;
  std::printf("ok: 28 refusals without a context, every one in its call's words\n");
  return 0;
}
