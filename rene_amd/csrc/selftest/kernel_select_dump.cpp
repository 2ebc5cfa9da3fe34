// kernel_select_dump -- prints what kernel_select.h decides for the cases on its standard input, one line per case:
//   in:  <features> <flags> <n_nodes> <stack_depth> <n_insts> <lights_len> <small_bytes> <RENE_NO_LDS_TABLES set: 0 | 1>
//   out: <the kernel's mangled name, as <unit>.res and the launch log print it> family=<item|while|restart> shade=<matte|single|multi>
//        lds=<bytes> lds_insts=<n> stack_entries=<0 | 1> reads_frame_stream=<0 | 1>
// tests/test_kernel_select.py compares the output with tests/kernel_matrix.py's restatement over every input of the selection.
//   kernel_select_dump <block size of the render kernels>
#include "../kernel_select.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char** argv) {
  if (argc != 2 || std::atoi(argv[1]) < 64) {
    std::fprintf(stderr, "usage: kernel_select_dump <block size of the render kernels> < cases\n");
    return 2;
  }
  rene::SelectInputs in{};
  in.block = (uint32_t)std::atoi(argv[1]);
  unsigned no_tables = 0;
  int n;
  while ((n = std::scanf("%u %u %u %u %u %u %u %u", &in.features, &in.flags, &in.n_nodes, &in.stack_depth, &in.n_insts, &in.lights_len, &in.small_bytes, &no_tables)) == 8) {
    in.no_lds_tables = no_tables != 0;
    const rene::KernelChoice k = rene::select_kernel(in);
    const bool wf = k.family == rene::KernelFamily::Restart;
    const std::string fn = wf ? "render_kernel_wf" : "render_kernel";  // the Itanium name of rene::<fn><feat, maxl, count, aov[, tables]>(SceneView, RenderParams)
    std::string args = "Lj" + std::to_string(k.feat) + "ELi" + std::to_string(k.maxl) + "ELb" + std::to_string((int)k.count) + "ELb" + std::to_string((int)k.aov) + "E";
    if (wf) args += "Lb" + std::to_string((int)k.tables) + "E";
    else if (k.tables) args += "?";  // (no such render_kernel: not a name)
    static const char* const family[] = {"item", "while", "restart"};
    static const char* const shade[] = {"matte", "single", "multi"};
    std::printf("_ZN4rene%zu%sI%sEEvNS_9SceneViewENS_12RenderParamsE family=%s shade=%s lds=%zu lds_insts=%u stack_entries=%d reads_frame_stream=%d\n", fn.size(), fn.c_str(),
                args.c_str(), family[(int)k.family], shade[(int)k.shade], k.lds, k.lds_insts, (int)k.stack_entries, (int)k.reads_frame_stream);
  }
  if (n != EOF) {
    std::fprintf(stderr, "kernel_select_dump: a case needs eight unsigned integers\n");
    return 2;
  }
  return 0;
}
