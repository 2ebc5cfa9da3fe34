// exr_store.h -- the one store the OpenEXR packs share (kernels_exr.hip, kernels_exr_passes.hip): a 4-byte value at an even address of a chunk.
#pragma once
#include <hip/hip_runtime.h>

namespace rene {

// a 4-byte value at an even address: one dword where the address is a multiple of 4, else its two halves, each a store of its own (through a
// volatile access, because the backend otherwise joins the two into the one unaligned dword store this target would let it issue)
__device__ __forceinline__ void store_word(uint8_t* p, uint32_t v, bool aligned) {
  if (aligned) {
    *reinterpret_cast<uint32_t*>(p) = v;
  } else {
    using GlobalHalfWord = volatile __attribute__((address_space(1))) uint16_t;  // (global memory: a volatile generic access would be a flat store)
    GlobalHalfWord* h = (GlobalHalfWord*)reinterpret_cast<uintptr_t>(p);
    h[0] = (uint16_t)v;
    h[1] = (uint16_t)(v >> 16);
  }
}

}  // namespace rene
