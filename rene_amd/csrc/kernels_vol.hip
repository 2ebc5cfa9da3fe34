// kernels_vol.hip -- render kernels of the volumetric integrator (Integrator "volpath", lib.rs:477-803):
// render_kernel with FEAT_VOLPATH over the item loop (small scenes) or the while-while BVH traversal (shallow trees), and
// render_kernel_wf with FEAT_VOLPATH (deep trees: traversal restart, its walks -- tr / tr_emit -- as phases of the state machine).
// Separate translation unit so that it compiles in parallel with the path-integrator families; kernels.hip launches what this unit instantiates.
#include "device_code.inc"  // opens namespace rene

RenderKernel vol_render_kernel(const KernelChoice& k) {  // every leaf of the integrator, once
  constexpr uint32_t MATTE = FEAT_LIGHTS | FEAT_VOLPATH, GEN1 = shade_feat(ShadeClass::Single) | FEAT_VOLPATH, ALL = FEAT_ALL | FEAT_VOLPATH;
  return find_leaf<MATTE, MATTE | FEAT_SMALL, GEN1, GEN1 | FEAT_SMALL, ALL, ALL | FEAT_SMALL>(k);
}

}  // namespace rene
