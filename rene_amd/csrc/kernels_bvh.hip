// kernels_bvh.hip -- the BVH family of render kernels: the traversal-restart state machine (render_kernel_wf, render_wf.inc) and, for shallow
// trees and A/B tests (RENE_FLAG_NO_RESTART), the plain while-while kernel.  Separate translation unit so that it compiles in parallel with
// kernels.hip, which launches what this unit instantiates.
#include "device_code.inc"  // opens namespace rene

RenderKernel bvh_render_kernel(const KernelChoice& k) {  // every leaf of the family, once
  constexpr uint32_t GEN = FEAT_GENERAL_BSDF | FEAT_TEXTURES | FEAT_BACKGROUND, SUB = GEN | FEAT_NO_SPECULAR | FEAT_NO_MICROFACET;
  // (FEAT_NO_EMITTERS: dragon-class, distant lights only, and the teapot scenes, an environment light only)
  return find_leaf<FEAT_LIGHTS, FEAT_LIGHTS | FEAT_NO_EMITTERS, SUB, SUB | FEAT_NO_EMITTERS, GEN, shade_feat(ShadeClass::Single), FEAT_ALL>(k);
}

}  // namespace rene
