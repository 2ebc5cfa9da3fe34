// kernel_select.h -- which render kernel a launch runs, on its own: the family, the leaf instantiation, its template booleans and what the launch
// sets up for it.  Host only and pure, like launch_plan.h: the launchers (kernels*.hip) map the choice to a kernel pointer, rene_hip.cpp asks what a
// context's launches need; tests/test_kernel_select.py checks every input against tests/kernel_matrix.py (selftest/kernel_select_dump.cpp).
#pragma once
#include <cstddef>

#include "../../include/rene_hip.h"
#include "device_scene.h"

namespace rene {

enum class KernelFamily { ItemLoop, WhileWhile, Restart };  // render_kernel over the wave-coherent item loop / the BVH, render_kernel_wf (render_wf.inc)
enum class ShadeClass { Matte, Single, Multi };             // Matte only (Cornell, dragon-class), general single-lobe, general multi-lobe

constexpr uint32_t FEAT_ALL = FEAT_SPHERES | FEAT_GENERAL_BSDF | FEAT_TEXTURES | FEAT_LIGHTS | FEAT_BACKGROUND | FEAT_MULTI_LOBE;
constexpr ShadeClass shade_class(uint32_t f) { return !(f & (FEAT_ALL & ~FEAT_LIGHTS)) ? ShadeClass::Matte : (f & FEAT_MULTI_LOBE) ? ShadeClass::Multi : ShadeClass::Single; }
// a class's widest leaf (the wavefront family's only one) and its lobe count
constexpr uint32_t shade_feat(ShadeClass s) { return s == ShadeClass::Matte ? FEAT_LIGHTS : s == ShadeClass::Multi ? FEAT_ALL : FEAT_ALL & ~FEAT_MULTI_LOBE; }
constexpr int shade_maxl(ShadeClass s) { return s == ShadeClass::Multi ? 5 : 1; }

struct SelectInputs {
  uint32_t features, flags;   // FEAT_* of the scene as the launchers see them (LaunchConfig::features); RENE_FLAG_COUNTERS / _NO_AOV / _NO_RESTART
  uint32_t n_nodes, stack_depth;  // nodes of the main structure; LDS traversal stack entries per lane
  uint32_t n_insts, lights_len;
  uint32_t small_bytes;       // FEAT_SMALL: the scene's LDS image
  uint32_t block;             // lanes of a workgroup (device_code.inc, BLOCK)
  bool no_lds_tables;         // RENE_NO_LDS_TABLES is set (A/B tests)
};
struct KernelChoice {
  KernelFamily family;
  ShadeClass shade;         // (what the wavefront family shades by)
  uint32_t feat;            // the instantiation: render_kernel<feat, maxl, count, aov> or render_kernel_wf<feat, maxl, count, aov, tables>
  int maxl;
  bool count, aov, tables;
  size_t lds;               // bytes of LDS in front of the launch's seed tables
  uint32_t lds_insts;       // SceneView::lds_insts
  bool stack_entries;       // RenderParams::stack_entries = stack_depth (what follows the stack in LDS starts there)
  bool reads_frame_stream;  // the kernel reads RenderParams::frame_stream: the launch needs the table, filled
};

inline KernelChoice select_kernel(const SelectInputs& in) {
  const uint32_t f = in.features;
  const bool want_count = (in.flags & RENE_FLAG_COUNTERS) != 0, want_aov = !(in.flags & RENE_FLAG_NO_AOV);
  const bool vol = (f & FEAT_VOLPATH) != 0, small = (f & FEAT_SMALL) != 0;
  KernelChoice k{};
  k.shade = shade_class(f);
  k.feat = shade_feat(k.shade);
  k.maxl = shade_maxl(k.shade);
  // a tree of a few hundred nodes is shallow and its rays stay coherent: the plain while-while loop wins there (forced-BVH Cornell 17.2 vs 10.9,
  // veach-mis 10.8 vs 6.3, zoo 5.1 vs 3.3 Grays/s); deep trees need the restart scheduling (teapot-class 4.4 vs 3.5, dragon-class 4.4 vs 2.0)
  k.family = small ? KernelFamily::ItemLoop : ((in.flags & RENE_FLAG_NO_RESTART) || in.n_nodes <= 512u) ? KernelFamily::WhileWhile : KernelFamily::Restart;
  const bool restart = k.family == KernelFamily::Restart;
  if (vol) k.feat |= FEAT_VOLPATH | (f & FEAT_SMALL);  // the volumetric integrator: the class's widest leaf in every family
  else if (small) {
    // Matte with triangle emitters only (Cornell) or with distant lights; general single-lobe scenes without textures, distant lights or a background
    // (veach-mis: Matte + Metal, sphere emitters) -- with Metal as the only general material the other lobe kinds are compiled out: 118 VGPRs, four waves
    if (k.shade == ShadeClass::Matte) k.feat = f & FEAT_LIGHTS;
    else if (k.shade == ShadeClass::Single && !(f & (FEAT_TEXTURES | FEAT_LIGHTS | FEAT_BACKGROUND)))
      k.feat = FEAT_SPHERES | FEAT_GENERAL_BSDF | ((f & FEAT_NO_SPECULAR) && (f & FEAT_NO_BLEND) ? FEAT_NO_SPECULAR | FEAT_NO_BLEND : 0u);
    k.feat |= FEAT_SMALL;
  } else {
    // dragon-class: distant lights only; general single-lobe scenes without spheres and distant lights (teapot-class: Substrate + textures + environment
    // map) -- with Substrate as the only general material, and for the teapot scenes an environment light as the only light
    if (k.shade == ShadeClass::Matte) k.feat |= f & FEAT_NO_EMITTERS;
    else if (k.shade == ShadeClass::Single && !(f & (FEAT_SPHERES | FEAT_LIGHTS))) {
      k.feat = FEAT_GENERAL_BSDF | FEAT_TEXTURES | FEAT_BACKGROUND;
      if ((f & FEAT_NO_SPECULAR) && (f & FEAT_NO_MICROFACET)) k.feat |= FEAT_NO_SPECULAR | FEAT_NO_MICROFACET | (f & FEAT_NO_EMITTERS);
    }
    if (!restart) k.feat &= ~FEAT_NO_EMITTERS;  // (the while-while loop has no instantiation of its own for that bit)
  }
  // render_kernel outside the path integrator's item loop comes in two forms only: everything or nothing
  k.aov = want_count || want_aov;
  k.count = (vol ? !restart : k.family == KernelFamily::WhileWhile) ? k.aov : want_count;
  k.lds = small ? (vol ? 0u : in.small_bytes) : (size_t)in.stack_depth * in.block * sizeof(uint32_t);
  k.stack_entries = restart;
  // the restart kernels keep the instance records and the distant lights in LDS behind the stack when that still leaves four workgroups per CU
  // (a quarter of 160 KB each): every shaded hit reads its instance, every light loop its light
  const size_t tables = (size_t)in.n_insts * sizeof(Inst) + (size_t)in.lights_len * sizeof(Light);
  k.tables = restart && !vol && !want_count && want_aov && in.n_insts && k.lds + tables <= 40u * 1024u && !in.no_lds_tables;
  k.lds_insts = k.tables ? in.n_insts : 0u;
  k.lds += k.tables ? tables : 0u;
  k.reads_frame_stream = small && !vol && k.shade == ShadeClass::Matte;  // (device_code.inc, frame_stream_feat of these two leaves)
  return k;
}

}  // namespace rene
