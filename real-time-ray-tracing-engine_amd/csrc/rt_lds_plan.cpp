// rt_lds_plan.cpp — the LDS residency planners (rt_lds_plan.h): pure integer
// functions of a kernel instance's attributes, the device's CU count, the
// scene's sizes and its tuning.  No HIP here: host/rtx_plan_check.cpp runs
// them on the CPU, tests/test_lds_plan.py pins their outcomes.
#include "rt_lds_plan.h"

#include <algorithm>

// LDS plan per block at the occupancy the instance's register count allows
// (blocks of block_waves waves over the 4 SIMDs): the bytes left for the
// staged BVH prefix after the static LDS and the traversal stacks, and whether
// those two fit at all.
RtkLdsPlan lds_plan(KernelAttrs a, int features, int stack_depth, int lds_cap) {
  const int wps = waves_per_simd(a.num_regs);
  size_t cap = kLdsPerBlock;
  if (lds_cap > 0 && (size_t)lds_cap < cap) cap = (size_t)lds_cap;
  const int bw = block_waves((unsigned)features);
  const int blocks_per_cu = std::max(1, wps * 4 / bw);
  const size_t per_block = std::min(kLdsPerCu / blocks_per_cu, cap);
  const size_t fixed = (size_t)a.static_lds + lds_bytes(features, stack_depth, 0);
  RtkLdsPlan plan;
  plan.waves_per_simd = wps;
  plan.block_budget = (int32_t)per_block;
  plan.fixed_bytes = (int32_t)fixed;
  plan.stack_fits = fixed <= per_block;
  plan.n_nodes = per_block > fixed ? (int)((per_block - fixed) / RT_LDS_NODE_BYTES(features)) : 0;
  // stacks over the share: fewer blocks per CU (no nodes are staged then)
  const int lds_blocks = fixed > 0 ? (int)(kLdsPerCu / fixed) : blocks_per_cu;
  plan.resident_waves_per_cu = std::min(blocks_per_cu, std::max(1, lds_blocks)) * bw;
  return plan;
}

Collapse4 collapse4_verdict(KernelAttrs a4, int features, int d4, int lds_cap) {
  const int stack = 3 * d4 + 1; // rtx::bvh4_stack_depth (rt_scene.h)
  if (stack > RT_STACK_DEPTH4) return COLLAPSE4_TOO_DEEP;
  return lds_plan(a4, features | RT_FEAT_BVH4, stack, lds_cap).stack_fits ? COLLAPSE4_FITS : COLLAPSE4_OVER_SHARE;
}

namespace {

// The persistent instance a scene uses and the LDS it has left for staging
// after its stacks and static LDS: blocks of kPcWaves waves (one per CU, which
// may own the CU's whole LDS) if their stacks fit, else blocks of kWaves waves
// (one per SIMD at the occupancy target: a quarter of the CU's LDS each);
// pcw 0 / free_bytes -1 when neither fits or the feature set has no
// persistent instance.
struct PcShape {
  int pcw = 0, blocks_per_cu = 0;
  int64_t free_bytes = -1;
};
PcShape persistent_shape(const LdsPlanInput &in, int force_waves) {
  PcShape r;
  if (!RT_PERSIST_F((unsigned)in.features & 63u)) return r;
  for (int w : {kPcWaves, kWaves}) { // force_waves == kWaves (tests): the 4-wave form on any scene
    if (force_waves == kWaves && w != kWaves) continue;
    const KernelAttrs a = w == kPcWaves ? in.pc16 : in.pc4;
    const int bpc = std::max(1, waves_per_simd(a.num_regs) * 4 / w); // resident blocks per CU
    const size_t per_block = kLdsPerCu / bpc;
    const size_t fixed = (size_t)a.static_lds + lds_bytes_pc(in.features, w, in.stack_depth, 0, 0, 0);
    if (fixed <= per_block) {
      r.pcw = w;
      r.blocks_per_cu = bpc;
      r.free_bytes = (int64_t)(per_block - fixed);
      return r;
    }
  }
  return r;
}

} // namespace

SceneLdsPlan plan_scene_lds(const LdsPlanInput &in, const rt_tuning &tune) {
  SceneLdsPlan r{};
  const RtkLdsPlan plan = r.render = lds_plan(in.render, in.features, in.stack_depth, tune.lds_cap);
  // the one-unit instance: the BFS prefix of the nodes sized to what the
  // instance's occupancy leaves free
  r.wave_slots = in.cus * 4 * plan.waves_per_simd;
  int budget = plan.n_nodes;
  if (!plan.stack_fits) {
    if ((size_t)plan.fixed_bytes > kLdsPerBlock) {
      r.outcome = LDS_UNSUPPORTED;
      return r;
    }
    r.outcome = LDS_STACKS_OVER_SHARE;
    budget = 0;
    r.wave_slots = in.cus * plan.resident_waves_per_cu;
  }
  // A/B experiments, within the plan (< 0: none); this also replaces the 0 of
  // stacks over the share -- by 0 again: plan.n_nodes is 0 there
  if (tune.lds_nodes != 0)
    budget = std::max(0, std::min((int)tune.lds_nodes, plan.n_nodes));
  r.n_lds_nodes = std::max(0, std::min(budget, in.n_nodes));
  // the persistent instance: its node prefix, then -- if the whole tree is
  // staged and room is left -- the world items and spheres
  const PcShape pc = persistent_shape(in, tune.pc_waves);
  r.pc_waves = pc.pcw;
  r.pc_grid = in.cus * pc.blocks_per_cu;
  const int64_t node_b = RT_LDS_NODE_BYTES(in.features);
  r.n_lds_nodes_pc = pc.free_bytes < 0 ? -1 : (int32_t)std::min<int64_t>(pc.free_bytes / node_b, in.n_nodes);
  if (tune.lds_nodes_pc != 0 && r.n_lds_nodes_pc >= 0) // A/B experiments, within what the plan leaves free
    r.n_lds_nodes_pc = (int32_t)std::max<int64_t>(
        0, std::min<int64_t>({(int64_t)tune.lds_nodes_pc, in.n_nodes, pc.free_bytes / node_b}));
  const int64_t prim_b = (int64_t)((size_t)in.n_items * sizeof(DItem) + (size_t)in.n_spheres * sizeof(DSphere));
  if (!tune.no_lds_prims && pc.free_bytes >= 0 && r.n_lds_nodes_pc == in.n_nodes &&
      pc.free_bytes - (int64_t)in.n_nodes * node_b >= prim_b && in.n_items > 0) {
    r.lds_items_pc = in.n_items;
    r.lds_spheres_pc = in.n_spheres;
  }
  // the one Perlin table of a noise scene in LDS (tune.no_lds_perlin: from
  // HBM, A/B runs and the bit-identity test); several tables stay in HBM
  r.lds_perlin = (in.features & RT_FEAT_NOISE) && in.n_perlin == 1 && !tune.no_lds_perlin;
  return r;
}
