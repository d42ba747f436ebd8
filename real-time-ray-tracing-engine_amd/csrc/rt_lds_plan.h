// rt_lds_plan.h — the LDS residency plan of a scene, defined once.
//
// What a scene's blocks keep in LDS -- traversal stacks, a BFS prefix of the
// world BVH, for the persistent instance also the world items and spheres,
// the Perlin table -- and how many of them a CU holds follows from a handful
// of integers: a kernel instance's register count and static LDS (what the
// HIP runtime reports: KernelAttrs), the CU count, the scene's feature set,
// stack depth and table sizes, and rt_tuning.  This header holds the block
// shapes and byte counts that arithmetic shares with the launcher
// (rt_kernel.hip sizes its dynamic LDS from lds_bytes / lds_bytes_pc);
// rt_lds_plan.cpp holds the planners (plain C++, no HIP:
// host/rtx_plan_check.cpp runs them on the CPU, tests/test_lds_plan.py pins
// their outcomes).  rt_api.cpp fetches the attributes and applies the plan.
#ifndef RT_LDS_PLAN_H
#define RT_LDS_PLAN_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_api.h"
#include "rt_layout.h"

constexpr int kWaves = 4; // waves (work units) per block
// Flat instances (no BVH, nothing staged in LDS) run one-wave blocks: a
// block's wave slots are released only when all of its waves have ended, so
// with 4-wave blocks a slot idles until the slowest unit of its block is done
// (measured: C2 +2.0 %, C4 +10.4 % over 4-wave blocks; 2-wave blocks +0.5 % /
// +6.3 %; profiles/r03g_ab.log).  BVH instances keep 4-wave blocks: their
// waves share the block's staged BVH prefix.
constexpr int block_waves(unsigned f) { return (f & RT_FEAT_FLAT) ? 1 : kWaves; }
// Waves per block of the persistent instance: one block per CU (16 = 4 SIMDs x
// its 4-waves/SIMD target), so the CU's 160 KB of LDS holds ONE copy of the
// staged BVH beside its 16 waves' stacks instead of four copies for four
// 4-wave blocks (gfx950: a workgroup may own all 160 KB).
constexpr int kPcWaves = RT_PC_WAVES; // rt_layout.h
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr size_t kLdsPerBlock = 64 * 1024; // what a block may use without opt-in
// Feature sets with a persistent chunked-frame instance (render_tiles<.., PC>,
// whose waves pull work units from a counter): the plain BVH walks (C3 +3.4 %,
// profiles/r02ab-af_*); the flat and the rich instances keep one unit per wave
// -- the unit loop's extra live state cost them 2-20 %.
#define RT_PERSIST_F(F) (((F) & ~(unsigned)RT_FEAT_BVH4) == 0)

// What the HIP runtime reports about one kernel instance (hipFuncAttributes
// numRegs, sharedSizeBytes).
struct KernelAttrs {
  int32_t num_regs;
  int32_t static_lds;
};

// Resident waves per SIMD an instance's registers allow: 512 VGPRs per lane
// and SIMD, allocated in blocks of 8, at most 8 waves.
inline int waves_per_simd(int num_regs) {
  const int regs = ((num_regs + 7) / 8) * 8;
  const int w = regs > 0 ? 512 / regs : 8;
  return w > 8 ? 8 : w < 1 ? 1 : w;
}

// Dynamic LDS of a one-unit instance's block: its waves' traversal stacks
// (stack[depth][lane]) and the staged node prefix ...
inline size_t lds_bytes_waves(int features, int waves, int stack_depth, int n_lds_nodes) {
  return (size_t)waves * stack_depth * 64 * sizeof(int) + (size_t)n_lds_nodes * RT_LDS_NODE_BYTES(features);
}
inline size_t lds_bytes(int features, int stack_depth, int n_lds_nodes) {
  return lds_bytes_waves(features, block_waves((unsigned)features), stack_depth, n_lds_nodes);
}
// ... and of a persistent instance's block of pcw waves, which stages the
// world items and spheres after its nodes
inline size_t lds_bytes_pc(int features, int pcw, int stack_depth, int n_lds_nodes, int n_items, int n_spheres) {
  return lds_bytes_waves(features, pcw, stack_depth, n_lds_nodes) + (size_t)n_items * sizeof(DItem) +
         (size_t)n_spheres * sizeof(DSphere);
}

// LDS plan of one render instance: its occupancy target and what the
// per-block LDS share at that occupancy leaves for staged BVH nodes.
struct RtkLdsPlan {
  int32_t waves_per_simd; // resident waves per SIMD the instance's registers allow
  int32_t block_budget;   // LDS bytes per block at that occupancy (<= 64 KB)
  int32_t fixed_bytes;    // static LDS + traversal stacks per block
  int32_t stack_fits;     // fixed_bytes <= block_budget
  int32_t n_nodes;        // BVH nodes that fit in the rest (BFS prefix)
  int32_t resident_waves_per_cu; // waves resident per CU with no nodes staged (LDS may limit it)
};
// lds_cap > 0 lowers the per-block cap (rt_tuning.lds_cap: tests of the fallback)
RtkLdsPlan lds_plan(KernelAttrs a, int features, int stack_depth, int lds_cap);

// Whether a 4-wide collapse of d4 levels is walked: its stack must fit
// RT_STACK_DEPTH4, and its traversal stacks (three entries per 4-wide level,
// so a deep or lopsided collapse costs more LDS than the binary walk's one per
// level) the 4-wide instance's per-block share at its occupancy target: LDS
// must never lower occupancy.  Otherwise the tree stays binary.
enum Collapse4 { COLLAPSE4_FITS = 0, COLLAPSE4_TOO_DEEP, COLLAPSE4_OVER_SHARE };
// a4: the attributes of the instance of features | RT_FEAT_BVH4
Collapse4 collapse4_verdict(KernelAttrs a4, int features, int d4, int lds_cap);

struct LdsPlanInput {
  KernelAttrs render;   // the one-unit instance of `features`
  KernelAttrs pc16, pc4; // the persistent instance in blocks of kPcWaves / kWaves waves
                         // (read only where RT_PERSIST_F(features))
  int32_t cus;          // compute units of the device
  int32_t features, stack_depth;
  int32_t n_nodes, n_items, n_spheres, n_perlin; // world BVH nodes, world items, spheres, Perlin tables
};
enum LdsOutcome {
  LDS_OK = 0,
  // the traversal stacks and static LDS exceed the block's share at the
  // occupancy target (a compiler or register change can move that share): no
  // nodes staged, fewer resident blocks per CU (the caller warns)
  LDS_STACKS_OVER_SHARE,
  // ... and exceed the 64 KB a block may use without opt-in: refused (the
  // plan's remaining fields are not filled)
  LDS_UNSUPPORTED
};
struct SceneLdsPlan {
  RtkLdsPlan render;
  LdsOutcome outcome;
  int32_t n_lds_nodes; // DScene::n_lds_nodes
  int32_t wave_slots;  // resident waves of the render instance on the device
  // the persistent instance (pc_waves 0: none; then n_lds_nodes_pc -1, pc_grid 0)
  int32_t pc_waves, n_lds_nodes_pc, lds_items_pc, lds_spheres_pc; // the DScene fields
  int32_t pc_grid;     // its resident blocks on the device
  int32_t lds_perlin;  // DScene::lds_perlin
};
// Reads of rt_tuning: lds_cap, lds_nodes, lds_nodes_pc, no_lds_prims, pc_waves,
// no_lds_perlin.
SceneLdsPlan plan_scene_lds(const LdsPlanInput &in, const rt_tuning &tune);

#endif
