// rt_scene.h — host scene compiler: rt_scene_desc -> flat device layout, and
// the host binding of a compiled scene (BoundHostScene).
#ifndef RT_SCENE_H
#define RT_SCENE_H
#include "../../include/rt_api.h"
#include "rt_layout.h"

#include <string>
#include <vector>

namespace rtx {

struct HostScene {
  std::vector<DNode> nodes;
  std::vector<DNode4> nodes4; // the world BVH collapsed to 4-wide nodes (bvh_arity 4)
  std::vector<DItem> items;
  // the world items in compile order -- the order compile_scene emits them in,
  // which a device build starts from -- once the host builder has put `items`
  // into leaf order; empty while `items` is still in that order itself
  std::vector<DItem> compile_items;
  std::vector<DItem> mitems; // media (not in the BVH)
  std::vector<float> mbox;   // 6 per medium
  std::vector<DItem> bitems;
  std::vector<DXform> xforms;
  std::vector<DSphere> spheres;
  std::vector<DQuad> quads;
  std::vector<DMedium> media;
  std::vector<DMat> mats;
  std::vector<DTex> texs;
  std::vector<DPerlin> perlin;
  std::vector<DLight> lights;
  std::vector<DRoot> roots;  // build_root_table: one per root item, or empty
  int32_t root_is_leaf = 0;
  int32_t n_root_items = 0;
  int32_t bvh_depth = 0;
  int32_t bvh_arity = 2;  // 4: nodes4 is the tree the kernel walks
  int32_t bvh_depth4 = 0; // levels of 4-wide nodes
  // device-built world BVH (0: built on the host; RT_BVH_DEVICE: linear BVH,
  // rt_bvh_build.hip; RT_BVH_DEVICE_SAH: binned SAH, rt_bvh_sah.hip): items still
  // in scene order, their boxes (lo xyz, hi xyz) and the centroid bounds; nodes
  // sized, not filled
  int32_t device_bvh = 0;
  // host SAH builder overrides (rt_tuning sah_*; 0: the builder's defaults),
  // set by the caller before compile_scene
  int32_t sah_leaf_max = 0, sah_leaf_split = 0, sah_trav_x4 = 0, sah_bins = 0;
  std::vector<double> item_boxes;
  double scene_lo[3] = {0, 0, 0}, scene_hi[3] = {0, 0, 0};
  // Live edits (rt_scene_set_transforms*, rt_scene_move_quads*; rt_live.h LiveIndex), one entry
  // per object of the description:
  //   xf_kind      X_TRANSLATE / X_ROTATE_Y for a translate / rotate_y object, -1 for any other;
  //   xf_first     CSR offsets (n_objects + 1) into xf_recs, the xforms[] records emit_chain wrote
  //                for the object: one per distinct chain it stands in ([T] and [T, R] are two);
  //   quad_of      a quad's DQuad record when it is a world primitive item or a light leaf, -1
  //                when the object has no such record, -2 when it (also) bounds a medium.
  std::vector<int32_t> xf_kind, xf_first, xf_recs, quad_of;
};

// The object each xforms[] record came from, one entry per record: the live
// index above read the other way (ray queries, rt_query.h: the first record of
// an item's chain names the outermost transform above it).  Its own table
// beside the scene's: DScene and the bytes of its tables stay what they were.
inline std::vector<int32_t> xform_objects(const std::vector<int32_t> &xf_first, const std::vector<int32_t> &xf_recs) {
  std::vector<int32_t> obj(xf_recs.size(), -1);
  for (size_t o = 0; o + 1 < xf_first.size(); ++o)
    for (int32_t k = xf_first[o]; k < xf_first[o + 1]; ++k) obj[xf_recs[k]] = (int32_t)o;
  return obj;
}

// 1 when no sphere moves (DScene::static_spheres): a flat world then runs the
// static instantiation of its item walk and hit record (rt_path.h trace,
// trace_tail), without the center.at(time) arithmetic, whose result is c0
// exactly for these spheres.  BVH worlds ignore the flag.
inline int32_t all_spheres_static(const HostScene &H) {
  for (const DSphere &s : H.spheres)
    if (s.dir[0] != 0.0 || s.dir[1] != 0.0 || s.dir[2] != 0.0) return 0;
  return 1;
}

// The packed root-item table (DScene::roots; rt_layout.h DRoot): built for a
// flat world whose root items are all untransformed spheres and in which no
// sphere moves -- the world the static sphere-only walk of the plain flat
// instance serves.  The values are copies of the doubles in DSphere and of
// DItem::mat, in root-item order; nothing is recomputed.  Every other world
// gets no table and keeps the item -> sphere walk.  Called once the host's
// world tree is final (compile_scene); a device-built tree leaves it empty.
inline void build_root_table(HostScene &H) {
  H.roots.clear();
  if (!H.root_is_leaf || H.n_root_items <= 0 || (size_t)H.n_root_items > H.items.size()) return;
  if (!all_spheres_static(H)) return;
  for (int32_t i = 0; i < H.n_root_items; ++i)
    if (H.items[i].kind != I_SPHERE || H.items[i].xf_count != 0) return;
  H.roots.resize(H.n_root_items);
  for (int32_t i = 0; i < H.n_root_items; ++i) {
    const DItem &it = H.items[i];
    const DSphere &s = H.spheres[it.idx];
    DRoot &r = H.roots[i];
    for (int a = 0; a < 3; ++a) r.test.c0[a] = s.c0[a];
    r.test.rr = s.rr;
    r.inv_r = s.inv_r;
    r.mat = it.mat;
    r.pad = 0;
  }
}

// The feature bits of the path-tracer instance a compiled scene needs
// (RT_FEAT_MEDIA / XFORM / LIGHTS / NOISE; RT_FEAT_FLAT and RT_FEAT_BVH4 follow
// from the world tree once it is built): the GPU library's choice and the CPU
// backend's (host/rtx_cpu.cpp) alike.
inline int32_t scene_features(const HostScene &H) {
  int32_t f = 0;
  if (!H.mitems.empty()) f |= RT_FEAT_MEDIA;
  for (const DItem &it : H.items)
    if (it.xf_count) f |= RT_FEAT_XFORM;
  for (const DItem &it : H.mitems)
    if (it.xf_count) f |= RT_FEAT_XFORM;
  for (const DLight &L : H.lights)
    if (L.xf_count) f |= RT_FEAT_XFORM;
  if (!H.lights.empty()) f |= RT_FEAT_LIGHTS;
  for (const DTex &t : H.texs)
    if (t.kind == RT_TEX_NOISE) f |= RT_FEAT_NOISE;
  return f;
}

// 1 when every entry of the materials table is Lambertian and the texture it
// names is a solid colour (RT_FEAT_DIFFUSE): shade then needs no material kind
// and tex_value is one colour load (rt_path.h M_DIFFUSE).  Over the table, not
// over what the world references: an unused metal material turns it off, so
// the bit never depends on reachability.  An empty table has no material to
// vouch for.
inline int32_t diffuse_only(const HostScene &H) {
  if (H.mats.empty()) return 0;
  for (const DMat &m : H.mats) {
    if (m.kind != RT_MAT_LAMBERTIAN) return 0;
    if (m.tex < 0 || (size_t)m.tex >= H.texs.size() || H.texs[m.tex].kind != RT_TEX_SOLID) return 0;
  }
  return 1;
}

// The scene's tables, named once: f(DScene member, HostScene vector) for each,
// in the order the GPU library lays them out in a scene's device block
// (rt_api.cpp).  A table added to DScene is added here and nowhere else.
template <class F>
inline void for_each_table(F &&f) {
  f(&DScene::nodes, &HostScene::nodes);
  f(&DScene::items, &HostScene::items);
  f(&DScene::bitems, &HostScene::bitems);
  f(&DScene::mitems, &HostScene::mitems);
  f(&DScene::mbox, &HostScene::mbox);
  f(&DScene::xforms, &HostScene::xforms);
  f(&DScene::spheres, &HostScene::spheres);
  f(&DScene::quads, &HostScene::quads);
  f(&DScene::media, &HostScene::media);
  f(&DScene::mats, &HostScene::mats);
  f(&DScene::texs, &HostScene::texs);
  f(&DScene::perlin, &HostScene::perlin);
  f(&DScene::lights, &HostScene::lights);
  f(&DScene::roots, &HostScene::roots);
}

// What a DScene holds of a compiled scene beside its tables: the counts, the
// binary world tree's shape and the instance key (RT_FEAT_FLAT from
// root_is_leaf).  The GPU library calls it once the world tree is final.
inline void bind_counts(DScene &S, const HostScene &H) {
  S.n_mitems = (int32_t)H.mitems.size();
  S.n_lights = (int32_t)H.lights.size();
  S.n_nodes = (int32_t)H.nodes.size();
  S.root_is_leaf = H.root_is_leaf;
  S.n_root_items = H.n_root_items;
  S.static_spheres = all_spheres_static(H);
  S.n_roots = (int32_t)H.roots.size();
  S.features = scene_features(H) | (H.root_is_leaf ? RT_FEAT_FLAT : 0) | (diffuse_only(H) ? RT_FEAT_DIFFUSE : 0);
}

// A DScene over the HostScene's own vectors, the binary tree in `nodes`.  The
// LDS fields stay 0; stack_depth is the caller's (traversal_stack_depth).
// BoundHostScene below is the whole host binding, 4-wide tree included.
inline DScene bind_host_scene(const HostScene &H) {
  DScene S{};
  for_each_table([&](auto dm, auto hm) { S.*dm = (H.*hm).data(); });
  bind_counts(S, H);
  return S;
}

// Scenes with at least this many world primitives build their BVH on the
// device when rt_scene_desc.bvh_builder is RT_BVH_AUTO.
constexpr int kDeviceBuildMin = 65536;

// Host SAH build from HostScene::item_boxes (fallback of the device build).
void build_world_bvh_host(HostScene &H);

// Scenes with at least this many world primitives walk a 4-wide BVH when
// rt_scene_desc.bvh_arity is 0 (auto).
constexpr int kBvh4Min = 4096;
// The arity rule: whether a description's world walks a 4-wide tree, where it
// has a tree at all (rt_scene_create*; the kernels' host twins).
inline bool wants_bvh4(const rt_scene_desc *desc, const HostScene &H) {
  return desc->bvh_arity == 4 || (desc->bvh_arity == 0 && H.items.size() >= (size_t)kBvh4Min);
}

// Collapses the binary BFS-ordered tree `bin` (root 0) into 4-wide nodes, BFS
// order, root 0: each 4-wide node starts from one binary node's two children
// and repeatedly replaces its largest-area inner child by that child's two
// children until it holds four (or only leaves).  Leaf entries keep their
// encoding, so the leaf item ranges are shared with the binary tree.  Returns
// the number of 4-wide levels.
int collapse_bvh4(const std::vector<DNode> &bin, std::vector<DNode4> &out);

// SAH cost of a binary tree (rt_scene_bvh_cost): 1 + sum over child boxes of
// (1 for an inner child, its item count for a leaf) x area / root area.
double bvh_sah_cost(const std::vector<DNode> &nodes);

// The traversal stack a 4-wide walk of depth4 levels needs: at most three
// pushed siblings per level on the current root path.
inline int bvh4_stack_depth(int depth4) { return 3 * depth4 + 1; }

// The per-lane traversal stack of the tree a scene walks (DScene::stack_depth):
// one entry per BVH level suffices (a pushed entry is the sibling of a node on
// the current root path; bvh4_stack_depth for a 4-wide tree, bvh_arity 4).
// The walk pushes without an overflow check (rt_path.h trace), so the depth the
// stack is sized from must be the tree's, never clamped below it: a tree
// deeper than RT_STACK_DEPTH / RT_STACK_DEPTH4 is refused -- returns 0 with
// `err` filled.
inline int traversal_stack_depth(const HostScene &H, std::string &err) {
  if (H.bvh_depth + 1 > RT_STACK_DEPTH) {
    err = "world BVH deeper than the traversal stack (" + std::to_string(H.bvh_depth) + " levels)";
    return 0;
  }
  if (H.bvh_arity != 4) return H.bvh_depth + 1 > 1 ? H.bvh_depth + 1 : 1;
  if (bvh4_stack_depth(H.bvh_depth4) > RT_STACK_DEPTH4) {
    err = "4-wide world BVH deeper than the traversal stack (" + std::to_string(H.bvh_depth4) + " levels)";
    return 0;
  }
  return bvh4_stack_depth(H.bvh_depth4);
}

// Returns RT_OK or an error code with `err` filled.
int compile_scene(const rt_scene_desc *desc, HostScene &out, std::string &err);

// Camera::initialize (Camera.cpp:31-73), same operation order.
int camera_setup(const rt_camera_desc *cam, rt_frame *frame, std::string &err);

// The validation both backends apply to a launch (librtx_hip.so's rt_render*
// and librtx_cpu.so's rt_cpu_render): a set-up frame -> the kernel's camera
// values, and the params' row band, stratum range, output, layout, tile subset
// and chunk count -> the launch geometry (one work unit per tile, or every
// tile in strata_chunks chunks).  strata_chunks < 0 is refused here:
// RT_CHUNKS_AUTO is resolved by the callers that accept it.
int device_camera(const rt_frame *frame, DCamera &c, std::string &err);
int launch_geometry(const rt_frame *frame, const rt_render_params *p, DLaunch &L, std::string &err);

// A description as host code walks it (the CPU backend, host/rtx_cpu.cpp; the kernels' host twins,
// tests/native/*_emu.cpp, rt_emulate.cpp): compiled, its world tree built by the host builder whatever
// builder it names (the device builders need a GPU), collapsed to 4-wide nodes when wanted and there is
// a tree -- S.nodes / n_nodes are then that tree and S.features has RT_FEAT_BVH4, as in the GPU library's
// DScene -- and S.stack_depth the tree's.  Owns the HostScene that S points into.  bind: RT_OK,
// compile_scene's code (compiled false) or RT_ERR_UNSUPPORTED for a tree deeper than the stack, `err` filled.
struct BoundHostScene {
  HostScene H; // the sah_* overrides may be set before bind
  DScene S{};
  std::string err;
  bool compiled = false;
  BoundHostScene() = default;
  BoundHostScene(const BoundHostScene &) = delete; // S points into H
  bool bvh4() const { return H.bvh_arity == 4; }
  // want4: 1 / 0 the caller's choice of tree, -1 the library's (wants_bvh4)
  int bind(const rt_scene_desc *desc, int want4 = -1) {
    if (int rc = compile_scene(desc, H, err)) return rc;
    compiled = true;
    if (H.device_bvh) build_world_bvh_host(H);
    if ((want4 < 0 ? wants_bvh4(desc, H) : want4 != 0) && !H.root_is_leaf && !H.nodes.empty()) {
      H.bvh_depth4 = collapse_bvh4(H.nodes, H.nodes4);
      H.bvh_arity = 4;
    }
    S = bind_host_scene(H);
    if (bvh4()) {
      S.nodes = (const DNode *)(const void *)H.nodes4.data();
      S.n_nodes = (int32_t)H.nodes4.size();
      S.features |= RT_FEAT_BVH4;
    }
    S.stack_depth = traversal_stack_depth(H, err);
    return S.stack_depth ? RT_OK : RT_ERR_UNSUPPORTED;
  }
};

} // namespace rtx
#endif
