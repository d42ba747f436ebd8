// tests/native/rt_live_emu.cpp — TEST INFRASTRUCTURE ONLY.
//
// The live edits' shared source (csrc/rt_live.h: which entry is applied and what
// it writes; csrc/rt_live_check.h: what the host variants refuse; csrc/rt_refit.h:
// medium_box and item_box) compiled by g++ next to the scene compiler
// (csrc/rt_scene.cpp), for tests/test_live_edits.py: no GPU.  A handle is one
// compiled scene whose tables the edits are applied to, exactly as the
// library's kernels apply them to the device's copy.
#include "../../real-time-ray-tracing-engine_amd/csrc/rt_live_check.h"
#include "../../real-time-ray-tracing-engine_amd/csrc/rt_refit.h"
#include "../../real-time-ray-tracing-engine_amd/csrc/rt_scene.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Live {
  rtx::HostScene H;
  std::vector<double> quad_n; // 3 per DQuad record, as the library keeps them
};

rt_live::LiveIndex index_of(const Live &s) {
  rt_live::LiveIndex L{};
  L.n_objects = (int32_t)s.H.xf_kind.size();
  L.xf_kind = s.H.xf_kind.data();
  L.xf_first = s.H.xf_first.data();
  L.xf_recs = s.H.xf_recs.data();
  L.quad_of = s.H.quad_of.data();
  return L;
}

void say(const std::string &err, char *msg, int cap) {
  if (msg && cap > 0) std::snprintf(msg, (size_t)cap, "%s", err.c_str());
}

// the world items in compile order (a host build leaves H.items in leaf order)
const std::vector<DItem> &compile_items(const rtx::HostScene &H) { return H.compile_items.empty() ? H.items : H.compile_items; }

} // namespace

// Compiles `desc` as given (its bvh_builder included): a handle, or null with msg filled.
extern "C" void *live_emu_open(const rt_scene_desc *desc, char *msg, int cap) {
  Live *s = new Live();
  std::string err;
  if (rtx::compile_scene(desc, s->H, err) != RT_OK) {
    say(err, msg, cap);
    delete s;
    return nullptr;
  }
  if (s->H.device_bvh) rtx::build_world_bvh_host(s->H); // the tree the refit test needs; items go to leaf order
  s->quad_n.resize(3 * s->H.quads.size());
  for (size_t q = 0; q < s->H.quads.size(); ++q)
    for (int a = 0; a < 3; ++a) s->quad_n[3 * q + a] = s->H.quads[q].n[a];
  return s;
}
extern "C" void live_emu_close(void *h) { delete (Live *)h; }

// A table of the compiled scene: its address and *bytes.  which: 0 xforms, 1 quads, 2 mbox (as
// compiled), 3 nodes (binary), 4 items (leaf order), 5 mitems, 6 bitems, 7 media, 8 spheres,
// 9 items in compile order, 10 xf_kind, 11 xf_first, 12 xf_recs, 13 quad_of, 14 lights.
extern "C" const void *live_emu_table(void *h, int which, long long *bytes) {
  rtx::HostScene &H = ((Live *)h)->H;
  auto give = [&](const auto &v) -> const void * {
    *bytes = (long long)(v.size() * sizeof(v[0]));
    return v.data();
  };
  switch (which) {
  case 0: return give(H.xforms);
  case 1: return give(H.quads);
  case 2: return give(H.mbox);
  case 3: return give(H.nodes);
  case 4: return give(H.items);
  case 5: return give(H.mitems);
  case 6: return give(H.bitems);
  case 7: return give(H.media);
  case 8: return give(H.spheres);
  case 9: return give(compile_items(H));
  case 10: return give(H.xf_kind);
  case 11: return give(H.xf_first);
  case 12: return give(H.xf_recs);
  case 13: return give(H.quad_of);
  case 14: return give(H.lights);
  }
  *bytes = 0;
  return nullptr;
}
extern "C" int live_emu_root_is_leaf(void *h) { return ((Live *)h)->H.root_is_leaf; }

// rt_refit::item_box of every world item from the tables as they are now, in leaf order
// (leaf_order != 0) or in compile order: 6 doubles each.
extern "C" void live_emu_item_boxes(void *h, int leaf_order, double *out) {
  const rtx::HostScene &H = ((Live *)h)->H;
  const std::vector<DItem> &items = leaf_order ? H.items : compile_items(H);
  for (size_t i = 0; i < items.size(); ++i) {
    const rt_refit::Bx b = rt_refit::item_box(items[i], H.spheres.data(), H.quads.data(), H.xforms.data());
    for (int a = 0; a < 3; ++a) {
      out[6 * i + a] = b.lo[a];
      out[6 * i + 3 + a] = b.hi[a];
    }
  }
}

// rt_refit::medium_box of every world medium from the tables as they are now: 6 floats each.
extern "C" void live_emu_medium_boxes(void *h, float *out) {
  const rtx::HostScene &H = ((Live *)h)->H;
  for (size_t m = 0; m < H.mitems.size(); ++m)
    rt_refit::medium_box(H.mitems[m], H.media.data(), H.bitems.data(), H.spheres.data(), H.quads.data(),
                         H.xforms.data(), out + 6 * m);
}

// The host variants, on the handle's tables: the shared check, then the shared apply per entry.
// Returns the code rt_scene_set_transforms / rt_scene_move_quads returns, msg filled on a refusal.
extern "C" int live_emu_set_transforms(void *h, int n, const int32_t *ids, const double *values, char *msg, int cap) {
  Live &s = *(Live *)h;
  const rt_live::LiveIndex L = index_of(s);
  std::string err;
  const int rc = rt_live::check_transforms(L, n, ids, values, err);
  say(err, msg, cap);
  if (rc != RT_OK) return rc;
  for (int j = 0; j < n; ++j) rt_live::apply_transform(L, ids[j], values + 3 * (size_t)j, s.H.xforms.data());
  return RT_OK;
}
extern "C" int live_emu_move_quads(void *h, int n, const int32_t *ids, const double *corners, char *msg, int cap) {
  Live &s = *(Live *)h;
  const rt_live::LiveIndex L = index_of(s);
  std::string err;
  const int rc = rt_live::check_quads(L, n, ids, corners, s.quad_n.data(), err);
  say(err, msg, cap);
  if (rc != RT_OK) return rc;
  for (int j = 0; j < n; ++j) {
    double D = 0.0;
    rt_live::quad_entry(L, ids[j], corners + 3 * (size_t)j, s.quad_n.data(), 3, D);
    rt_live::apply_quad(s.H.quads[L.quad_of[ids[j]]], corners + 3 * (size_t)j, D);
  }
  return RT_OK;
}
