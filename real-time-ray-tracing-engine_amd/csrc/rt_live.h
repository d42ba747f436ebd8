// rt_live.h — live edits of a scene's transforms and quads: which entry of an
// update is applied, and what applying it writes.  One source for the kernels
// (rt_refit.hip, one thread per entry), for the host variants' validation
// (rt_api.cpp) and for the host twin (tests/native/rt_live_emu.cpp).
//
// A transform object owns every xforms[] record the scene compiler emitted for
// it (rt_scene.cpp emit_chain: one per distinct chain the object stands in);
// setting it writes them all.  A quad move writes Q and the plane constant
// D = dot(n, Q), the compiler's expression (quad_record: dotp(nn, Q)); u, v, n,
// w, area and aa do not depend on Q.  Built with -ffp-contract=off everywhere.
#ifndef RT_LIVE_H
#define RT_LIVE_H
#include <math.h>
#include <stdint.h>

#include "rt_layout.h"
#include "rt_refit.h"

namespace rt_live {

// Per object of the description (HostScene::xf_kind, xf_first, xf_recs, quad_of).
struct LiveIndex {
  int32_t n_objects, pad_;
  const int32_t *xf_kind;  // X_TRANSLATE / X_ROTATE_Y, -1: not a transform object
  const int32_t *xf_first; // n_objects + 1 offsets into xf_recs
  const int32_t *xf_recs;  // xforms[] records, grouped by object
  const int32_t *quad_of;  // DQuad record; -1: none; -2: the quad bounds a medium
};

// Why an entry is not applied (0: it is).  LIVE_TWICE is the caller's to find.
enum {
  LIVE_OK = 0,
  LIVE_RANGE,     // id outside [0, n_objects)
  LIVE_KIND,      // not a translate / rotate_y (set_transforms); no quad record (move_quads)
  LIVE_NO_RECORD, // a transform object that stands in no chain
  LIVE_BOUNDARY,  // a quad that bounds a medium
  LIVE_VALUE,     // a value that is not finite
  LIVE_PLANE,     // dot(n, Q) of the new corner is not finite
  LIVE_TWICE
};

RT_REFIT_HD bool finite_(double x) { return x - x == 0.0; } // neither NaN nor an infinity

RT_REFIT_HD int transform_entry(const LiveIndex &L, int32_t id, const double *v) {
  if (id < 0 || id >= L.n_objects) return LIVE_RANGE;
  const int32_t kind = L.xf_kind[id];
  if (kind < 0) return LIVE_KIND;
  if (L.xf_first[id + 1] == L.xf_first[id]) return LIVE_NO_RECORD;
  const int n = kind == X_TRANSLATE ? 3 : 2; // a rotate_y row's third value is not looked at
  for (int a = 0; a < n; ++a)
    if (!finite_(v[a])) return LIVE_VALUE;
  return LIVE_OK;
}
RT_REFIT_HD void apply_transform(const LiveIndex &L, int32_t id, const double *v, DXform *xforms) {
  const bool translate = L.xf_kind[id] == X_TRANSLATE;
  for (int32_t k = L.xf_first[id]; k < L.xf_first[id + 1]; ++k) {
    DXform &x = xforms[L.xf_recs[k]];
    x.a = v[0];
    x.b = v[1];
    if (translate) x.c = v[2];
  }
}

// quad_record's D: dotp(nn, Q)
RT_REFIT_HD double plane_constant(const double n[3], const double Q[3]) { return n[0] * Q[0] + n[1] * Q[1] + n[2] * Q[2]; }

// `normals`: 3 doubles per DQuad record, at `stride` doubles (the device reads
// DQuad::n in place, the host a packed copy kept from creation)
RT_REFIT_HD int quad_entry(const LiveIndex &L, int32_t id, const double *corner, const double *normals, int stride,
                           double &D) {
  if (id < 0 || id >= L.n_objects) return LIVE_RANGE;
  const int32_t rec = L.quad_of[id];
  if (rec == -2) return LIVE_BOUNDARY;
  if (rec < 0) return LIVE_KIND;
  for (int a = 0; a < 3; ++a)
    if (!finite_(corner[a])) return LIVE_VALUE;
  D = plane_constant(normals + (size_t)stride * rec, corner);
  return finite_(D) ? LIVE_OK : LIVE_PLANE;
}
RT_REFIT_HD void apply_quad(DQuad &q, const double *corner, double D) {
  for (int a = 0; a < 3; ++a) q.Q[a] = corner[a];
  q.D = D;
}

// A pose (rt_scene_pose_device): everything the edits above and a sphere move
// can write, three doubles per table record -- (a, b, c) of the xforms[]
// records, then c0 of the spheres[] records, then Q of the quads[] records.
// Indexed by table record: a rebuild permutes the items, never these tables
// (rt_api.cpp rt_scene_rebuild_bvh commits nodes and items only).  D of a quad
// follows from Q and is not part of it; a rotate_y record's c is carried along
// unread.  Read by rt_motion.h alone.
struct PoseCounts {
  int32_t n_xforms, n_spheres, n_quads, pad_;
};
RT_REFIT_HD int64_t pose_records(const PoseCounts &c) { return (int64_t)c.n_xforms + c.n_spheres + c.n_quads; }
RT_REFIT_HD int64_t pose_bytes(const PoseCounts &c) { // a multiple of 256, >= 256
  const int64_t b = 3 * (int64_t)sizeof(double) * pose_records(c);
  return b < 256 ? 256 : (b + 255) & ~(int64_t)255;
}
RT_REFIT_HD const double *pose_xform(const PoseCounts &, const double *pose, int rec) { return pose + 3 * (int64_t)rec; }
RT_REFIT_HD const double *pose_sphere(const PoseCounts &c, const double *pose, int rec) {
  return pose + 3 * ((int64_t)c.n_xforms + rec);
}
RT_REFIT_HD const double *pose_quad(const PoseCounts &c, const double *pose, int rec) {
  return pose + 3 * ((int64_t)c.n_xforms + c.n_spheres + rec);
}
// record k in [0, pose_records) of the pose of these tables
RT_REFIT_HD void pose_pack(const PoseCounts &c, int64_t k, const DXform *xforms, const DSphere *spheres,
                           const DQuad *quads, double out[3]) {
  if (k < c.n_xforms) {
    const DXform &x = xforms[k];
    out[0] = x.a, out[1] = x.b, out[2] = x.c;
  } else if (k < (int64_t)c.n_xforms + c.n_spheres) {
    const DSphere &s = spheres[k - c.n_xforms];
    out[0] = s.c0[0], out[1] = s.c0[1], out[2] = s.c0[2];
  } else {
    const DQuad &q = quads[k - c.n_xforms - c.n_spheres];
    out[0] = q.Q[0], out[1] = q.Q[1], out[2] = q.Q[2];
  }
}

} // namespace rt_live
#endif
