// rt_live_check.h — what the host variants of rt_scene_set_transforms and
// rt_scene_move_quads refuse, over rt_live.h's entry rules (which the device
// variants apply entry by entry): everything is validated before anything is
// written.  Host only, no device needed: rt_api.cpp calls these, and so does
// the host twin (tests/native/rt_live_emu.cpp).
#ifndef RT_LIVE_CHECK_H
#define RT_LIVE_CHECK_H
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_live.h"

namespace rt_live {

inline int refusal(int why, int32_t j, int32_t id, bool transforms, std::string &err) {
  const std::string at = "entry " + std::to_string(j) + ": object " + std::to_string(id);
  switch (why) {
  case LIVE_RANGE: err = at + " is out of range"; break;
  case LIVE_KIND:
    err = at + (transforms ? " is not a translate or rotate_y object"
                           : " is not a quad among the world's primitive items or the lights");
    break;
  case LIVE_NO_RECORD: err = at + " stands in no transform chain of the world, a medium or the lights"; break;
  case LIVE_BOUNDARY: err = at + " bounds a constant medium: its face constants would have to follow"; break;
  case LIVE_VALUE: err = at + (transforms ? ": the value is not finite" : ": the corner is not finite"); break;
  case LIVE_PLANE: err = at + ": the plane constant dot(n, Q) of the new corner is not finite"; break;
  default: err = at + " is named twice"; break;
  }
  return why == LIVE_BOUNDARY ? RT_ERR_UNSUPPORTED : RT_ERR_INVALID;
}

inline int check_transforms(const LiveIndex &L, int32_t n, const int32_t *ids, const double *values, std::string &err) {
  std::vector<char> seen((size_t)L.n_objects, 0);
  for (int32_t j = 0; j < n; ++j) {
    const int why = transform_entry(L, ids[j], values + 3 * (size_t)j);
    if (why != LIVE_OK) return refusal(why, j, ids[j], true, err);
    if (seen[ids[j]]) return refusal(LIVE_TWICE, j, ids[j], true, err);
    seen[ids[j]] = 1;
  }
  return RT_OK;
}

// normals: 3 doubles per DQuad record, packed
inline int check_quads(const LiveIndex &L, int32_t n, const int32_t *ids, const double *corners, const double *normals,
                       std::string &err) {
  std::vector<char> seen((size_t)L.n_objects, 0);
  for (int32_t j = 0; j < n; ++j) {
    double D;
    const int why = quad_entry(L, ids[j], corners + 3 * (size_t)j, normals, 3, D);
    if (why != LIVE_OK) return refusal(why, j, ids[j], false, err);
    if (seen[ids[j]]) return refusal(LIVE_TWICE, j, ids[j], false, err);
    seen[ids[j]] = 1;
  }
  return RT_OK;
}

} // namespace rt_live
#endif
