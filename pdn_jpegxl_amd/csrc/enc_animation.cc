// The geometry rules of animation encode (see enc_animation.h).
#include "enc_animation.h"
#include <algorithm>

namespace jxlhip {

AnimRect AnimFrameRect(int32_t k, int32_t key_interval, const AnimExtent& ext, int32_t w, int32_t h, bool lossless) {
  if (AnimIsKeyFrame(k, key_interval)) return AnimRect{0, 0, w, h};
  if (AnimExtentEmpty(ext)) return AnimRect{0, 0, 1, 1};
  int32_t x0 = ext.x0, y0 = ext.y0, x1 = ext.x1 + 1, y1 = ext.y1 + 1;   // [x0, x1) x [y0, y1)
  if (!lossless) {
    x0 &= ~7; y0 &= ~7;
    x1 = (int32_t)std::min<int64_t>(w, ((int64_t)x1 + 7) & ~(int64_t)7);
    y1 = (int32_t)std::min<int64_t>(h, ((int64_t)y1 + 7) & ~(int64_t)7);
  }
  return AnimRect{x0, y0, x1 - x0, y1 - y0};
}

EncFramePlacement AnimPlacement(int32_t k, int32_t n, const AnimRect& r, int32_t w, int32_t h, uint32_t duration) {
  EncFramePlacement at;
  at.have_crop = !(r.x == 0 && r.y == 0 && r.w == w && r.h == h);
  at.x0 = r.x; at.y0 = r.y;
  at.width = (uint32_t)r.w; at.height = (uint32_t)r.h;
  at.duration = duration;
  at.is_last = k == n - 1;
  at.save_as_reference = at.is_last ? 0 : kAnimSlot;
  at.source = kAnimSlot;
  return at;
}

}  // namespace jxlhip
