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

// ---- several rectangles per frame

namespace {

struct Box { int32_t x0, y0, x1, y1; };   // [x0, x1) x [y0, y1)

inline int64_t Area(const Box& b) { return (int64_t)(b.x1 - b.x0) * (b.y1 - b.y0); }
inline Box Bound(const Box& a, const Box& b) { return Box{std::min(a.x0, b.x0), std::min(a.y0, b.y0), std::max(a.x1, b.x1), std::max(a.y1, b.y1)}; }
inline bool Overlap(const Box& a, const Box& b) { return a.x0 < b.x1 && b.x0 < a.x1 && a.y0 < b.y1 && b.y0 < a.y1; }

// the tile's box in canvas pixels, inclusive corners
inline AnimExtent TileExtent(uint32_t word, int32_t tx, int32_t ty) {
  return AnimExtent{tx * kAnimTile + (int32_t)(word & 255), ty * kAnimTile + (int32_t)(word >> 8 & 255), tx * kAnimTile + (int32_t)(word >> 16 & 255),
                    ty * kAnimTile + (int32_t)(word >> 24)};
}

inline void Widen(AnimExtent& e, const AnimExtent& t) {
  if (AnimExtentEmpty(e)) { e = t; return; }
  e.x0 = std::min(e.x0, t.x0); e.y0 = std::min(e.y0, t.y0);
  e.x1 = std::max(e.x1, t.x1); e.y1 = std::max(e.y1, t.y1);
}

// step 3: boxes that share a pixel become their bounding box, until none do (the result does not depend on the order: it is the
// finest partition of the boxes into groups whose bounding boxes are disjoint)
void Close(std::vector<Box>& b) {
  for (bool again = true; again;) {
    again = false;
    for (size_t i = 0; i < b.size(); i++) {
      for (size_t j = i + 1; j < b.size();) {
        if (!Overlap(b[i], b[j])) { j++; continue; }
        b[i] = Bound(b[i], b[j]);
        b[j] = b.back();
        b.pop_back();
        again = true;
        j = i + 1;   // b[i] grew: what it passed over may touch it now
      }
    }
  }
}

}  // namespace

const char* AnimRectOptionsRefusal(int32_t max_rects, int32_t merge_pixels) {
  if (max_rects < 1 || max_rects > kAnimMaxRects) return "the rectangles per frame (max_rects) must be 1..16";
  if (merge_pixels < 0) return "merge_pixels must not be negative";
  return nullptr;
}

const char* AnimToleranceRefusal(float tolerance) {
  if (tolerance != tolerance || tolerance - tolerance != 0.f) return "the tolerance must be a finite number";
  if (tolerance < 0.f) return "the tolerance must not be negative";
  return nullptr;
}

AnimExtent AnimTilesExtent(const uint32_t* tiles, int32_t w, int32_t h) {
  const int32_t nx = (int32_t)AnimTilesAcross(w), ny = (int32_t)AnimTilesAcross(h);
  AnimExtent e{-1, -1, -1, -1};
  for (int32_t ty = 0; ty < ny; ty++)
    for (int32_t tx = 0; tx < nx; tx++) {
      const uint32_t word = tiles[(size_t)ty * nx + tx];
      if (word != kAnimTileEmpty) Widen(e, TileExtent(word, tx, ty));
    }
  return e;
}

std::vector<AnimRect> AnimFrameRects(const uint32_t* tiles, int32_t w, int32_t h, bool lossless, int32_t max_rects, int64_t merge_pixels) {
  const int32_t nx = (int32_t)AnimTilesAcross(w), ny = (int32_t)AnimTilesAcross(h);
  // 2. components of the non-empty tiles, 8-connected, by flooding
  std::vector<uint8_t> seen((size_t)nx * ny, 0);
  std::vector<int32_t> stack;
  std::vector<Box> boxes;
  for (int32_t start = 0; start < nx * ny; start++) {
    if (seen[(size_t)start] || tiles[(size_t)start] == kAnimTileEmpty) continue;
    AnimExtent e{-1, -1, -1, -1};
    seen[(size_t)start] = 1;
    stack.assign(1, start);
    while (!stack.empty()) {
      const int32_t t = stack.back(), tx = t % nx, ty = t / nx;
      stack.pop_back();
      Widen(e, TileExtent(tiles[(size_t)t], tx, ty));
      for (int32_t yy = std::max(ty - 1, 0); yy <= std::min(ty + 1, ny - 1); yy++)
        for (int32_t xx = std::max(tx - 1, 0); xx <= std::min(tx + 1, nx - 1); xx++) {
          const size_t u = (size_t)yy * nx + xx;
          if (seen[u] || tiles[u] == kAnimTileEmpty) continue;
          seen[u] = 1;
          stack.push_back((int32_t)u);
        }
    }
    const AnimRect r = AnimFrameRect(1, 0, e, w, h, lossless);   // (the lossy snapping, stated there)
    boxes.push_back(Box{r.x, r.y, r.x + r.w, r.y + r.h});
  }
  if (boxes.empty()) return {AnimRect{0, 0, 1, 1}};               // 1.
  Close(boxes);                                                   // 3.
  if ((int32_t)boxes.size() > kAnimMaxComponents) {               // 4.
    Box all = boxes[0];
    for (const Box& b : boxes) all = Bound(all, b);
    boxes.assign(1, all);
  }
  // 5.
  auto in_order = [](const Box& a, const Box& b) { return a.y0 != b.y0 ? a.y0 < b.y0 : a.x0 < b.x0; };
  std::sort(boxes.begin(), boxes.end(), in_order);
  while (boxes.size() >= 2) {
    size_t bi = 0, bj = 1;
    int64_t best = -1;
    for (size_t i = 0; i < boxes.size(); i++)
      for (size_t j = i + 1; j < boxes.size(); j++) {
        const int64_t cost = Area(Bound(boxes[i], boxes[j])) - Area(boxes[i]) - Area(boxes[j]);
        if (best < 0 || cost < best) { best = cost; bi = i; bj = j; }
      }
    if ((int32_t)boxes.size() <= max_rects && best > merge_pixels) break;
    boxes[bi] = Bound(boxes[bi], boxes[bj]);
    boxes.erase(boxes.begin() + (ptrdiff_t)bj);
    Close(boxes);
    std::sort(boxes.begin(), boxes.end(), in_order);
  }
  std::vector<AnimRect> out;
  for (const Box& b : boxes) out.push_back(AnimRect{b.x0, b.y0, b.x1 - b.x0, b.y1 - b.y0});
  return out;
}

}  // namespace jxlhip
