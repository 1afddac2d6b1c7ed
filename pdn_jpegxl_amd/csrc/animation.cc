// Chunks and slot liveness of an animation decode (animation.h).
#include "animation.h"
#include <algorithm>
#include "../../include/jxlfiletypeio.h"
#include "batch_layout.h"
#include "entropy_plan.h"

namespace jxlhip {

size_t FrameScratchBytes(ParsedFrame& f) {
  std::vector<ParsedFrame> frames(1);
  std::swap(frames[0], f);
  const std::vector<int> status(1, DecoderStatus_Ok);
  size_t bytes = 0;
  try {
    const EntropyPlan plan = PlanEntropy(frames, status, EntropyPlanOptions());
    // measuring only: no address below is ever dereferenced
    const uint16_t* d_natural[kNumOrders] = {};
    const U32x2* d_scan[kNumQuantTables] = {};
    const float* d_dq[kNumQuantTables] = {};
    uint32_t dq_n[kNumQuantTables];
    for (int q = 0; q < kNumQuantTables; q++) dq_n[q] = (uint32_t)(GetStaticTables().dq[q].size() / 3);
    const uint8_t* dev_data[1] = {(const uint8_t*)256};   // the codestream is resident: none is uploaded with the frame
    uint8_t* dev_out[1] = {nullptr};
    const std::vector<Composite> comps;
    const std::vector<int> file_of(1, 0);
    const std::vector<ParsedFrame> files;
    BatchInput in;
    in.frames = &frames; in.parse_status = &status; in.plan = &plan;
    in.dev_data = dev_data; in.dev_out = dev_out;
    in.comps = &comps; in.file_of = &file_of; in.files = &files; in.nfiles = 1;
    in.d_natural = d_natural; in.d_scan = d_scan; in.d_dq = d_dq; in.dq_n = dq_n;
    BatchRegions measured;
    BatchOutput unplaced;
    BuildBatch(in, measured, unplaced);
    bytes = measured.blob.off + measured.WorkspaceBytes();
  } catch (...) {
    std::swap(frames[0], f);
    throw;
  }
  std::swap(frames[0], f);
  return bytes;
}

AnimPlan PlanAnimation(Animation& a) {
  AnimPlan p;
  const size_t n = a.frames.size();
  p.scratch.resize(n);
  for (size_t k = 0; k < n; k++) p.scratch[k] = FrameScratchBytes(a.frames[k]);
  // backwards: what is read behind frame k before it is overwritten; forwards: what has been written up to frame k
  p.live_after.assign(n, 0);
  int live = 0;
  for (size_t k = n; k-- > 0;) {
    p.live_after[k] = live;
    if (a.save[k] >= 0) live &= ~(1 << a.save[k]);
    live |= SlotsRead(a.frames[k], a.head.xsize, a.head.ysize);
  }
  int written = 0;
  for (size_t k = 0; k < n; k++) {
    if (a.save[k] >= 0) written |= 1 << a.save[k];
    p.live_after[k] &= written;
  }
  return p;
}

AnimChunk NextChunk(const Animation& a, const AnimPlan& p, int first, int last_shown, int chunk_frames, size_t scratch_budget, int first_stored,
                    int step) {
  AnimChunk c;
  c.step = step;
  const int n = (int)a.frames.size();
  const int cap = chunk_frames >= 1 ? std::min(chunk_frames, kMaxLayerFrames) : kMaxLayerFrames;
  c.first = first;
  c.first_shown = -1;
  c.live_in = first > 0 ? p.live_after[first - 1] : 0;
  size_t scratch = 0;
  for (int k = first; k < n && c.count < cap; k++) {
    if (c.count > 0 && scratch + p.scratch[k] > scratch_budget) break;
    scratch += p.scratch[k];
    c.count++;
    if (a.show[k] >= 0) {
      if (c.first_shown < 0) c.first_shown = a.show[k];
      c.shown++;
      if (a.show[k] >= first_stored && (a.show[k] - first_stored) % step == 0) {
        if (c.first_stored < 0) c.first_stored = a.show[k];
        c.stored++;
      }
      if (a.show[k] >= last_shown) break;
    }
  }
  if (c.first_shown < 0) c.first_shown = 0;
  c.live_out = p.live_after[first + c.count - 1];
  return c;
}

std::vector<int> EntryPoints(const Animation& a, const AnimPlan& p) {
  std::vector<int> e;
  for (int j = 0; j < (int)a.completes.size(); j++) {
    const int f = FirstFrame(a, j);
    if (f == 0 || p.live_after[f - 1] == 0) e.push_back(j);
  }
  return e;
}

int FirstFrame(const Animation& a, int j) {
  if (j <= 0) return 0;
  return j >= (int)a.completes.size() ? (int)a.frames.size() : a.completes[j - 1] + 1;
}

int ImageOfFrame(const Animation& a, int k) {
  return (int)(std::lower_bound(a.completes.begin(), a.completes.end(), k) - a.completes.begin());
}

bool SeekCursor(const Animation& a, const std::vector<int>& entry_points, AnimCursor& cur, int j) {
  if (j < 0 || j > (int)a.completes.size()) return false;
  if (j == cur.shown) return true;
  // (image 0 is always an entry point, so there is one at or in front of every j)
  const int e = *(std::upper_bound(entry_points.begin(), entry_points.end(), j) - 1);
  const int at = ImageOfFrame(a, cur.frame);
  if (!(e <= at && at <= j)) cur.frame = FirstFrame(a, e);
  cur.shown = j;
  return true;
}

int SelectedImages(const Animation& a, const AnimCursor& cur, int count, int step) {
  const int left = (int)a.completes.size() - cur.shown;
  return std::max(0, std::min(count, (left + step - 1) / step));
}

}  // namespace jxlhip
