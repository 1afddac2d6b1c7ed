// The plan of an animation decode: which consecutive codestream frames form a chunk - one pass through the batched
// entropy and pixel stages and one compose launch - and which reference slots are alive where one chunk ends and the next begins.
// Host arithmetic only: no HIP calls, so the CPU suite checks it (tests/test_animation_plan.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "host_parse.h"

namespace jxlhip {

// Scratch a chunk may take before it is cut: the sum of its frames' scratch as BuildBatch measures each on its own (workspace and
// uploaded tables; the planes that the frames of a batch share in the pixel stages count once per frame, so the sum is an upper bound).
// A frame larger than this is a chunk of its own.  16 GiB: a 4K RGBA lossy frame measures 0.49 GB and a lossless one 0.17 GB, so 32
// of the former decode side by side and the frame limit cuts the latter - a chunk costs the latency of its longest serial entropy
// chain whatever its size, so chunks should be as large as the memory allows.
constexpr size_t kAnimChunkScratch = (size_t)16 << 30;

struct AnimChunk {
  int first = 0, count = 0;           // codestream frames [first, first + count)
  int first_shown = 0, shown = 0;     // displayed images [first_shown, first_shown + shown) are completed inside it
  int live_in = 0, live_out = 0;      // bit s: slot s is loaded at entry / stored at exit
};

struct AnimPlan {
  std::vector<size_t> scratch;   // per frame
  // per frame k: the slots alive at a cut right behind it: written by a frame up to k, and read by a later frame before any frame
  // between overwrites them.  A dead slot costs no bytes.
  std::vector<int> live_after;
};

// What one frame costs in a batch of its own: BuildBatch's measuring pass (blob + workspace bytes).
size_t FrameScratchBytes(ParsedFrame& f);
AnimPlan PlanAnimation(Animation& a);
// The chunk that starts at frame `first` when displayed images up to `last_shown` (inclusive) are asked for: it ends behind the frame
// that completes `last_shown`, after kMaxLayerFrames frames (chunk_frames >= 1: after that many, if fewer), or in front of the frame
// that would take its scratch past scratch_budget (the decoder passes kAnimChunkScratch), whichever comes first; it always holds one
// frame, however large.
AnimChunk NextChunk(const Animation& a, const AnimPlan& p, int first, int last_shown, int chunk_frames, size_t scratch_budget);

}  // namespace jxlhip
