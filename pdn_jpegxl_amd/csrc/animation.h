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
  // of the images completed inside it, those that are stored: first_stored, first_stored + step, ... (`stored` of them; the others are
  // decoded for the slots only, ComposeFrame::show -1).  first_stored is -1 when there is none.
  int first_stored = -1, stored = 0, step = 1;
};

// Where an animation decode stands: the chunk that runs next starts at codestream frame `frame` (every frame in front of it has been
// decoded into the slots), and the next image that is delivered is `shown`.  `shown` may lie behind the image that `frame` belongs
// to: a seek is lazy, and the images in between are decoded for the slots together with the images then asked for.
struct AnimCursor {
  int frame = 0, shown = 0;
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
// frame, however large.  Of the images it completes it stores those from `first_stored` on, every `step`-th one (the defaults: all).
AnimChunk NextChunk(const Animation& a, const AnimPlan& p, int first, int last_shown, int chunk_frames, size_t scratch_budget, int first_stored = 0,
                    int step = 1);

// Random access.  Displayed image j is an entry point when it is image 0 or no slot is alive in front of its
// first frame (live_after[first frame - 1] == 0): the kernel starts every slot at zero, so a decode that starts there computes what the
// sequential one does.  Ascending.
std::vector<int> EntryPoints(const Animation& a, const AnimPlan& p);
// The first codestream frame of displayed image j (j == number of displayed images: the number of frames), and the displayed image
// that codestream frame k belongs to.
int FirstFrame(const Animation& a, int j);
int ImageOfFrame(const Animation& a, int k);
// Moves the cursor so that image j is delivered next (j == number of displayed images: the end); false, and the cursor as it was,
// when j is out of range.  j == cur.shown changes nothing.  Otherwise decoding resumes at the latest entry point e <= j, unless the
// image the cursor's frame belongs to lies in [e, j]: then it goes on from where it stands - a forward seek never goes back.
bool SeekCursor(const Animation& a, const std::vector<int>& entry_points, AnimCursor& cur, int j);
// How many images a request for `count` images, every step-th from the cursor on, delivers: min(count, ceil((total - shown) / step)).
int SelectedImages(const Animation& a, const AnimCursor& cur, int count, int step);

// Delivers n images, every step-th from cur.shown on (n <= SelectedImages): the chunks from cur.frame up to the frame that completes
// the last of them, each handed to run(chunk, images of the request stored before it).  The frames between the cursor's frame and the
// first image asked for travel in the same chunks and store nothing.  When run returns false the cursor stays in front of that chunk,
// with `shown` at the first image not yet delivered, and the result is false.
template <class Run>
bool DeliverImages(const Animation& a, const AnimPlan& p, AnimCursor& cur, int n, int step, int chunk_frames, size_t scratch_budget, Run&& run) {
  if (n <= 0) return true;
  const int first = cur.shown, last = first + (n - 1) * step;
  int done = 0;
  while (ImageOfFrame(a, cur.frame) <= last) {
    const AnimChunk c = NextChunk(a, p, cur.frame, last, chunk_frames, scratch_budget, first + done * step, step);
    if (!run(c, done)) return false;
    cur.frame += c.count;
    done += c.stored;
    cur.shown = first + done * step;
  }
  const int total = (int)a.completes.size();
  cur.shown = first + n * step < total ? first + n * step : total;
  return true;
}

}  // namespace jxlhip
