// Workspace layout of a batch encode: a pure host function (no HIP call), so the CPU suite checks it (csrc/selftest.cc).
#include "enc_batch_layout.h"
#include <cstring>

namespace jxlhip {

void SetEncGeometry(uint32_t w, uint32_t h, EncImage& im) {
  memset(&im, 0, sizeof(im));
  im.w = (int32_t)w; im.h = (int32_t)h;
  im.w8 = (int32_t)((w + 7) / 8); im.h8 = (int32_t)((h + 7) / 8);
  im.wp = im.w8 * 8; im.hp = im.h8 * 8;
  im.xg = (int32_t)((w + 255) / 256); im.yg = (int32_t)((h + 255) / 256); im.ng = im.xg * im.yg;
  im.xlf = (int32_t)((w + 2047) / 2048); im.ylf = (int32_t)((h + 2047) / 2048); im.nlf = im.xlf * im.ylf;
}

namespace {

constexpr size_t kAlign = 256;   // what hipMalloc gives the single-image path: the loaders of encode_kernels.hip rely on it
size_t Up(size_t v) { return (v + kAlign - 1) & ~(kAlign - 1); }

// Hands out pieces of the workspace: bulk buffers from the body, counters from the region of their kind in the head.
struct Carver {
  uint8_t* base;
  size_t body;
  size_t head[kNumEncCounterKinds];
  template <class T> T* At(size_t& cursor, size_t count) {
    cursor = Up(cursor);
    T* p = (T*)((uintptr_t)base + cursor);
    cursor += std::max<size_t>(count * sizeof(T), kAlign);
    return p;
  }
  template <class T> T* Get(size_t count) { return At<T>(body, count); }
  template <class T> T* Counter(EncCounterKind kind, size_t count) { return At<T>(head[kind], count); }
};

// one pass over the batch; `start`: where the regions begin (all zero: the pass only measures the regions)
void Pass(const EncBatchItem* items, int n, uint8_t* base, const size_t* start, size_t body_start, EncImage* ims, EncBatchLayout* lay, Carver* end) {
  Carver c;
  c.base = base;
  for (int k = 0; k < kNumEncCounterKinds; k++) c.head[k] = start[k];
  c.body = body_start;
  lay->slots.assign((size_t)n, EncBatchSlot());
  lay->total_sections = 0;
  for (int i = 0; i < n; i++) {
    const EncBatchItem& it = items[i];
    EncImage& im = ims[i];
    EncBatchSlot& sl = lay->slots[(size_t)i];
    SetEncGeometry(it.w, it.h, im);
    im.gray = it.nch < 3;
    im.has_alpha = (it.nch & 1) ? 0 : 1;
    im.lossless = it.lossless ? 1 : 0;
    im.cfl = (!it.lossless && it.cfl) ? 1 : 0;
    sl.begin = Up(c.body);
    sl.src = (size_t)((uintptr_t)c.Get<uint8_t>((size_t)it.w * it.nch * it.sample_bytes * it.h) - (uintptr_t)base);
    sl.surface = it.sample_bytes == 1 ? (size_t)((uintptr_t)c.Get<uint8_t>((size_t)it.w * 4 * it.h) - (uintptr_t)base) : sl.src;
    if (im.lossless) {
      im.ll_nch = (im.gray ? 1 : 3) + im.has_alpha;
      LayLosslessPlanes(c, im);
      im.hist_mod = c.Counter<uint32_t>(kEncHist, kNumEncLeaves * kEncSyms);
      LayLosslessSections(c, im);
    } else {
      LayLossyPlanes(c, im);
      LayLossyCoding(c, im);
    }
    sl.end = c.body;
    lay->total_sections += (size_t)EncNumSections(im);
  }
  *end = c;
}

}  // namespace

void LayEncBatch(const EncBatchItem* items, int n, uint8_t* base, EncImage* ims, EncBatchLayout* lay) {
  // the regions' sizes, then the same pass from where the regions begin
  const size_t zero[kNumEncCounterKinds] = {0, 0, 0};
  Carver m;
  Pass(items, n, nullptr, zero, 0, ims, lay, &m);
  size_t pos = 0;
  for (int k = 0; k < kNumEncCounterKinds; k++) { lay->region[k] = pos; pos = Up(pos + m.head[k]); }
  lay->region[kNumEncCounterKinds] = lay->head_bytes = pos;
  size_t lossy = 0;
  for (int i = 0; i < n; i++) lossy += items[i].lossless ? 0 : 1;
  lay->tables = pos; pos = Up(pos + kEncBatchTables * 3 * EncBatchTableStride(n));
  lay->records_m = pos; pos = Up(pos + (size_t)n * sizeof(EncImage));
  lay->mcodes = pos; pos = Up(pos + (size_t)n * kEncModCodeBytes);
  lay->records_a = pos; pos = Up(pos + (size_t)n * sizeof(EncImage));
  lay->acodes = pos; pos = Up(pos + lossy * kEncHfCodeBytes);
  lay->dst_off = pos; pos = Up(pos + (lay->total_sections + 1) * 8);
  lay->body = pos;
  Carver e;
  Pass(items, n, base, lay->region, pos, ims, lay, &e);
  lay->total_bytes = Up(e.body);
}

}  // namespace jxlhip
