// Host-side check of the batch layout under a sanitizer: parses the .jxl files named on the command line, plans them as one batch and
// each alone, and runs BuildBatch measuring and then placing, the blob in a heap buffer of exactly the measured size (the workspace,
// the output buffers and the static tables get fake bases that are never dereferenced).  No GPU, no HIP runtime call.  Build, from the
// repository root (see profiles/batch_layout_host_asan.txt):
//   clang++ -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -I<rocm>/include -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//     tools/batch_layout_check.cc pdn_jpegxl_amd/csrc/{batch_layout,entropy_plan,host_parse,icc}.cc -o batch_layout_check
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../include/jxlfiletypeio.h"
#include "../pdn_jpegxl_amd/csrc/batch_layout.h"

using namespace jxlhip;

static int Check(const std::vector<std::vector<uint8_t>>& files, int downscale, bool debug_taps) {
  const int n = (int)files.size();
  std::vector<ParsedFrame> frames((size_t)n);
  std::vector<int> status((size_t)n, DecoderStatus_Ok);
  for (int i = 0; i < n; i++) {
    try {
      ParseFile(files[i].data(), files[i].size(), false, frames[i]);
      if (frames[i].layers) status[i] = DecoderStatus_DecodeError;   // (layered files are expanded by the decoder, not here)
    } catch (const std::exception&) {
      status[i] = DecoderStatus_DecodeError;
    }
  }
  EntropyPlanOptions o;
  o.downscale = downscale;
  const EntropyPlan plan = PlanEntropy(frames, status, o);
  std::vector<uint8_t*> dev_out((size_t)n);
  for (int i = 0; i < n; i++) dev_out[i] = (uint8_t*)(((uintptr_t)3 << 44) + ((uintptr_t)i << 34));
  const uint16_t* d_natural[kNumOrders]; const U32x2* d_scan[kNumQuantTables]; const float* d_dq[kNumQuantTables]; uint32_t dq_n[kNumQuantTables];
  for (int k = 0; k < kNumOrders; k++) d_natural[k] = (const uint16_t*)(((uintptr_t)4 << 44) + ((uintptr_t)k << 24));
  for (int q = 0; q < kNumQuantTables; q++) {
    d_scan[q] = (const U32x2*)(((uintptr_t)4 << 44) + ((uintptr_t)(64 + q) << 24)); d_dq[q] = (const float*)(((uintptr_t)4 << 44) + ((uintptr_t)(128 + q) << 24));
    dq_n[q] = (uint32_t)(GetStaticTables().dq[q].size() / 3);
  }
  const std::vector<Composite> comps;
  const std::vector<int> file_of;
  const std::vector<ParsedFrame> layered;
  BatchInput in;
  in.frames = &frames; in.parse_status = &status; in.plan = &plan;
  in.dev_out = dev_out.data();
  in.comps = &comps; in.file_of = &file_of; in.files = &layered; in.nfiles = n;
  in.d_natural = d_natural; in.d_scan = d_scan; in.d_dq = d_dq; in.dq_n = dq_n;
  in.ds = downscale == 8; in.debug_taps = debug_taps;
  BatchRegions M;
  BatchOutput unplaced;
  BuildBatch(in, M, unplaced);
  uint8_t* blob = (uint8_t*)calloc(1, M.blob.off ? M.blob.off : 1);
  BatchRegions R{Region(blob, blob, M.blob.off), Region(nullptr, (const void*)((uintptr_t)1 << 44), M.zero.off), Region(nullptr, (const void*)((uintptr_t)2 << 44), M.ws.off),
                 Region(nullptr, (const void*)((uintptr_t)5 << 44), M.pix.off)};
  BatchOutput B;
  BuildBatch(in, R, B);
  const bool same = R.blob.off == M.blob.off && R.zero.off == M.zero.off && R.ws.off == M.ws.off && R.pix.off == M.pix.off;
  int decoded = 0;
  for (int s : status) decoded += s == DecoderStatus_Ok;
  printf("  %d files (%d laid out), downscale %d, debug_taps %d: blob %zu B, zeroed %zu B, per-image workspace %zu B, chunk planes %zu B, %zu records; the passes %s\n", n, decoded, downscale,
         (int)debug_taps, M.blob.off, M.zero.off, M.ws.off, M.pix.off, B.imgs.size(), same ? "agree" : "DISAGREE");
  free(blob);
  return same ? 0 : 1;
}

int main(int argc, char** argv) {
  std::vector<std::vector<uint8_t>> files;
  for (int a = 1; a < argc; a++) {
    FILE* fp = fopen(argv[a], "rb");
    if (!fp) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
    std::vector<uint8_t> bytes;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), fp)) > 0;) bytes.insert(bytes.end(), buf, buf + k);
    fclose(fp);
    files.push_back(std::move(bytes));
  }
  int bad = 0;
  for (int ds : {1, 8})
    for (bool taps : {false, true}) {
      if (ds == 8 && taps) continue;
      bad += Check(files, ds, taps);
      for (const auto& f : files) bad += Check({f}, ds, taps);
    }
  printf("%s\n", bad ? "FAILED" : "clean");
  return bad ? 1 : 0;
}
