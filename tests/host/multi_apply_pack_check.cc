// Stand-alone host check of PackMultiApply (kernels/hip/multi_apply_pack.h):
// no GPU, no HIP. Built with -fsanitize=address,undefined by
// tests/test_multi_apply_pack.py; exits 0 when every case holds.
//
// For each list of tensor sizes it replays the launches the way the kernel
// reads them (block -> slot -> tensor, chunk -> element range) and counts how
// often each element of each tensor is covered: exactly once, in every case.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kernels/hip/multi_apply_pack.h"

namespace {

int failures = 0;

#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      ++failures;                             \
      std::printf("FAIL %s: ", what);         \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
    }                                         \
  } while (0)

// Returns the number of launches.
int Check(const char* what, const std::vector<int64_t>& sizes,
          int want_launches = -1) {
  std::vector<std::vector<uint8_t>> seen(sizes.size());
  for (size_t t = 0; t < sizes.size(); ++t) seen[t].assign(sizes[t], 0);
  int launches = 0;
  int64_t blocks = 0;
  bool ok = PackMultiApply(
      sizes.data(), (int)sizes.size(), [&](const MultiApplyPlan& p) {
        ++launches;
        CHECK(p.num_tensors >= 1 && p.num_tensors <= kMultiApplyMaxTensors,
              "launch %d has %d tensors", launches, p.num_tensors);
        CHECK(p.num_blocks >= 1 && p.num_blocks <= kMultiApplyMaxBlocks,
              "launch %d has %d blocks", launches, p.num_blocks);
        std::vector<int> slot_used(kMultiApplyMaxTensors, 0);
        for (int b = 0; b < p.num_blocks; ++b) {
          int slot = p.block_tensor[b];
          CHECK(slot < p.num_tensors, "block %d: slot %d of %d", b, slot,
                p.num_tensors);
          if (slot >= p.num_tensors) continue;
          slot_used[slot] = 1;
          int t = p.tensor_index[slot];
          CHECK(t >= 0 && t < (int)sizes.size(), "slot %d: tensor %d", slot, t);
          if (t < 0 || t >= (int)sizes.size()) continue;
          // what the kernel does with (tensor, chunk)
          int64_t start = (int64_t)p.block_chunk[b] * kMultiApplyChunk;
          int64_t left = sizes[t] - start;
          CHECK(p.block_chunk[b] >= 0 && left > 0,
                "block %d: chunk %d of tensor %d starts outside it", b,
                p.block_chunk[b], t);
          if (p.block_chunk[b] < 0 || left <= 0) continue;
          int64_t n = left < kMultiApplyChunk ? left : kMultiApplyChunk;
          for (int64_t i = 0; i < n; ++i) ++seen[t][start + i];
          ++blocks;
        }
        for (int s = 0; s < p.num_tensors; ++s)
          CHECK(slot_used[s], "launch %d: slot %d has no block", launches, s);
      });
  CHECK(ok, "PackMultiApply refused");
  int64_t want_blocks = 0;
  for (size_t t = 0; t < sizes.size(); ++t) {
    want_blocks += (sizes[t] + kMultiApplyChunk - 1) / kMultiApplyChunk;
    int64_t bad = 0;
    for (uint8_t c : seen[t]) bad += c != 1;
    CHECK(bad == 0, "tensor %zu (%lld elements): %lld not covered once", t,
          (long long)sizes[t], (long long)bad);
  }
  CHECK(blocks == want_blocks, "%lld blocks, want %lld", (long long)blocks,
        (long long)want_blocks);
  if (want_launches >= 0)
    CHECK(launches == want_launches, "%d launches, want %d", launches,
          want_launches);
  std::printf("%-34s %4zu tensors %6lld blocks %3d launches\n", what,
              sizes.size(), (long long)blocks, launches);
  return launches;
}

}  // namespace

int main() {
  const int64_t C = kMultiApplyChunk;
  const int T = kMultiApplyMaxTensors, B = kMultiApplyMaxBlocks;

  Check("empty list", {}, 0);
  Check("only zero-element tensors", {0, 0, 0}, 0);
  Check("zero-element between others", {5, 0, 7, 0, 0, C + 1, 0}, 1);
  Check("single element", {1}, 1);
  Check("small odd sizes", {1, 7, 8, 255, 1024, 3 * 3 * 8 * 16}, 1);
  Check("exactly one chunk", {C}, 1);
  Check("ragged last chunk", {2 * C + 13}, 1);
  Check("one short of a chunk", {C - 1, C + 1}, 1);

  Check("exactly full tensor table", std::vector<int64_t>(T, 3), 1);
  Check("tensor table + 1", std::vector<int64_t>(T + 1, 3), 2);
  Check("tensor table + 5", std::vector<int64_t>(T + 5, 1), 2);
  Check("three tensor tables", std::vector<int64_t>(3 * T, 2), 3);
  {
    std::vector<int64_t> s(T + 5, 1);
    for (int i = 0; i < T + 5; i += 3) s[i] = 0;  // empties take no slot
    Check("tensor table + 5, a third empty", s, 1);
  }

  Check("exactly full block map", {(int64_t)B * C}, 1);
  Check("block map + 1 element", {(int64_t)B * C + 1}, 2);
  Check("block map full, ragged", {(int64_t)(B - 1) * C + 13}, 1);
  Check("tensor across a launch boundary", {(int64_t)(B - 2) * C, 3 * C + 13, 9},
        2);
  Check("boundary right after a tensor", {(int64_t)B * C, 5}, 2);
  Check("both tables fill together",
        [&] {
          std::vector<int64_t> s(T, 1);
          s[T - 1] = (int64_t)(B - T + 1) * C;  // last slot, last block
          s.push_back(4);
          return s;
        }(),
        2);

  // the shapes of a ResNet-50: 54 weights, then 107 small vectors
  {
    std::vector<int64_t> w = {7 * 7 * 3 * 64, 2048 * 1000};
    for (int64_t c : {64, 128, 256, 512})
      for (int i = 0; i < 13; ++i) w.push_back(3 * 3 * c * c + i);
    Check("resnet-like weights", w);
    Check("resnet-like vectors", std::vector<int64_t>(107, 257), 3);
  }

  // refused: nothing emitted
  {
    const char* what = "negative size";
    int64_t sizes[2] = {4, -1};
    int emitted = 0;
    bool ok = PackMultiApply(sizes, 2, [&](const MultiApplyPlan&) { ++emitted; });
    CHECK(!ok && emitted == 0, "ok=%d emitted=%d", (int)ok, emitted);
  }

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("all packing checks passed\n");
  return 0;
}
