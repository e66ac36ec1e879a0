// Host-side packing for the multi-tensor optimizer kernels (optimizer.hip):
// a list of tensor sizes becomes as few launches as the fixed capacities
// allow. Each launch has a table of up to kMultiApplyMaxTensors tensors and a
// map of up to kMultiApplyMaxBlocks blocks; block b updates chunk
// block_chunk[b] (kMultiApplyChunk elements, the last one of a tensor maybe
// fewer) of tensor slot block_tensor[b]. A tensor that does not fit into what
// is left of a launch continues in the next one. Pure C++, no HIP: the
// stand-alone host check (tests/host/multi_apply_pack_check.cc) includes it.
#pragma once

#include <cstdint>

// 64 Ki elements per block: 512 threads x 32 four-element steps.
constexpr int64_t kMultiApplyChunk = 65536;
// Capacities: the kernel-argument struct built from a plan is
// 48 * 32 + 320 * 5 = 3136 bytes (static_assert in optimizer.hip), inside the
// 4 KB kernel-argument limit with the three scalar arguments on top.
constexpr int kMultiApplyMaxTensors = 48;
constexpr int kMultiApplyMaxBlocks = 320;

struct MultiApplyPlan {
  int num_tensors = 0;
  int tensor_index[kMultiApplyMaxTensors] = {};  // slot -> index into the list
  int num_blocks = 0;
  uint8_t block_tensor[kMultiApplyMaxBlocks] = {};  // block -> slot
  int32_t block_chunk[kMultiApplyMaxBlocks] = {};   // block -> chunk of tensor
};

// Calls emit(const MultiApplyPlan&) once per launch, in order. Tensors with
// no elements get no slot and no block. Returns false, having emitted
// nothing, if a size is negative or has more chunks than an int32 counts.
template <typename Emit>
bool PackMultiApply(const int64_t* sizes, int count, Emit&& emit) {
  static_assert(kMultiApplyMaxTensors <= 256, "block_tensor is a uint8_t");
  for (int t = 0; t < count; ++t)
    if (sizes[t] < 0 ||
        (sizes[t] + kMultiApplyChunk - 1) / kMultiApplyChunk > INT32_MAX)
      return false;
  MultiApplyPlan p;
  for (int t = 0; t < count; ++t) {
    int64_t chunks = (sizes[t] + kMultiApplyChunk - 1) / kMultiApplyChunk;
    int slot = -1;  // of tensor t in the launch being filled
    for (int64_t c = 0; c < chunks; ++c) {
      if (slot < 0) {
        if (p.num_tensors == kMultiApplyMaxTensors) {
          emit(p);
          p = MultiApplyPlan();
        }
        slot = p.num_tensors++;
        p.tensor_index[slot] = t;
      }
      p.block_tensor[p.num_blocks] = (uint8_t)slot;
      p.block_chunk[p.num_blocks] = (int32_t)c;
      if (++p.num_blocks == kMultiApplyMaxBlocks) {
        emit(p);
        p = MultiApplyPlan();
        slot = -1;
      }
    }
  }
  if (p.num_blocks > 0) emit(p);
  return true;
}
