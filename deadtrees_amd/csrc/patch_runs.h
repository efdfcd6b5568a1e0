// Shared by the kernels that walk a label plane in 64-pixel chunks (patches.hip, attributes.hip): the defensive read of a
// caller's label and the runs of equal labels inside a wave.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

// a label plane handed in by a caller: whatever is no label of an n-pixel plane counts as background, so that no index
// derived from it leaves the planes
__device__ __forceinline__ int pt_label_at(const int32_t* __restrict__ labels, int64_t i, int64_t n) {
  if (i >= n) return 0;
  const int label = labels[i];
  return label > 0 && label <= n ? label : 0;
}

// ---------------------------------------------------------------- runs of equal labels in a wave
// head: this lane starts a run (lane 0, another label than the lane before, or `brk`); len: the run's length, valid in
// head lanes; heads: the ballot of head
__device__ __forceinline__ void pt_runs(int label, bool brk, int lane, bool& head, int& len, uint64_t& heads) {
  const int prev = __shfl_up(label, 1, 64);
  head = lane == 0 || prev != label || brk;
  heads = __ballot(head);
  const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
  len = above ? __ffsll((long long)above) : 64 - lane;
}
