// The project's one channel softmax: the loss and evaluation kernels of head_loss.hip and the probability histogram of
// curves.hip include it, so a probability is the same float wherever it is computed from the same logits.
#pragma once
#include <math.h>

// ---- downstream of the logits: ONE definition of every step the loss kernels and head_eval_kernel share
// Channel softmax: max, expf(z - max), sum in class order, times 1 / sum.  `p` may be `z` itself.
template <int K>
__device__ __forceinline__ void loss_softmax(const float (&z)[K], float (&p)[K]) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) m = fmaxf(m, z[k]);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    p[k] = expf(z[k] - m);
    sum += p[k];
  }
  const float inv = 1.f / sum;
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] = p[k] * inv;
}
