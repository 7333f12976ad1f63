// vsg_block_tree.h -- the reduction tree of the bundle adjustments' and the essential graph's kernels, ONE copy
// (vsg_ba_kernels.inc and vsg_essential_graph.hip include it; vsg_pose.hip and vsg_sim3_opt.hip keep the trees of their
// in-workgroup solvers).
#pragma once
#include "vsg_pose_opt.h"

namespace vsg {

// the fixed tree of vsg_pose_opt.h over one workgroup of pose::kThreads lanes: butterfly over the wave, the waves serially
template <int N, bool kMax>
__device__ __forceinline__ void block_tree(double *acc, double *lds) {
  const int lane = threadIdx.x & (pose::kWave - 1), wave = threadIdx.x / pose::kWave;
#pragma unroll
  for (int k = 0; k < N; k++) {
    double v = acc[k];
#pragma unroll
    for (int s = 1; s < pose::kWave; s <<= 1) {
      const double o = __shfl_xor(v, s, pose::kWave);
      v = kMax ? (v < o ? o : v) : v + o;
    }
    acc[k] = v;
  }
  __syncthreads();  // the previous tree's readers are done with lds
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) lds[wave * N + k] = acc[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++) {
    double t = lds[k];
#pragma unroll
    for (int w = 1; w < pose::kWaves; w++) {
      const double o = lds[w * N + k];
      t = kMax ? (t < o ? o : t) : t + o;
    }
    acc[k] = t;
  }
}

}  // namespace vsg
