// k_predict: score raw features through the flat forest (forest_view.h). One thread per row; X is column-major fp32
// [F][N], so adjacent lanes read adjacent rows of a feature. Per tree, in forest order: from roots[t] follow
// forest_go_left to a leaf (feat < 0), then out[row][cls[t]] += value[leaf] in fp32 and, when asked for,
// leaf_out[row][t] = the leaf's node index. No LDS, no atomics: a row's cells belong to its thread.
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_predict: 14 VGPR, 56 SGPR, 0 bytes of scratch, 0 spills, no LDS, occupancy 8 waves per SIMD
#include <hip/hip_runtime.h>

#include "forest_view.h"

namespace {

__global__ void k_predict(const float* __restrict__ X, long long N, int K, ForestView fv, float* __restrict__ out,
                          int* __restrict__ leaf_out /*nullable [N][n_trees]*/) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= N) return;
  for (int t = 0; t < fv.n_trees; ++t) {
    int n = fv.roots[t];
    while (fv.feat[n] >= 0) {
      const float x = X[(long long)fv.feat[n] * N + row];
      n = forest_go_left(fv, n, x) ? fv.left[n] : fv.right[n];
    }
    out[row * K + fv.cls[t]] += fv.value[n];
    if (leaf_out) leaf_out[row * fv.n_trees + t] = n;
  }
}

}  // namespace

extern "C" {

// X: float32 [F][N]; fv: the flat forest (host pointer, read here); out: float32 [N][K], accumulated into;
// leaf_out: int32 [N][n_trees] or null.
int h2o_predict(const void* X, long long N, int K, const ForestView* fv, void* out, void* leaf_out, hipStream_t s) {
  const int blk = 256;
  const long long grid = (N + blk - 1) / blk;
  hipLaunchKernelGGL(k_predict, dim3((unsigned)grid), dim3(blk), 0, s, (const float*)X, N, K, *fv, (float*)out,
                     (int*)leaf_out);
  return (int)hipGetLastError();
}

}  // extern "C"
