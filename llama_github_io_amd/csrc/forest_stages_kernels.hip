// Per-tree and per-feature by-products of the forest walk (gfx950): for every row of X, walk every tree of the flat
// forest (forest_view.h) ONCE, in forest order, and write any subset of three outputs (a null pointer = not asked):
//
//   stage[T][N] fp32: cell (t, i) = the running sum, from 0.0f, of value[leaf] over the trees t' <= t with
//     cls[t'] == cls[t], one fp32 add per tree in forest order: bit for bit column cls[t] of k_predict
//     (predict_kernels.hip) over the trees [0, t + 1) of the view (staged predictions).
//   leaf[T][N] int32: the flat node index of the leaf row i reaches in tree t: k_predict's leaf_out, transposed
//     (leaf node assignment).
//   freq[F][N] int32: how many split nodes on row i's T paths split on feature f (feature frequencies).
//
// Layout: all three are tree-major / feature-major, so the 64 lanes of a wave store 64 adjacent cells of one
// column (k_predict's leaf_out[N][T] has the lanes n_trees ints apart); X is read column-major [F][N] as in k_predict.
//
// k_forest_stages: one lane owns one row, a block is ONE wave (64 rows). Every split is decided by forest_go_left.
//   The running sum is one register: a launch with `sliced` set has grid z = K and block z walks only the trees of
//   class z (as k_predict_permuted does), so across the slices every tree is still walked once per row and no
//   accumulator is indexed by a run-time class. An unsliced launch (grid z = 1) walks every tree; the launcher uses
//   it when no stage is asked for, and for the frequency counters of a forest with K > 1, which must see every tree
//   exactly once: the launcher then makes two launches (sliced: stage and leaf; unsliced: freq), never atomics across
//   slices. With K == 1 one launch writes everything.
//   Frequency counters (template parameter FREQ): 1 = a lane-owned LDS column cnt[F][64] (int32, lane-contiguous:
//   bank = lane mod 32, conflict free), zeroed by the lane, bumped per split, stored to freq[f][row] at the end;
//   2 = the global cells freq[f][row] themselves (zeroed by the lane, then own-cell read-modify-write; coalesced
//   like every other access here). The launcher picks 1 while F * 256 bytes fit under the byte cap it is given
//   (ops/forest.py: STAGES_FREQ_LDS_BYTES), never above 64 KiB, else 2. Either way every cell of freq is written.
//   A cell belongs to one thread: no atomics and NO barrier, so a lane with row >= N leaves at once.
//
// LDS budget: F * 256 bytes of dynamic LDS with FREQ == 1 (F = 28: 7,168 bytes = 22 blocks = 22 waves per CU of
// 160 KiB; the default cap of 16 KiB, F <= 64, still leaves 10 waves per CU), none otherwise.
// Indexing: t * N + row and f * N + row in 64 bits (T * N passes 2^31 at workload sizes).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_forest_stages<0>: 16 VGPR, 60 SGPR, 0 bytes of scratch, 0 spills, no LDS, occupancy 8 waves per SIMD
//   k_forest_stages<1>: 26 VGPR, 66 SGPR, 0 bytes of scratch, 0 spills, dynamic LDS only, occupancy by registers 8
//   k_forest_stages<2>: 20 VGPR, 62 SGPR, 0 bytes of scratch, 0 spills, no LDS, occupancy 8 waves per SIMD
#include <hip/hip_runtime.h>

#include "forest_view.h"

namespace {

constexpr int FS_ROWS = 64;             // rows per block: one wave
constexpr int FS_MAX_LDS = 64 << 10;    // dynamic LDS per block at most

template <int FREQ>                     // 0: no frequencies, 1: counters in LDS, 2: counters in freq itself
__global__ __launch_bounds__(FS_ROWS) void k_forest_stages(
    const float* __restrict__ X, long long N, int F, ForestView fv, int sliced, float* __restrict__ stage /*[T][N]*/,
    int* __restrict__ leaf /*[T][N]*/, int* __restrict__ freq /*[F][N]*/) {
  extern __shared__ int cnt_lds[];        // FREQ == 1: cnt [F][FS_ROWS]
  const int lane = threadIdx.x;
  const long long row = (long long)blockIdx.x * FS_ROWS + lane;
  if (row >= N) return;                   // no barrier in this kernel: a lane may leave
  const int cls = blockIdx.z;
  int* cnt = cnt_lds + lane;
  if (FREQ == 1) for (int f = 0; f < F; ++f) cnt[f * FS_ROWS] = 0;
  if (FREQ == 2) for (int f = 0; f < F; ++f) freq[(long long)f * N + row] = 0;

  float acc = 0.0f;
  for (int t = 0; t < fv.n_trees; ++t) {
    if (sliced && fv.cls[t] != cls) continue;
    int n = fv.roots[t];
    int f = fv.feat[n];
    while (f >= 0) {
      if (FREQ == 1) cnt[f * FS_ROWS] += 1;
      if (FREQ == 2) freq[(long long)f * N + row] += 1;
      n = forest_go_left(fv, n, X[(long long)f * N + row]) ? fv.left[n] : fv.right[n];
      f = fv.feat[n];
    }
    acc += fv.value[n];
    if (stage) stage[(long long)t * N + row] = acc;
    if (leaf) leaf[(long long)t * N + row] = n;
  }
  if (FREQ == 1) for (int f = 0; f < F; ++f) freq[(long long)f * N + row] = cnt[f * FS_ROWS];
}

int launch(int mode, unsigned tiles, unsigned z, hipStream_t s, const float* X, long long N, int F,
           const ForestView& fv, float* stage, int* leaf, int* freq) {
  const dim3 grid(tiles, 1, z), blk(FS_ROWS);
  const int sliced = z > 1;
  if (mode == 0)
    hipLaunchKernelGGL(k_forest_stages<0>, grid, blk, 0, s, X, N, F, fv, sliced, stage, leaf, (int*)nullptr);
  else if (mode == 1)
    hipLaunchKernelGGL(k_forest_stages<1>, grid, blk, (size_t)F * FS_ROWS * sizeof(int), s, X, N, F, fv, sliced, stage,
                       leaf, freq);
  else
    hipLaunchKernelGGL(k_forest_stages<2>, grid, blk, 0, s, X, N, F, fv, sliced, stage, leaf, freq);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// X: float32 [F][N]; fv: the flat forest (host pointer, read here) of T = n_trees trees, classes in [0, K), splitting
// on features < F only (the caller checks). stage: float32 [T][N], leaf: int32 [T][N], freq: int32 [F][N]; each may
// be null, every cell of the others is written. freq_lds_bytes: the frequency counters live in LDS while
// F * 256 bytes fit under it (and under 64 KiB), in freq itself past it.
int h2o_forest_stages(const void* X, long long N, int K, int F, const ForestView* fv, int freq_lds_bytes, void* stage,
                      void* leaf, void* freq, hipStream_t s) {
  if (N <= 0 || fv->n_trees <= 0 || fv->n_nodes <= 0 || (!stage && !leaf && !freq)) return 0;
  const long long tiles = (N + FS_ROWS - 1) / FS_ROWS;
  if (K <= 0 || K > 65535 || F <= 0 || tiles > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const long long cnt_bytes = (long long)F * FS_ROWS * (long long)sizeof(int);
  const int fmode = !freq ? 0 : (cnt_bytes <= freq_lds_bytes && cnt_bytes <= FS_MAX_LDS) ? 1 : 2;
  if (!stage || K == 1)       // one launch: nothing to slice (no stage), or one slice is the whole forest
    return launch(fmode, (unsigned)tiles, stage ? (unsigned)K : 1u, s, (const float*)X, N, F, *fv, (float*)stage,
                  (int*)leaf, (int*)freq);
  const int e = launch(0, (unsigned)tiles, (unsigned)K, s, (const float*)X, N, F, *fv, (float*)stage, (int*)leaf,
                       nullptr);
  if (e != 0 || !freq) return e;
  return launch(fmode, (unsigned)tiles, 1u, s, (const float*)X, N, F, *fv, nullptr, nullptr, (int*)freq);
}

}  // extern "C"
