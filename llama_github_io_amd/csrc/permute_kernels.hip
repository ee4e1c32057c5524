// Permutation importance on device (gfx950): score every row of X through the forest once per VARIANT, where
// variant j sees X[feats[j]][src[j][i]] in place of X[feats[j]][i] for row i (one feature shuffled, the others
// the row's own; feats may repeat, src need not be a permutation). out[J][N][K] (fp32): cell (j, i, c) is the sum,
// over the trees of class c in forest order, of the leaf that row i reaches under variant j: bit for bit what
// k_predict (predict_kernels.hip) gives on a copy of X whose row feats[j] was overwritten with X[feats[j]][src[j]]:
// both walks decide every split with forest_go_left (forest_view.h) and every cell takes exactly one fp32 add per
// tree, in forest order, from 0.0f.
//
// Down a row's own path only the splits on feature f can send a variant that shuffles f elsewhere, and a depth-6
// path meets at most 6 features, so most (variant, row, tree) triples share the row's own leaf. The walk forks
// where a variant diverges instead of repeating itself per variant:
//
// k_predict_permuted: one lane owns one row, a block is ONE wave (64 rows), one chunk of at most 64 variants and
//   one class (grid = row tiles x chunks x K). Prologue: the lane zeroes its accumulators and gathers its
//   shuffled values xv[j] = X[feats[j] * N + src[j * N + row]] once (src is read coalesced, the gather is the only
//   uncoalesced read and happens once per (variant, row), not once per split). Per tree of the block's class the
//   lane walks its own path with its own X values (coalesced as in k_predict) and keeps a 64-bit set pend of the
//   variants still on that path. At a split on f it takes the variants of fmask[chunk][f] & pend (fmask: bit j =
//   "variant j of the chunk shuffles f", built on the host); a variant whose forest_go_left(xv[j]) disagrees with
//   the row's own decision leaves pend, is walked from the OTHER child to its leaf (xv[j] at later splits on f,
//   the row's X elsewhere) and takes that leaf's value. At the row's own leaf every variant left in pend takes its
//   value.
//
// LDS: two fp32 arrays [variant][lane], acc then xv (lane-contiguous: bank = lane mod 32, conflict free; a column
// is touched only by its owning lane, so plain read-modify-write, no atomics and NO barrier: a lane with
// row >= N may leave at once). Dynamic, 512 bytes per variant of the launch's largest chunk: 32,768 bytes at 64
// variants = 5 blocks = 5 waves per CU (of 160 KiB); 8,192 bytes at 16 variants = 20 waves per CU. The chunk size
// is a launch argument (at most 64, the width of a mask). ops/forest.py passes 16: at 100,000 rows x 140 variants
// 6.6 ms against 11.5 ms at 64 (the row's own walk is repeated per chunk, but four times the waves hide its
// loads), never more than 2 % behind 64 at 10,000 to 1,000,000 rows (profiles/permvi_gpu.md).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_predict_permuted: 36 VGPR, 78 SGPR, 0 bytes of scratch, 0 spills, occupancy by registers 8 waves per SIMD
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "forest_view.h"

namespace {

constexpr int PV_MAX_CHUNK = 64;        // variants per chunk at most: one bit each of a feature mask
constexpr int PV_ROWS = 64;             // rows per block: one wave

__global__ __launch_bounds__(PV_ROWS) void k_predict_permuted(
    const float* __restrict__ X, long long N, int K, int F, ForestView fv, const int* __restrict__ feats /*[J]*/,
    const int* __restrict__ src /*[J][N]*/, long long J, long long j_begin, int chunk,
    const unsigned long long* __restrict__ fmask /*[chunks of J][F]*/, float* __restrict__ out /*[J][N][K]*/) {
  extern __shared__ float lds[];          // acc [jmax][PV_ROWS], then xv [jmax][PV_ROWS]; jmax = the launch's largest chunk
  const int lane = threadIdx.x;
  const long long row = (long long)blockIdx.x * PV_ROWS + lane;
  const long long j0 = j_begin + (long long)blockIdx.y * chunk;
  const int jc = (int)((J - j0) < (long long)chunk ? (J - j0) : (long long)chunk);
  const int jmax = (int)((J - j_begin) < (long long)chunk ? (J - j_begin) : (long long)chunk);
  const int cls = blockIdx.z;
  if (row >= N || jc <= 0) return;        // no barrier in this kernel: a lane may leave
  const unsigned long long full = jc >= 64 ? ~0ull : ((1ull << jc) - 1ull);
  const unsigned long long* fm = fmask + (j0 / chunk) * (long long)F;
  float* a = lds + lane;
  float* xv = lds + jmax * PV_ROWS + lane;
  for (int j = 0; j < jc; ++j) {
    a[j * PV_ROWS] = 0.0f;
    xv[j * PV_ROWS] = X[(long long)feats[j0 + j] * N + src[(j0 + j) * N + row]];
  }

  for (int t = 0; t < fv.n_trees; ++t) {
    if (fv.cls[t] != cls) continue;
    unsigned long long pend = full;
    int n = fv.roots[t];
    int f = fv.feat[n];
    while (f >= 0) {
      const bool go_left = forest_go_left(fv, n, X[(long long)f * N + row]);
      unsigned long long m = fm[f] & pend;
      while (m) {
        const int j = __ffsll((unsigned long long)m) - 1;
        m &= m - 1ull;
        const float xj = xv[j * PV_ROWS];
        if (forest_go_left(fv, n, xj) == go_left) continue;
        pend &= ~(1ull << j);
        int d = go_left ? fv.right[n] : fv.left[n];
        int df = fv.feat[d];
        while (df >= 0) {
          const float x = df == f ? xj : X[(long long)df * N + row];
          d = forest_go_left(fv, d, x) ? fv.left[d] : fv.right[d];
          df = fv.feat[d];
        }
        a[j * PV_ROWS] += fv.value[d];
      }
      n = go_left ? fv.left[n] : fv.right[n];
      f = fv.feat[n];
    }
    const float v = fv.value[n];
    while (pend) {
      const int j = __ffsll((unsigned long long)pend) - 1;
      a[j * PV_ROWS] += v;
      pend &= pend - 1ull;
    }
  }
  for (int j = 0; j < jc; ++j) out[((j0 + j) * N + row) * K + cls] = a[j * PV_ROWS];
}

}  // namespace

extern "C" {

// X: float32 [F][N]; fv: the flat forest (host pointer, read here), splitting on features < F only; feats: int32
// [J], every one in [0, F); src: int32 [J][N], every one in [0, N) (the caller checks both: the kernel reads
// X[feats[j] * N + src[j][i]] unguarded). fmask: uint64 [ceil(J / chunk)][F], bit b of fmask[c][f] = variant
// c * chunk + b shuffles f. out: float32 [J][N][K], every cell is written. Variants go in launches of at most
// max_chunks chunks of `chunk` (1 ... 64) variants.
int h2o_predict_permuted(const void* X, long long N, int K, int F, const ForestView* fv, const void* feats,
                         const void* src, long long J, const void* fmask, int chunk, int max_chunks, void* out,
                         hipStream_t s) {
  if (N <= 0 || J <= 0 || fv->n_trees <= 0 || fv->n_nodes <= 0) return 0;
  const long long tiles = (N + PV_ROWS - 1) / PV_ROWS;
  if (K <= 0 || K > 65535 || F <= 0 || chunk <= 0 || chunk > PV_MAX_CHUNK || max_chunks <= 0 ||
      tiles > 0x7fffffffLL || !fmask) return (int)hipErrorInvalidValue;
  if (max_chunks > 65535) max_chunks = 65535;    // grid y
  const long long per_launch = (long long)max_chunks * chunk;
  for (long long j_begin = 0; j_begin < J; j_begin += per_launch) {
    const long long left_j = J - j_begin;
    const unsigned chunks = (unsigned)(((left_j < per_launch ? left_j : per_launch) + chunk - 1) / chunk);
    const size_t lds = (size_t)(left_j < chunk ? left_j : chunk) * PV_ROWS * 2 * sizeof(float);
    hipLaunchKernelGGL(k_predict_permuted, dim3((unsigned)tiles, chunks, (unsigned)K), dim3(PV_ROWS), lds, s,
                       (const float*)X, N, K, F, *fv, (const int*)feats, (const int*)src, J, j_begin, chunk,
                       (const unsigned long long*)fmask, (float*)out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
