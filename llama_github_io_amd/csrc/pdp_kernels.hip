// Partial dependence on device (gfx950): score every row of X through the forest once per GRID TUPLE, where a
// tuple g replaces the row's values of a feature set S by V[s][g]. out[G][N][K] (fp32): cell (g, i, c) is the sum,
// over the trees of class c in forest order, of the leaf that row i reaches under tuple g: bit for bit what
// k_predict (predict_kernels.hip) gives on a copy of X whose S rows were overwritten with tuple g: both walks decide
// every split with forest_go_left (forest_view.h) and add the leaves in the same order.
//
// Down one row's path only the splits on a feature of S depend on the tuple, so most tuples share their leaf. The
// walk forks on the tuples instead of repeating itself per tuple:
//
// k_pd_node_masks: one thread per (node, chunk of at most 64 tuples). For a split on a feature of S it writes a
//   64-bit mask, bit g = "tuple g of the chunk goes left", from forest_go_left (NaN and categorical codes
//   outside [0, cat_nbits) take na_left, else the bitset bit; numeric x < thr in fp32). Chunk 0 also writes
//   featx[node]: the node's feature with PD_SEL set when it is in S (-1 for a leaf), which is what the walk reads
//   instead of feat.
// k_predict_grid: one lane owns one row, a block is ONE wave (64 rows) and one chunk of tuples and one class
//   (grid = row tiles x chunks x K: one pass per class over that class's trees, the others are skipped). Per tree
//   the lane's remaining tuples start as the chunk's full mask; it takes the lowest remaining tuple, walks from
//   the root following that tuple's bit at the splits on S (ANDing the running mask with the node mask or its
//   complement) and its own X[feat * N + row] elsewhere (adjacent lanes, adjacent rows: coalesced as in
//   k_predict), adds the leaf to the accumulator of every tuple left in the running mask, clears them from the
//   remaining set and repeats until it is empty: stackless, one root-to-leaf walk per distinct leaf.
//
// Accumulators: fp32 in LDS, acc[g][lane] (lane-contiguous: bank = lane mod 32, conflict free; only the owning
// lane touches its column, so plain read-modify-write, no atomics, no barrier). They start at 0.0f and take the
// trees in forest order per cell. LDS per block (dynamic): 256 bytes per tuple of the launch's largest chunk, so
// 16,384 bytes (10 waves per CU) for 64 tuples and 5,120 bytes (the full 32 waves per CU) for a 20-value grid.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_pd_node_masks: 20 VGPR, 33 SGPR, 0 bytes of scratch, 0 spills, no LDS, occupancy 8 waves per SIMD
//   k_predict_grid:  22 VGPR, 82 SGPR, 0 bytes of scratch, 0 spills, occupancy by registers 8 waves per SIMD
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "forest_view.h"

namespace {

constexpr int PD_CHUNK = 64;            // tuples per chunk: one bit each of a node mask (PD_CHUNK in ops/forest.py)
constexpr int PD_ROWS = 64;             // rows per block: one wave
constexpr int PD_SEL = 1 << 30;         // featx bit: the split's feature is in S

__global__ __launch_bounds__(256) void k_pd_node_masks(
    ForestView fv, const int* __restrict__ sel, const float* __restrict__ V, long long G, long long g_begin,
    unsigned long long* __restrict__ masks /*[chunks of this launch][n_nodes]*/, int* __restrict__ featx) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= fv.n_nodes) return;
  const int f = fv.feat[n];
  const int s = f >= 0 ? sel[f] : -1;
  if (blockIdx.y == 0) featx[n] = f < 0 ? -1 : (s >= 0 ? (f | PD_SEL) : f);
  unsigned long long m = 0ull;
  if (s >= 0) {
    const long long g0 = g_begin + (long long)blockIdx.y * PD_CHUNK;
    const int gc = (int)((G - g0) < (long long)PD_CHUNK ? (G - g0) : (long long)PD_CHUNK);
    const float* v = V + (long long)s * G + g0;
    for (int g = 0; g < gc; ++g) {
      if (forest_go_left(fv, n, v[g])) m |= 1ull << g;
    }
  }
  masks[(long long)blockIdx.y * fv.n_nodes + n] = m;
}

__global__ __launch_bounds__(PD_ROWS) void k_predict_grid(
    const float* __restrict__ X, long long N, int K, long long G, long long g_begin, ForestView fv,
    const int* __restrict__ featx, const unsigned long long* __restrict__ masks,
    float* __restrict__ out /*[G][N][K]*/) {
  extern __shared__ float acc[];          // [tuples of the launch's largest chunk][PD_ROWS]
  const int lane = threadIdx.x;
  const long long row = (long long)blockIdx.x * PD_ROWS + lane;
  const long long g0 = g_begin + (long long)blockIdx.y * PD_CHUNK;
  const int gc = (int)((G - g0) < (long long)PD_CHUNK ? (G - g0) : (long long)PD_CHUNK);
  const int cls = blockIdx.z;
  if (row >= N || gc <= 0) return;       // no barrier in this kernel: a lane may leave
  const unsigned long long full = gc >= 64 ? ~0ull : ((1ull << gc) - 1ull);
  const unsigned long long* nm = masks + (long long)blockIdx.y * fv.n_nodes;
  float* a = acc + lane;
  for (int g = 0; g < gc; ++g) a[g * PD_ROWS] = 0.0f;

  for (int t = 0; t < fv.n_trees; ++t) {
    if (fv.cls[t] != cls) continue;
    const int root = fv.roots[t];
    unsigned long long rem = full;
    while (rem) {
      const int first = __ffsll((unsigned long long)rem) - 1;
      unsigned long long m = rem;
      int n = root;
      int fx = featx[n];
      while (fx >= 0) {
        bool go_left;
        if (fx & PD_SEL) {
          const unsigned long long k = nm[n];
          go_left = (k >> first) & 1ull;
          m &= go_left ? k : ~k;
        } else {
          go_left = forest_go_left(fv, n, X[(long long)fx * N + row]);
        }
        n = go_left ? fv.left[n] : fv.right[n];
        fx = featx[n];
      }
      const float v = fv.value[n];
      rem &= ~m;
      while (m) {
        const int g = __ffsll((unsigned long long)m) - 1;
        a[g * PD_ROWS] += v;
        m &= m - 1ull;
      }
    }
  }
  for (int g = 0; g < gc; ++g) out[((g0 + g) * N + row) * K + cls] = a[g * PD_ROWS];
}

}  // namespace

extern "C" {

// X: float32 [F][N]; fv: the flat forest (host pointer, read here); sel: int32 [F], -1 or the position of the
// feature in S; V: float32 [|S|][G]. out: float32 [G][N][K], every cell is written. Workspace: masks uint64
// [ws_chunks][n_nodes], featx int32 [n_nodes]. Tuples go in launches of at most ws_chunks chunks of 64.
int h2o_predict_grid(const void* X, long long N, int K, const ForestView* fv, const void* sel, const void* V,
                     long long G, void* masks, void* featx, int ws_chunks, void* out, hipStream_t s) {
  if (N <= 0 || G <= 0 || fv->n_trees <= 0 || fv->n_nodes <= 0) return 0;
  const long long tiles = (N + PD_ROWS - 1) / PD_ROWS;
  if (K <= 0 || K > 65535 || ws_chunks <= 0 || tiles > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (ws_chunks > 65535) ws_chunks = 65535;      // grid y
  const long long per_launch = (long long)ws_chunks * PD_CHUNK;
  for (long long g_begin = 0; g_begin < G; g_begin += per_launch) {
    const long long left_g = G - g_begin;
    const unsigned chunks = (unsigned)(((left_g < per_launch ? left_g : per_launch) + PD_CHUNK - 1) / PD_CHUNK);
    const size_t lds = (size_t)(left_g < PD_CHUNK ? left_g : PD_CHUNK) * PD_ROWS * sizeof(float);
    hipLaunchKernelGGL(k_pd_node_masks, dim3((unsigned)((fv->n_nodes + 255) / 256), chunks), dim3(256), 0, s, *fv,
                       (const int*)sel, (const float*)V, G, g_begin, (unsigned long long*)masks, (int*)featx);
    hipLaunchKernelGGL(k_predict_grid, dim3((unsigned)tiles, chunks, (unsigned)K), dim3(PD_ROWS), lds, s,
                       (const float*)X, N, K, G, g_begin, *fv, (const int*)featx,
                       (const unsigned long long*)masks, (float*)out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
