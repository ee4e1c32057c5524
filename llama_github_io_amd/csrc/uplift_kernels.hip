// Uplift DRF level kernels (gfx950): the per-level histogram of the four integer statistics, the node totals of the
// last level and the one-pass row routing. Everything here is integer: sums do not depend on the order of the
// atomics, so the histogram is exact and the forest grown from it equals the PyTorch reference's bit for bit.
//
// Inputs shared by the kernels: bins uint8 [N][stride] (row-major, the first F columns are features; bin 255 = NA),
//   node int32 [N] (slot of the row's node in the level, -1 = not in the level), treat / y uint8 [N] in {0, 1}.
//
// Packed cell: a row touches exactly one arm (treated / control) per feature, so one atomic of `count | y` per row
//   and feature is enough. Global cells are uint64 `count << 32 | ysum` (a launch rejects N >= 2^31, so neither half
//   can carry): P[W][F][256][2], arm 0 = treated, arm 1 = control; ops/uplift.py unpacks them to (n_t, y_t, n_c, y_c).
//
// k_uplift_hist_lds (narrow windows): a block owns UP_TILE rows and a group of FG features and keeps the group's
//   cells in LDS as uint32 `count << 16 | ysum`: UP_TILE = 4096 <= 65535, so neither 16-bit half can carry even when
//   every row of the tile lands in one cell with y = 1. One lane per row: node, treat and y are read once, then one
//   byte and one ds_add_u32 per feature. The flush adds every non-zero cell to P with one 64-bit atomic.
//   Dynamic LDS: W * FG * 2 KiB per block, at most UP_LDS_CELLS * 4 = 64 KiB (W * FG <= 32: two blocks per CU;
//   the caller picks FG, so a smaller group buys more resident blocks).
// k_uplift_hist_direct (wide levels): one lane per (row, feature), one 64-bit global atomic each; rows per node are
//   few, so are the collisions.
// k_uplift_totals: T[A][2] packed like P, one 64-bit atomic per row of the level.
// k_uplift_route: out[r] = child[n] + (bins[r][feat[n]] < bin[n] ? 0 : 1) for n = node[r]; -1 when the row is not
//   in the level, the node became a leaf (child < 0) or the table is out of range. NA (255) goes right.
//
// Bounds: a bin is a byte, so < 256; a node slot is used only after 0 <= n - n0 < W (0 <= n < A in the route and
//   the totals); features are < F <= stride; rows < N; row * stride in 64 bits.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch, no spills:
//   k_uplift_hist_lds 17 VGPR / 50 SGPR, dynamic LDS only; k_uplift_hist_direct 19 / 48; k_uplift_totals 11 / 26;
//   k_uplift_route 14 / 35; occupancy by registers 8 waves per SIMD each. Measured crossover: profiles/uplift_gpu.md.
#include <hip/hip_runtime.h>

namespace {

constexpr int UP_BLOCK = 256;
constexpr int UP_TILE = 4096;             // rows per block of the LDS variant (16-bit halves: must stay <= 65535)
constexpr int UP_LDS_CELLS = 16384;       // uint32 cells per block = 64 KiB
constexpr int UP_CELLS_NF = 512;          // cells per (node, feature): 256 bins x 2 arms

static_assert(UP_TILE <= 65535, "a packed LDS cell holds a 16-bit count and a 16-bit sum");

typedef unsigned long long u64;

__global__ __launch_bounds__(UP_BLOCK) void k_uplift_hist_lds(const unsigned char* __restrict__ bins, long long N,
                                                              int stride, int F, int FG,
                                                              const int* __restrict__ node,
                                                              const unsigned char* __restrict__ treat,
                                                              const unsigned char* __restrict__ y, int n0, int W,
                                                              u64* __restrict__ P /*[W][F][256][2]*/) {
  extern __shared__ unsigned cells[];                 // [W][nf][256][2], W * FG * 2 KiB of dynamic LDS
  const int f0 = blockIdx.y * FG;
  const int nf = min(FG, F - f0);
  const int used = W * nf * UP_CELLS_NF;              // <= UP_LDS_CELLS (the launcher checks W * FG)
  for (int i = threadIdx.x; i < used; i += UP_BLOCK) cells[i] = 0u;
  __syncthreads();

  const long long r0 = (long long)blockIdx.x * UP_TILE;
  const long long r1 = min(r0 + UP_TILE, N);
  for (long long r = r0 + threadIdx.x; r < r1; r += UP_BLOCK) {
    const int n = node[r] - n0;
    if (n < 0 || n >= W) continue;
    const unsigned arm = treat[r] ? 0u : 1u;
    const unsigned add = (1u << 16) | (y[r] ? 1u : 0u);
    const unsigned char* b = bins + r * stride + f0;
    unsigned* c = cells + (size_t)n * nf * UP_CELLS_NF + arm;
    for (int f = 0; f < nf; ++f) atomicAdd(c + f * UP_CELLS_NF + 2 * (unsigned)b[f], add);
  }
  __syncthreads();

  for (int i = threadIdx.x; i < used; i += UP_BLOCK) {
    const unsigned v = cells[i];
    if (v == 0u) continue;
    const int w = i / (nf * UP_CELLS_NF);
    const int rem = i - w * (nf * UP_CELLS_NF);       // f_local * 512 + bin * 2 + arm
    const size_t g = ((size_t)w * F + f0) * UP_CELLS_NF + rem;
    atomicAdd(P + g, ((u64)(v >> 16) << 32) | (u64)(v & 0xffffu));
  }
}

__global__ __launch_bounds__(UP_BLOCK) void k_uplift_hist_direct(const unsigned char* __restrict__ bins, long long N,
                                                                 int stride, int F, const int* __restrict__ node,
                                                                 const unsigned char* __restrict__ treat,
                                                                 const unsigned char* __restrict__ y, int n0, int W,
                                                                 u64* __restrict__ P /*[W][F][256][2]*/) {
  const long long total = N * F;
  const long long step = (long long)gridDim.x * UP_BLOCK;
  for (long long i = (long long)blockIdx.x * UP_BLOCK + threadIdx.x; i < total; i += step) {
    const long long r = i / F;
    const int f = (int)(i - r * F);
    const int n = node[r] - n0;
    if (n < 0 || n >= W) continue;
    const unsigned arm = treat[r] ? 0u : 1u;
    const unsigned bin = bins[r * stride + f];
    atomicAdd(P + ((size_t)n * F + f) * UP_CELLS_NF + 2 * bin + arm, (1ull << 32) | (u64)(y[r] ? 1 : 0));
  }
}

__global__ __launch_bounds__(UP_BLOCK) void k_uplift_totals(long long N, const int* __restrict__ node,
                                                            const unsigned char* __restrict__ treat,
                                                            const unsigned char* __restrict__ y, int A,
                                                            u64* __restrict__ T /*[A][2]*/) {
  const long long step = (long long)gridDim.x * UP_BLOCK;
  for (long long r = (long long)blockIdx.x * UP_BLOCK + threadIdx.x; r < N; r += step) {
    const int n = node[r];
    if (n < 0 || n >= A) continue;
    atomicAdd(T + (size_t)n * 2 + (treat[r] ? 0 : 1), (1ull << 32) | (u64)(y[r] ? 1 : 0));
  }
}

__global__ __launch_bounds__(UP_BLOCK) void k_uplift_route(const unsigned char* __restrict__ bins, long long N,
                                                           int stride, int F, const int* __restrict__ node, int A,
                                                           const int* __restrict__ split_feat,
                                                           const int* __restrict__ split_bin,
                                                           const int* __restrict__ child, int* __restrict__ out) {
  const long long step = (long long)gridDim.x * UP_BLOCK;
  for (long long r = (long long)blockIdx.x * UP_BLOCK + threadIdx.x; r < N; r += step) {
    const int n = node[r];
    int o = -1;
    if (n >= 0 && n < A) {
      const int c = child[n];
      const int f = split_feat[n];
      if (c >= 0 && f >= 0 && f < F) o = c + ((int)bins[r * stride + f] < split_bin[n] ? 0 : 1);
    }
    out[r] = o;
  }
}

unsigned up_grid(long long work) {        // memory-bound passes: at most 2048 blocks, grid-stride the rest
  const long long b = (work + UP_BLOCK - 1) / UP_BLOCK;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

}  // namespace

extern "C" {

// P: uint64 [W][F][256][2], zeroed by the caller, added to here. variant 0 = LDS-privatised (W * fgroup <= 32 =
// UP_LDS_CELLS / UP_CELLS_NF, 1 <= fgroup <= F), 1 = direct global atomics (fgroup ignored).
int h2o_uplift_hist(const void* bins, long long N, int stride, int F, const void* node, const void* treat,
                    const void* y, int n0, int W, int variant, int fgroup, void* P, hipStream_t s) {
  if (N <= 0 || W <= 0) return 0;
  if (F <= 0 || stride < F || n0 < 0 || N >= (1LL << 31)) return (int)hipErrorInvalidValue;
  if (variant == 0) {
    if (fgroup < 1 || fgroup > F || (long long)W * fgroup * UP_CELLS_NF > UP_LDS_CELLS)
      return (int)hipErrorInvalidValue;
    const long long tiles = (N + UP_TILE - 1) / UP_TILE;
    const dim3 grid((unsigned)tiles, (unsigned)((F + fgroup - 1) / fgroup));
    const size_t lds = (size_t)W * fgroup * UP_CELLS_NF * sizeof(unsigned);
    hipLaunchKernelGGL(k_uplift_hist_lds, grid, dim3(UP_BLOCK), lds, s, (const unsigned char*)bins, N, stride, F,
                       fgroup, (const int*)node, (const unsigned char*)treat, (const unsigned char*)y, n0, W,
                       (u64*)P);
  } else if (variant == 1) {
    hipLaunchKernelGGL(k_uplift_hist_direct, dim3(up_grid(N * F)), dim3(UP_BLOCK), 0, s,
                       (const unsigned char*)bins, N, stride, F, (const int*)node, (const unsigned char*)treat,
                       (const unsigned char*)y, n0, W, (u64*)P);
  } else {
    return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

// T: uint64 [A][2], zeroed by the caller.
int h2o_uplift_totals(long long N, const void* node, const void* treat, const void* y, int A, void* T,
                      hipStream_t s) {
  if (N <= 0 || A <= 0) return 0;
  if (N >= (1LL << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_uplift_totals, dim3(up_grid(N)), dim3(UP_BLOCK), 0, s, N, (const int*)node,
                     (const unsigned char*)treat, (const unsigned char*)y, A, (u64*)T);
  return (int)hipGetLastError();
}

// split_feat / split_bin / child: int32 [A]; out: int32 [N], every cell written; out and node are different buffers.
int h2o_uplift_route(const void* bins, long long N, int stride, int F, const void* node, int A,
                     const void* split_feat, const void* split_bin, const void* child, void* out, hipStream_t s) {
  if (N <= 0) return 0;
  if (F <= 0 || stride < F || A < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_uplift_route, dim3(up_grid(N)), dim3(UP_BLOCK), 0, s, (const unsigned char*)bins, N, stride,
                     F, (const int*)node, A, (const int*)split_feat, (const int*)split_bin, (const int*)child,
                     (int*)out);
  return (int)hipGetLastError();
}

}  // extern "C"
