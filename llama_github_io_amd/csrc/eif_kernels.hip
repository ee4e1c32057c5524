// Extended Isolation Forest scoring (gfx950): for every row of X, walk every tree of the packed forest (eif_view.h)
// in forest order and store the fp64 sum of the leaf values it reaches: out[i] = sum_t value[leaf_t(i)].
//
// k_eif_path: one lane owns one row; a block is 256 rows (4 waves). At a split the lane computes
//     s = 0.0;  for k in [nz_begin[n], nz_begin[n + 1]):  s = s + (double)x[nz_feat[k]] * nz_val[k]
//   with every product and every sum rounded on its own, and goes left iff (s - off[n]) <= 0.0, so a NaN projection
//   goes right. No FMA: `#pragma clang fp contract(off)` covers this file and the walk uses the plain operators under
//   it (the HIP header's __dmul_rn / __dadd_rn are compiled contractible and DO fuse into v_fmac_f64 once inlined;
//   the ISA of this file holds v_mul_f64 + v_add_f64 and no fp64 FMA). A sequential fp64 loop on the host therefore
//   reproduces the walk bit for bit. The leaf values are added to an fp64 register, one add per tree in forest
//   order, from 0.0.
//   nan_to_zero: the native model's mapping of non-finite inputs, NaN -> 0 and +-inf -> +-DBL_MAX (what
//   torch.nan_to_num(x.double(), nan=0.0) gives); without it the values pass through (MOJO semantics: a NaN or an
//   infinity in a listed feature poisons the projection, which is why imported forests list every feature).
//
// Rows (template parameter STAGED): true = the block copies its rows into dynamic LDS once, xs[f][lane]
//   (lane-contiguous: bank = lane mod 32 whatever feature a lane reads, so lanes at different nodes never conflict),
//   NaN -> 0 applied on the way in (an infinity has no float image of DBL_MAX and is clamped when widened); a lane
//   reads only its own column, so there is NO barrier and a lane with row >= N leaves at once. false = the lane reads
//   X[f * N + row] (coalesced across the wave for a given f, served by L1/L2 on the re-reads). The launcher stages
//   while F * 256 * 4 bytes fit under the byte cap it is given (ops/eif.py: EIF_ROW_LDS_BYTES), never above 64 KiB.
// Node records and component lists are read from global memory: the packed forest is a few MB and stays in L2.
//
// LDS budget when staged: F * 1 KiB per block (F = 28: 28 KiB = 5 blocks = 20 waves per CU of 160 KiB; F = 64:
// 64 KiB = 2 blocks = 8 waves). Indexing: f * N + row in 64 bits.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_eif_path<true>:  28 VGPR, 54 SGPR, 0 bytes of scratch, 0 spills, dynamic LDS only, occupancy by registers 8
//   k_eif_path<false>: 26 VGPR, 46 SGPR, 0 bytes of scratch, 0 spills, no LDS, occupancy 8 waves per SIMD
#include <hip/hip_runtime.h>

#include <cfloat>

#include "eif_view.h"

#pragma clang fp contract(off)

namespace {

constexpr int EIF_ROWS = 256;             // rows per block
constexpr int EIF_MAX_LDS = 64 << 10;     // dynamic LDS per block at most

template <bool STAGED>
__device__ __forceinline__ double eif_widen(float x, int nan_to_zero) {
  double d = (double)x;
  if (nan_to_zero) {
    if (!STAGED && x != x) d = 0.0;       // staged rows lost their NaNs on the way into LDS
    d = d > DBL_MAX ? DBL_MAX : (d < -DBL_MAX ? -DBL_MAX : d);
  }
  return d;
}

template <bool STAGED>
__global__ __launch_bounds__(EIF_ROWS) void k_eif_path(const float* __restrict__ X, long long N, int F, EifView ev,
                                                       int nan_to_zero, double* __restrict__ out /*[N]*/) {
  extern __shared__ float xs_lds[];       // STAGED: xs [F][EIF_ROWS]
  const int lane = threadIdx.x;
  const long long row = (long long)blockIdx.x * EIF_ROWS + lane;
  if (row >= N) return;                   // no barrier in this kernel: a lane may leave
  const float* xg = X + row;              // xg[f * N]
  const float* xs = xs_lds + lane;        // xs[f * EIF_ROWS]
  if (STAGED)
    for (int f = 0; f < F; ++f) {
      const float x = xg[(long long)f * N];
      xs_lds[f * EIF_ROWS + lane] = (nan_to_zero && x != x) ? 0.0f : x;
    }

  double acc = 0.0;
  for (int t = 0; t < ev.n_trees; ++t) {
    int n = ev.roots[t];
    int l = ev.left[n];
    while (l >= 0) {
      double s = 0.0;
      const int k1 = ev.nz_begin[n + 1];
      for (int k = ev.nz_begin[n]; k < k1; ++k) {
        const int f = ev.nz_feat[k];
        const float x = STAGED ? xs[f * EIF_ROWS] : xg[(long long)f * N];
        s = s + eif_widen<STAGED>(x, nan_to_zero) * ev.nz_val[k];     // two roundings: contraction is off
      }
      n = (s - ev.off[n] <= 0.0) ? l : ev.right[n];
      l = ev.left[n];
    }
    acc = acc + ev.value[n];
  }
  out[row] = acc;
}

}  // namespace

extern "C" {

// X: float32 [F][N]; ev: the packed forest (host pointer, read here), every nz_feat < F (the caller checks).
// out: float64 [N], every cell written. row_lds_bytes: the rows are staged in LDS while F * 1024 bytes fit under it
// (and under 64 KiB), read from X itself past it.
int h2o_eif_path(const void* X, long long N, int F, const EifView* ev, int nan_to_zero, int row_lds_bytes, void* out,
                 hipStream_t s) {
  if (N <= 0) return 0;
  const long long tiles = (N + EIF_ROWS - 1) / EIF_ROWS;
  if (F <= 0 || ev->n_trees <= 0 || ev->n_nodes <= 0 || tiles > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const long long row_bytes = (long long)F * EIF_ROWS * (long long)sizeof(float);
  const dim3 grid((unsigned)tiles), blk(EIF_ROWS);
  if (row_bytes <= row_lds_bytes && row_bytes <= EIF_MAX_LDS)
    hipLaunchKernelGGL(k_eif_path<true>, grid, blk, (size_t)row_bytes, s, (const float*)X, N, F, *ev, nan_to_zero,
                       (double*)out);
  else
    hipLaunchKernelGGL(k_eif_path<false>, grid, blk, 0, s, (const float*)X, N, F, *ev, nan_to_zero, (double*)out);
  return (int)hipGetLastError();
}

}  // extern "C"
