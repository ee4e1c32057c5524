// Path-decomposed TreeSHAP on device (gfx950). Formulation: Mitchell, Frank, Holmes, "GPUTreeShap:
// massively parallel exact calculation of SHAP scores for tree ensembles" (2020); the path table is built by
// ops/shap.py (forest_paths), the recursion this replaces on device is csrc/treeshap.cpp. What this kernel shares
// with k_shap_baseline (the table's device view, element load, condition test, phi tile) is path_table.h's.
//
// k_tree_shap<G>: lanes are path elements. A path is padded to G lanes (G = 8/16/32/64, the smallest that
// holds the forest's longest path), 64/G paths share a wave, a block of 256 threads holds 256/G paths per
// "round". Grid = row tiles (x) * path chunks (y); a block walks `rounds` rounds of paths over its SHAP_R
// rows. Per (row, path) every lane evaluates its element's merged split condition (one_fraction 0 or 1),
// the group runs the EXTEND recurrence (len-1 steps, pweight[i] from lanes i and i-1), then every lane
// i >= 1 runs UNWOUND_SUM for its own element (len-1 broadcasts of pweight[j]) and adds
// sum * (one - zero) * leaf_value to phi[row][cls][feature]. The DP and every accumulation are fp64.
//
// LDS per block (at most 52,032 bytes, so two blocks fit a CU): 1/k table, the round's zero fractions (read
// by broadcast in EXTEND), the phi tile [R][K][F+1] fp64 when it fits SHAP_PHI_BYTES (else fp64 atomics go
// straight to global), the X tile [F][R+1] fp32 when it fits SHAP_X_BYTES (else elements read X[f*N + r]).
// The phi tile is flushed with fp64 atomic adds (global_atomic_add_f64, ds_add_f64 in LDS: no compare-and-swap
// loop), so results differ in the last bits from run to run. The launcher splits the rows over several
// launches of about SHAP_PAIRS (row, path) pairs each.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   G = 8: 62 VGPR    G = 16: 62 VGPR    G = 32: 60 VGPR    G = 64: 56 VGPR
//   every instantiation: 0 bytes of scratch, 0 VGPR / SGPR spills, occupancy 8 waves per SIMD
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "path_table.h"

namespace {

constexpr int SHAP_THREADS = 256;
constexpr int SHAP_R = 64;              // rows per block (ROW_TILE in ops/shap.py)
constexpr int SHAP_RS = SHAP_R + 1;     // X tile row stride: lanes read different features of one row
constexpr int SHAP_RCP = 72;            // 1/k for k = 1..65, padded
constexpr int SHAP_X_BYTES = 16384;
constexpr int SHAP_PHI_BYTES = 32768;
constexpr long long SHAP_PAIRS = 1LL << 34;  // (row, path) pairs per launch

template <int G>
__global__ __launch_bounds__(SHAP_THREADS) void k_tree_shap(
    const float* __restrict__ X, long long N, long long row_begin, long long row_end, int F, int K, PathView pv,
    int rounds, int use_x, int use_phi, double* __restrict__ out) {
  extern __shared__ double smem[];
  double* s_rcp = smem;
  double* s_zf = smem + SHAP_RCP;
  double* s_phi = s_zf + SHAP_THREADS;
  const int F1 = F + 1;
  const int phi_n = use_phi ? SHAP_R * K * F1 : 0;
  float* s_x = (float*)(s_phi + phi_n);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int e = tid & (G - 1);          // element index inside the path
  const int gb = lane & ~(G - 1);       // first lane of this path's group in the wave
  const long long row0 = row_begin + (long long)blockIdx.x * SHAP_R;
  const int nrows = (int)((row_end - row0) < (long long)SHAP_R ? (row_end - row0) : (long long)SHAP_R);

  if (tid < SHAP_RCP) s_rcp[tid] = tid ? 1.0 / (double)tid : 0.0;
  phi_tile_zero<SHAP_THREADS>(s_phi, phi_n);
  if (use_x) {
    for (int i = tid; i < F * SHAP_R; i += SHAP_THREADS) {
      const int f = i / SHAP_R, r = i - f * SHAP_R;
      s_x[f * SHAP_RS + r] = r < nrows ? X[(long long)f * N + row0 + r] : 0.0f;
    }
  }

  for (int round = 0; round < rounds; ++round) {
    const long long first = ((long long)blockIdx.y * rounds + round) * (SHAP_THREADS / G);
    if (first >= pv.P) break;
    const int p = (int)first + tid / G;
    const bool valid = p < pv.P;
    double zf = 1.0;
    const PathElem el = path_elem_load<G>(pv, p, e, &zf);
    __syncthreads();                    // the X / phi staging above, and last round's readers of s_zf
    s_zf[tid] = zf;
    __syncthreads();

    int ml = el.len;                       // longest path of this wave: the wave-uniform trip count
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) ml = max(ml, __shfl_xor(ml, o));
    ml = __builtin_amdgcn_readfirstlane(ml);

    const bool real = e >= 1 && e < el.len;
    const int fx = el.feat < 0 ? 0 : el.feat;
    const int d = el.len - 1;              // index of the path's last element
    const double c1 = (double)(d + 1);
    const double c2 = zf * s_rcp[d + 1];
    const double c3 = c1 / zf;
    const double* gzf = s_zf + (tid & ~(G - 1));
    const long long o_base = ((long long)el.cls * F1 + fx);

    for (int r = 0; r < nrows; ++r) {
      const float v = use_x ? s_x[fx * SHAP_RS + r] : X[(long long)fx * N + row0 + r];
      const bool hot = path_elem_ok(el, pv.cat_bits, v) || !real;     // dummy root and padding: one_fraction 1
      const unsigned long long ofm = __ballot(hot) >> gb;

      // EXTEND: pweight of the path built from elements 0..dd
      double pw = e == 0 ? 1.0 : 0.0;
      for (int dd = 1; dd < ml; ++dd) {
        double left = __shfl_up(pw, 1, G);
        if (e == 0) left = 0.0;
        const double rd = s_rcp[dd + 1];
        const double a = gzf[dd] * ((double)(dd - e) * rd);
        const double b = ((ofm >> dd) & 1ull) ? (double)e * rd : 0.0;
        const double nw = pw * a + left * b;
        pw = dd < el.len ? nw : pw;
      }

      // UNWOUND_SUM for this lane's element
      double next = __shfl(pw, d, G);
      double total = 0.0;
      for (int i = ml - 2; i >= 0; --i) {
        const double pi = __shfl(pw, i, G);
        if (i < d) {
          if (hot) {
            const double tmp = next * c1 * s_rcp[i + 1];
            total += tmp;
            next = pi - tmp * c2 * (double)(d - i);
          } else {
            total += pi * c3 * s_rcp[d - i];
          }
        }
      }
      if (real && valid) {
        const double c = total * ((hot ? 1.0 : 0.0) - zf) * el.val;
        if (use_phi) atomicAdd(&s_phi[(long long)r * K * F1 + o_base], c);
        else unsafeAtomicAdd(&out[(row0 + r) * K * F1 + o_base], c);
      }
    }
  }

  if (use_phi) phi_tile_flush<SHAP_THREADS>(s_phi, out + row0 * K * F1, nrows * K * F1);
}

}  // namespace

extern "C" {

// the compiled tile constants: the tests size their cases from the mirrors in ops/shap.py
int h2o_shap_tiles(int* out) {
  out[0] = SHAP_R; out[1] = SHAP_X_BYTES; out[2] = SHAP_PHI_BYTES;
  return 0;
}

// X: float32 [F][N]; pv: the path table (host pointer, read here); out: float64 [N][K][F+1], accumulated into (the
// caller zeroes it; the bias column is the caller's). rounds: groups of 256/G paths per block, 0 = pick from the
// grid size.
int h2o_tree_shap(const void* X, long long N, int F, int K, const PathView* pv, int rounds, void* out,
                  hipStream_t s) {
  if (N <= 0 || pv->P <= 0) return 0;
  if (F <= 0 || K <= 0 || !path_G_ok(pv->G)) return (int)hipErrorInvalidValue;
  // rows of one launch: whole tiles, about SHAP_PAIRS (row, path) pairs, so no launch runs for long
  long long rows_per_launch = (SHAP_PAIRS / pv->P) / SHAP_R * SHAP_R;
  if (rows_per_launch < SHAP_R) rows_per_launch = SHAP_R;
  if (rows_per_launch > N) rows_per_launch = N;
  const unsigned chunks = path_plan_rounds(*pv, SHAP_THREADS, (rows_per_launch + SHAP_R - 1) / SHAP_R, &rounds);
  const int use_x = (long long)F * SHAP_R * 4 <= SHAP_X_BYTES;
  const int use_phi = (long long)SHAP_R * K * (F + 1) * 8 <= SHAP_PHI_BYTES;
  size_t lds = (size_t)(SHAP_RCP + SHAP_THREADS) * 8;
  if (use_phi) lds += (size_t)SHAP_R * K * (F + 1) * 8;
  if (use_x) lds += (size_t)F * SHAP_RS * 4;
  for (long long r0 = 0; r0 < N; r0 += rows_per_launch) {
    const long long r1 = r0 + rows_per_launch < N ? r0 + rows_per_launch : N;
    const dim3 grid((unsigned)((r1 - r0 + SHAP_R - 1) / SHAP_R), chunks);
    path_dispatch(pv->G, false, [&](auto g, auto) {
      hipLaunchKernelGGL((k_tree_shap<decltype(g)::value>), grid, dim3(SHAP_THREADS), lds, s, (const float*)X, N, r0,
                         r1, F, K, *pv, rounds, use_x, use_phi, (double*)out);
    });
  }
  return (int)hipGetLastError();
}

}  // extern "C"
