// Baseline (interventional) SHAP on device (gfx950): Shapley values of the game v(S) = f(x_S, b_~S) for a row x
// against a background row b, over the path table of ops/shap.py (forest_paths). Closed form per (x, b, path):
// every real element's merged condition is evaluated on x and on b; if some element accepts neither row the path
// contributes nothing; otherwise with A = elements accepting x only (a of them) and C = elements accepting b only
// (c of them), a feature of A gets +val * T[a][c], a feature of C gets -val * T[c][a], and the bias cell gets val
// when a = 0 (b reaches the leaf). T[p][q] = (p-1)! q! / (p+q)! comes from the host (exact rationals rounded to
// fp64, [G][G]). What this kernel shares with k_tree_shap (the table's device view, element load, condition test,
// phi tile) is path_table.h's.
//
// k_shap_baseline<G, PER_REF>: lanes are path elements, a path is padded to G lanes (G = 8/16/32/64), 64/G paths share a
// wave, a block of 256 threads holds 256/G paths per "round". Grid = row tiles (x) * path chunks (y) * background
// tiles (z); a block owns SB_R rows x SB_BT background rows and walks `rounds` rounds of paths. Per round every
// lane evaluates its element's condition on the SB_R rows and the SB_BT background rows and the wave ballots each
// result into LDS (one 64-bit word per wave and row: the G-bit masks of its 64/G paths). The pair loop is mask
// arithmetic: xo = mx & ~mb, bo = mb & ~mx, dead = ~(mx | mb), two popcounts and one T lookup per lane. There is
// no EXTEND / UNWOUND recurrence.
//
// Two output modes. Summed over the background, out[N][K][F+1]: a lane sums its weights over the background tile
// in a register, adds the sum times the leaf value to the block's phi tile [SB_R][K][F+1] in LDS when that fits
// SB_PHI_BYTES (else straight to global), and the tile is flushed once per block. Per reference,
// out[N*B][K][F+1] with pair index i*B + j: every nonzero weight is one global add. All adds are native fp64
// atomics (global_atomic_add_f64, ds_add_f64: no compare-and-swap loop), so results differ in the last bits from
// run to run. The caller zeroes out. The launcher splits rows and background rows over several launches of about
// SB_TRIPLES (row, background row, path) triples each.
//
// LDS per block (at most 63,680 bytes): T [G][G] fp64, the round's ballots [4 waves][SB_R + SB_BT] 64-bit, the phi
// tile when used, the X / background tile [F][SB_R + SB_BT + 1] fp32 when F * (SB_R + SB_BT) * 4 fits SB_X_BYTES
// (else elements read X[f*N + r] and Bg[f*B + j]).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   summed:        G = 8: 30 VGPR    G = 16: 30 VGPR    G = 32: 32 VGPR    G = 64: 39 VGPR
//   per reference: G = 8: 30 VGPR    G = 16: 30 VGPR    G = 32: 32 VGPR    G = 64: 37 VGPR
//   every instantiation: 0 bytes of scratch, 0 VGPR / SGPR spills, occupancy 8 waves per SIMD
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "path_table.h"

namespace {

constexpr int SB_THREADS = 256;
constexpr int SB_R = 32;                // rows per block (BASELINE_ROW_TILE in ops/shap.py)
constexpr int SB_BT = 32;               // background rows per block (BG_TILE)
constexpr int SB_M = SB_R + SB_BT;      // ballots per wave and round
constexpr int SB_XS = SB_M + 1;         // X tile stride: lanes read different features of one row
constexpr int SB_X_BYTES = 12288;
constexpr int SB_PHI_BYTES = 16384;
constexpr long long SB_TRIPLES = 1LL << 36;  // (row, background row, path) triples per launch

template <int G> struct sb_mask { typedef uint32_t type; };
template <> struct sb_mask<64> { typedef uint64_t type; };

__device__ __forceinline__ int sb_popc(uint32_t m) { return __popc(m); }
__device__ __forceinline__ int sb_popc(uint64_t m) { return __popcll(m); }

template <int G, bool PER_REF>
__global__ __launch_bounds__(SB_THREADS) void k_shap_baseline(
    const float* __restrict__ X, long long N, long long row_begin, long long row_end,
    const float* __restrict__ Bg, long long B, long long bg_begin, long long bg_end, int F, int K, int P,
    const int* __restrict__ e_feat, const float* __restrict__ e_lo, const float* __restrict__ e_hi,
    const int* __restrict__ e_flags, const int* __restrict__ e_coff, const int* __restrict__ e_cnb,
    const uint32_t* __restrict__ cat_bits, const int* __restrict__ p_len, const double* __restrict__ p_val,
    const int* __restrict__ p_cls, const double* __restrict__ T, int rounds, int use_x, int use_phi, double* __restrict__ out) {
  typedef typename sb_mask<G>::type M;
  // the table's arrays arrive as separate arguments (no zf): with the PathView as one by-value argument this kernel
  // measured 2.5-4 % slower on an MI355X (profiles/forest_view_ab.md), k_tree_shap did not
  const PathView pv{e_feat, nullptr, e_lo, e_hi, e_flags, e_coff, e_cnb, cat_bits, p_len, p_val, p_cls, P, G};
  extern __shared__ double smem[];
  double* s_T = smem;
  unsigned long long* s_m = (unsigned long long*)(s_T + G * G);
  double* s_phi = (double*)(s_m + (SB_THREADS / 64) * SB_M);
  const int F1 = F + 1;
  const int phi_n = use_phi ? SB_R * K * F1 : 0;
  float* s_x = (float*)(s_phi + phi_n);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int e = tid & (G - 1);          // element index inside the path
  const int gb = lane & ~(G - 1);       // first lane of this path's group in the wave
  const long long row0 = row_begin + (long long)blockIdx.x * SB_R;
  const long long b0 = bg_begin + (long long)blockIdx.z * SB_BT;
  const int nrows = (int)((row_end - row0) < (long long)SB_R ? (row_end - row0) : (long long)SB_R);
  const int nb = (int)((bg_end - b0) < (long long)SB_BT ? (bg_end - b0) : (long long)SB_BT);
  unsigned long long* wm = s_m + (tid >> 6) * SB_M;

  for (int i = tid; i < G * G; i += SB_THREADS) s_T[i] = T[i];
  phi_tile_zero<SB_THREADS>(s_phi, phi_n);
  if (use_x) {
    for (int i = tid; i < F * SB_M; i += SB_THREADS) {
      const int f = i / SB_M, r = i - f * SB_M;
      float v = 0.0f;
      if (r < SB_R) {
        if (r < nrows) v = X[(long long)f * N + row0 + r];
      } else if (r - SB_R < nb) {
        v = Bg[(long long)f * B + b0 + (r - SB_R)];
      }
      s_x[f * SB_XS + r] = v;
    }
  }

  for (int round = 0; round < rounds; ++round) {
    const long long first = ((long long)blockIdx.y * rounds + round) * (SB_THREADS / G);
    if (first >= pv.P) break;
    const int p = (int)first + tid / G;
    const bool valid = p < pv.P;
    const PathElem el = path_elem_load<G>(pv, p, e);
    const int fe = el.feat < 0 ? 0 : el.feat;
    __syncthreads();                    // the staging above, and last round's readers of the ballots

    for (int i = 0; i < nrows + nb; ++i) {
      const int idx = i < nrows ? i : SB_R + (i - nrows);
      float v;
      if (use_x) v = s_x[fe * SB_XS + idx];
      else v = i < nrows ? X[(long long)fe * N + row0 + i] : Bg[(long long)fe * B + b0 + (i - nrows)];
      const unsigned long long m = __ballot(path_elem_ok(el, pv.cat_bits, v));
      if (lane == 0) wm[idx] = m;
    }
    __syncthreads();

    // elements 1 .. len-1 are real; the dummy root (bit 0) and the padding are in neither set
    const M realm = (M)((el.len >= 64 ? ~0ull : ((1ull << el.len) - 1ull)) & ~1ull);
    const M ebit = (M)((M)1 << e);
    const long long o_cell = (long long)el.cls * F1 + (e == 0 ? F : fe);
    const double e0 = e == 0 ? 1.0 : 0.0;   // lane 0 carries the bias cell

    for (int r = 0; r < nrows; ++r) {
      const M mx = (M)(wm[r] >> gb);
      double acc = 0.0;
      for (int j = 0; j < nb; ++j) {
        const M mb = (M)(wm[SB_R + j] >> gb);
        const M xo = mx & ~mb & realm, bo = mb & ~mx & realm;
        const bool dead = (~(mx | mb) & realm) != 0;
        const int a = sb_popc(xo), c = sb_popc(bo);
        const bool in_x = (xo & ebit) != 0, in_b = (bo & ebit) != 0;
        const double t = s_T[in_x ? a * G + c : c * G + a];
        double w = a == 0 ? e0 : 0.0;
        w = in_b ? -t : w;
        w = in_x ? t : w;
        w = dead ? 0.0 : w;
        if (PER_REF) {
          if (w != 0.0 && valid)
            unsafeAtomicAdd(&out[((row0 + r) * B + (b0 + j)) * K * F1 + o_cell], w * el.val);
        } else {
          acc += w;
        }
      }
      if (!PER_REF && acc != 0.0 && valid) {
        if (use_phi) atomicAdd(&s_phi[(long long)r * K * F1 + o_cell], acc * el.val);
        else unsafeAtomicAdd(&out[(row0 + r) * K * F1 + o_cell], acc * el.val);
      }
    }
  }

  if (use_phi) phi_tile_flush<SB_THREADS>(s_phi, out + row0 * K * F1, nrows * K * F1);
}

}  // namespace

extern "C" {

// the compiled tile constants: the tests size their cases from the mirrors in ops/shap.py
int h2o_shap_baseline_tiles(int* out) {
  out[0] = SB_R; out[1] = SB_BT; out[2] = SB_X_BYTES; out[3] = SB_PHI_BYTES;
  return 0;
}

// X: float32 [F][N], Bg: float32 [F][B]; pv: the path table (host pointer, read here; zf is not used); T: float64
// [G][G], T[p][q] = (p-1)! q! / (p+q)!, row 0 unused. out: float64, accumulated into (the caller zeroes it):
// [N][K][F+1] summed over the background rows, or with per_ref [N*B][K][F+1] (pair i*B + j). The bias cell of a
// pair is the raw margin of its background row. rounds: groups of 256/G paths per block, 0 = pick from the grid size.
int h2o_tree_shap_baseline(const void* X, long long N, const void* Bg, long long B, int F, int K, const PathView* pv,
                           const void* T, int rounds, int per_ref, void* out, hipStream_t s) {
  if (N <= 0 || B <= 0 || pv->P <= 0) return 0;
  if (F <= 0 || K <= 0 || !path_G_ok(pv->G)) return (int)hipErrorInvalidValue;
  const int P = pv->P, G = pv->G;
  // one launch: whole tiles, about SB_TRIPLES triples, so no launch runs for long. The background is cut first
  // (at most 65535 tiles: grid z), then the rows.
  long long bg_per_launch = (SB_TRIPLES / P / SB_R) / SB_BT * SB_BT;
  if (bg_per_launch < SB_BT) bg_per_launch = SB_BT;
  if (bg_per_launch > 65535LL * SB_BT) bg_per_launch = 65535LL * SB_BT;
  if (bg_per_launch > B) bg_per_launch = B;
  long long rows_per_launch = (SB_TRIPLES / P / bg_per_launch) / SB_R * SB_R;
  if (rows_per_launch < SB_R) rows_per_launch = SB_R;
  if (rows_per_launch > (1LL << 23) * SB_R) rows_per_launch = (1LL << 23) * SB_R;   // grid x * 256 threads < 2^32
  if (rows_per_launch > N) rows_per_launch = N;
  const long long tiles = ((rows_per_launch + SB_R - 1) / SB_R) * ((bg_per_launch + SB_BT - 1) / SB_BT);
  const unsigned chunks = path_plan_rounds(*pv, SB_THREADS, tiles, &rounds);
  const int use_x = (long long)F * SB_M * 4 <= SB_X_BYTES;
  const int use_phi = !per_ref && (long long)SB_R * K * (F + 1) * 8 <= SB_PHI_BYTES;
  size_t lds = (size_t)G * G * 8 + (size_t)(SB_THREADS / 64) * SB_M * 8;
  if (use_phi) lds += (size_t)SB_R * K * (F + 1) * 8;
  if (use_x) lds += (size_t)F * SB_XS * 4;
  for (long long r0 = 0; r0 < N; r0 += rows_per_launch) {
    const long long r1 = r0 + rows_per_launch < N ? r0 + rows_per_launch : N;
    for (long long c0 = 0; c0 < B; c0 += bg_per_launch) {
      const long long c1 = c0 + bg_per_launch < B ? c0 + bg_per_launch : B;
      const dim3 grid((unsigned)((r1 - r0 + SB_R - 1) / SB_R), chunks, (unsigned)((c1 - c0 + SB_BT - 1) / SB_BT));
      path_dispatch(G, per_ref != 0, [&](auto g, auto pr) {
        hipLaunchKernelGGL((k_shap_baseline<decltype(g)::value, decltype(pr)::value>), grid, dim3(SB_THREADS), lds, s,
                           (const float*)X, N, r0, r1, (const float*)Bg, B, c0, c1, F, K, P, pv->feat, pv->lo, pv->hi,
                           pv->flags, pv->cat_off, pv->cat_nbits, pv->cat_bits, pv->len, pv->value, pv->cls,
                           (const double*)T, rounds, use_x, use_phi, (double*)out);
      });
    }
  }
  return (int)hipGetLastError();
}

}  // extern "C"
