// Baseline (interventional) SHAP on device (gfx950): Shapley values of the game v(S) = f(x_S, b_~S) for a row x
// against a background row b, over the path table of ops/shap.py (forest_paths). Closed form per (x, b, path):
// every real element's merged condition is evaluated on x and on b; if some element accepts neither row the path
// contributes nothing; otherwise with A = elements accepting x only (a of them) and C = elements accepting b only
// (c of them), a feature of A gets +val * T[a][c], a feature of C gets -val * T[c][a], and the bias cell gets val
// when a = 0 (b reaches the leaf). T[p][q] = (p-1)! q! / (p+q)! comes from the host (exact rationals rounded to
// fp64, [G][G]).
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
//   per reference: G = 8: 32 VGPR    G = 16: 32 VGPR    G = 32: 34 VGPR    G = 64: 37 VGPR
//   every instantiation: 0 bytes of scratch, 0 VGPR / SGPR spills, occupancy 8 waves per SIMD
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int SB_THREADS = 256;
constexpr int SB_R = 32;                // rows per block (BASELINE_ROW_TILE in ops/shap.py)
constexpr int SB_BT = 32;               // background rows per block (BG_TILE)
constexpr int SB_M = SB_R + SB_BT;      // ballots per wave and round
constexpr int SB_XS = SB_M + 1;         // X tile stride: lanes read different features of one row
constexpr int SB_X_BYTES = 12288;
constexpr int SB_PHI_BYTES = 16384;
constexpr long long SB_TRIPLES = 1LL << 36;  // (row, background row, path) triples per launch
constexpr int SB_NA_OK = 1, SB_IS_CAT = 2, SB_HAS_HI = 4;

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
    const int* __restrict__ p_cls, const double* __restrict__ T, int rounds, int use_x, int use_phi,
    double* __restrict__ out) {
  typedef typename sb_mask<G>::type M;
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
  for (int i = tid; i < phi_n; i += SB_THREADS) s_phi[i] = 0.0;
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
    if (first >= P) break;
    const int p = (int)first + tid / G;
    const bool valid = p < P;
    int feat = -1, flags = SB_NA_OK, coff = 0, cnb = 0, len = 1, cls = 0;
    double val = 0.0;
    float lo = 0.0f, hi = 0.0f;
    if (valid) {
      const long long q = (long long)p * G + e;
      feat = e_feat[q]; lo = e_lo[q]; hi = e_hi[q];
      flags = e_flags[q]; coff = e_coff[q]; cnb = e_cnb[q];
      len = p_len[p]; val = p_val[p]; cls = p_cls[p];
    }
    const int fe = feat < 0 ? 0 : feat;
    const bool na_ok = flags & SB_NA_OK, is_cat = flags & SB_IS_CAT, has_hi = flags & SB_HAS_HI;
    __syncthreads();                    // the staging above, and last round's readers of the ballots

    for (int i = 0; i < nrows + nb; ++i) {
      const int idx = i < nrows ? i : SB_R + (i - nrows);
      float v;
      if (use_x) v = s_x[fe * SB_XS + idx];
      else v = i < nrows ? X[(long long)fe * N + row0 + i] : Bg[(long long)fe * B + b0 + (i - nrows)];
      bool ok;
      if (v != v) {
        ok = na_ok;
      } else if (is_cat) {
        const int code = (int)v;
        ok = (code >= 0 && code < cnb) ? ((cat_bits[coff + (code >> 5)] >> (code & 31)) & 1u) != 0 : na_ok;
      } else {
        ok = v >= lo && (!has_hi || v < hi);
      }
      const unsigned long long m = __ballot(ok);
      if (lane == 0) wm[idx] = m;
    }
    __syncthreads();

    // elements 1 .. len-1 are real; the dummy root (bit 0) and the padding are in neither set
    const M realm = (M)((len >= 64 ? ~0ull : ((1ull << len) - 1ull)) & ~1ull);
    const M ebit = (M)((M)1 << e);
    const long long o_cell = (long long)cls * F1 + (e == 0 ? F : fe);
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
            unsafeAtomicAdd(&out[((row0 + r) * B + (b0 + j)) * K * F1 + o_cell], w * val);
        } else {
          acc += w;
        }
      }
      if (!PER_REF && acc != 0.0 && valid) {
        if (use_phi) atomicAdd(&s_phi[(long long)r * K * F1 + o_cell], acc * val);
        else unsafeAtomicAdd(&out[(row0 + r) * K * F1 + o_cell], acc * val);
      }
    }
  }

  if (use_phi) {
    __syncthreads();
    double* o = out + row0 * K * F1;
    const int n = nrows * K * F1;
    for (int i = tid; i < n; i += SB_THREADS) {
      const double c = s_phi[i];
      if (c != 0.0) unsafeAtomicAdd(&o[i], c);
    }
  }
}

}  // namespace

extern "C" {

// X: float32 [F][N], Bg: float32 [F][B]; element arrays [P][G], path arrays [P] (ops/shap.py PathTable); T:
// float64 [G][G], T[p][q] = (p-1)! q! / (p+q)!, row 0 unused. out: float64, accumulated into (the caller zeroes
// it): [N][K][F+1] summed over the background rows, or with per_ref [N*B][K][F+1] (pair i*B + j). The bias cell
// of a pair is the raw margin of its background row. rounds: groups of 256/G paths per block, 0 = pick from the
// grid size.
int h2o_tree_shap_baseline(const void* X, long long N, const void* Bg, long long B, int F, int K, int G, int P,
                           const void* e_feat, const void* e_lo, const void* e_hi, const void* e_flags,
                           const void* e_coff, const void* e_cnb, const void* cat_bits, const void* p_len,
                           const void* p_val, const void* p_cls, const void* T, int rounds, int per_ref, void* out,
                           void* stream) {
  if (N <= 0 || B <= 0 || P <= 0) return 0;
  if (F <= 0 || K <= 0 || (G != 8 && G != 16 && G != 32 && G != 64)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const long long per_round = SB_THREADS / G;
  const long long total_rounds = (P + per_round - 1) / per_round;
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
  if (rounds <= 0) {
    // about 2048 blocks when there is that much work; few pairs spread over the chip through the paths
    long long r = total_rounds * tiles / 2048;
    rounds = (int)(r < 1 ? 1 : r > 32 ? 32 : r);
  }
  const long long min_rounds = (total_rounds + 65534) / 65535;
  if (rounds < min_rounds) rounds = (int)min_rounds;
  const long long chunks = (total_rounds + rounds - 1) / rounds;
  const int use_x = (long long)F * SB_M * 4 <= SB_X_BYTES;
  const int use_phi = !per_ref && (long long)SB_R * K * (F + 1) * 8 <= SB_PHI_BYTES;
  size_t lds = (size_t)G * G * 8 + (size_t)(SB_THREADS / 64) * SB_M * 8;
  if (use_phi) lds += (size_t)SB_R * K * (F + 1) * 8;
  if (use_x) lds += (size_t)F * SB_XS * 4;
  const dim3 block(SB_THREADS);
#define SB_LAUNCH(GG, PR)                                                                                          \
  hipLaunchKernelGGL((k_shap_baseline<GG, PR>), grid, block, lds, s, (const float*)X, N, r0, r1,                   \
                     (const float*)Bg, B, c0, c1, F, K, P, (const int*)e_feat, (const float*)e_lo,                 \
                     (const float*)e_hi, (const int*)e_flags, (const int*)e_coff, (const int*)e_cnb,               \
                     (const uint32_t*)cat_bits, (const int*)p_len, (const double*)p_val, (const int*)p_cls,        \
                     (const double*)T, rounds, use_x, use_phi, (double*)out)
#define SB_PICK(GG)                   \
  do {                                \
    if (per_ref) SB_LAUNCH(GG, true); \
    else SB_LAUNCH(GG, false);        \
  } while (0)
  for (long long r0 = 0; r0 < N; r0 += rows_per_launch) {
    const long long r1 = r0 + rows_per_launch < N ? r0 + rows_per_launch : N;
    for (long long c0 = 0; c0 < B; c0 += bg_per_launch) {
      const long long c1 = c0 + bg_per_launch < B ? c0 + bg_per_launch : B;
      const dim3 grid((unsigned)((r1 - r0 + SB_R - 1) / SB_R), (unsigned)chunks,
                      (unsigned)((c1 - c0 + SB_BT - 1) / SB_BT));
      if (G == 8) SB_PICK(8);
      else if (G == 16) SB_PICK(16);
      else if (G == 32) SB_PICK(32);
      else SB_PICK(64);
    }
  }
#undef SB_PICK
#undef SB_LAUNCH
  return (int)hipGetLastError();
}

}  // extern "C"
