// The path table of ops/shap.py (PathTable, mirrored there as a ctypes.Structure) as the device sees it, and what
// k_tree_shap and k_shap_baseline share on the device and in their launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

struct PathView {                       // element arrays [P][G], path arrays [P]
  const int* __restrict__ feat;         // -1 = dummy root / padding
  const double* __restrict__ zf;
  const float* __restrict__ lo;
  const float* __restrict__ hi;
  const int* __restrict__ flags;        // PATH_NA_OK | PATH_IS_CAT | PATH_HAS_HI
  const int* __restrict__ cat_off;      // word offset into cat_bits
  const int* __restrict__ cat_nbits;
  const uint32_t* __restrict__ cat_bits;
  const int* __restrict__ len;          // elements of the path, dummy root included
  const double* __restrict__ value;
  const int* __restrict__ cls;
  int P, G;                             // G = 8 / 16 / 32 / 64: the smallest that holds the longest path
};

constexpr int PATH_NA_OK = 1, PATH_IS_CAT = 2, PATH_HAS_HI = 4;    // NA_OK / IS_CAT / HAS_HI in ops/shap.py

struct PathElem {                       // a lane's element and its path; the defaults are the dummy / padding element
  int feat = -1, flags = PATH_NA_OK, coff = 0, cnb = 0, len = 1, cls = 0;
  float lo = 0.0f, hi = 0.0f;
  double val = 0.0;
};

// Element e of path p; p >= P gives the padding element. Only k_tree_shap reads zero fractions: it passes a zf that
// holds the padding's 1.0, the baseline kernel passes none and gains no load.
template <int G>
__device__ __forceinline__ PathElem path_elem_load(const PathView& pv, int p, int e, double* zf = nullptr) {
  PathElem el;
  if (p < pv.P) {
    const long long q = (long long)p * G + e;
    if (zf) *zf = pv.zf[q];
    el.feat = pv.feat[q]; el.lo = pv.lo[q]; el.hi = pv.hi[q];
    el.flags = pv.flags[q]; el.coff = pv.cat_off[q]; el.cnb = pv.cat_nbits[q];
    el.len = pv.len[p]; el.val = pv.value[p]; el.cls = pv.cls[p];
  }
  return el;
}

// Does a row whose value of the element's feature is v follow the path there? NaN and a categorical code outside
// [0, cat_nbits) take NA_OK, else the merged bitset bit; numeric: lo <= v, and v < hi when there is a hi.
__device__ __forceinline__ bool path_elem_ok(const PathElem& el, const uint32_t* __restrict__ cat_bits, float v) {
  const bool na_ok = el.flags & PATH_NA_OK;
  if (v != v) return na_ok;
  if (!(el.flags & PATH_IS_CAT)) return v >= el.lo && (!(el.flags & PATH_HAS_HI) || v < el.hi);
  const int code = (int)v;
  return (code >= 0 && code < el.cnb) ? ((cat_bits[el.coff + (code >> 5)] >> (code & 31)) & 1u) != 0 : na_ok;
}

// The LDS phi tile (n cells) of a block of THREADS threads: zeroed before the rounds, then added to out[0..n) with
// native fp64 atomics, cells that stayed 0 skipped.
template <int THREADS>
__device__ __forceinline__ void phi_tile_zero(double* s_phi, int n) {
  for (int i = threadIdx.x; i < n; i += THREADS) s_phi[i] = 0.0;
}

template <int THREADS>
__device__ __forceinline__ void phi_tile_flush(const double* s_phi, double* __restrict__ out, int n) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += THREADS) {
    const double c = s_phi[i];
    if (c != 0.0) unsafeAtomicAdd(&out[i], c);
  }
}

// Sets the rounds (groups of threads / G paths) one block walks and returns the path chunks (grid y) that leaves.
// rounds <= 0: about 2048 blocks when the launch's `tiles` row tiles give that much work. Raised to fit grid y.
inline unsigned path_plan_rounds(const PathView& pv, int threads, long long tiles, int* rounds) {
  const long long per_round = threads / pv.G;
  const long long total_rounds = (pv.P + per_round - 1) / per_round;
  if (*rounds <= 0) {
    const long long r = total_rounds * tiles / 2048;
    *rounds = (int)(r < 1 ? 1 : r > 32 ? 32 : r);
  }
  const long long min_rounds = (total_rounds + 65534) / 65535;
  if (*rounds < min_rounds) *rounds = (int)min_rounds;
  return (unsigned)((total_rounds + *rounds - 1) / *rounds);
}

inline bool path_G_ok(int G) { return G == 8 || G == 16 || G == 32 || G == 64; }

// The runtime G and a flag as template arguments: calls fn(std::integral_constant<int, G>, std::bool_constant<flag>),
// for a generic lambda that launches k<decltype(g)::value, decltype(f)::value>.
template <typename Fn>
inline void path_dispatch(int G, bool flag, Fn&& fn) {
  auto pick = [&](auto g) { flag ? fn(g, std::true_type()) : fn(g, std::false_type()); };
  if (G == 8) pick(std::integral_constant<int, 8>());
  else if (G == 16) pick(std::integral_constant<int, 16>());
  else if (G == 32) pick(std::integral_constant<int, 32>());
  else pick(std::integral_constant<int, 64>());
}
