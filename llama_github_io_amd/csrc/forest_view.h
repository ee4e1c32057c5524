// The flat forest of Forest.flatten (ops/forest.py, mirrored there as a ctypes.Structure) as the device sees it, and
// the one rule that says where a row goes at a split, for every kernel that walks the forest.
#pragma once

struct ForestView {                     // node arrays [n_nodes], tree arrays [n_trees], in Forest.flatten's order
  const int* __restrict__ feat;         // -1 = leaf
  const float* __restrict__ thr;        // numeric: x < thr goes left
  const int* __restrict__ left;         // children, absolute node indices
  const int* __restrict__ right;
  const int* __restrict__ na_left;
  const int* __restrict__ cat_off;      // -1 = numeric, else the word offset of the node's bitset in cat_bits
  const unsigned* __restrict__ cat_bits;
  const int* __restrict__ cat_nbits;
  const float* __restrict__ value;
  const int* __restrict__ roots;
  const int* __restrict__ cls;
  int n_trees, n_nodes;
};

// NaN and a categorical code outside [0, cat_nbits) take na_left, else the bitset bit decides; numeric: x < thr.
__device__ __forceinline__ bool forest_go_left(const ForestView& fv, int n, float x) {
  bool go_left;
  if (x != x) go_left = fv.na_left[n] != 0;
  else if (fv.cat_off[n] >= 0) {
    const int code = (int)x;
    if (code < 0 || code >= fv.cat_nbits[n]) go_left = fv.na_left[n] != 0;
    else go_left = (fv.cat_bits[fv.cat_off[n] + (code >> 5)] >> (code & 31)) & 1u;
  } else go_left = x < fv.thr[n];
  return go_left;
}
