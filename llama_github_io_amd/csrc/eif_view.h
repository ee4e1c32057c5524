// The packed Extended Isolation Forest of ops/eif.py pack() (mirrored there as a ctypes.Structure) as the device sees
// it: hyperplane splits with sparse normals, every index absolute over the whole forest.
#pragma once

struct EifView {                        // node arrays [n_nodes], tree arrays [n_trees], in pack()'s order
  const int* __restrict__ left;         // children, absolute node indices; -1 = leaf
  const int* __restrict__ right;
  const double* __restrict__ off;       // the row goes left iff (sum_k x[nz_feat[k]] * nz_val[k]) - off <= 0
  const double* __restrict__ value;     // leaf: the path length it contributes, depth + c(rows)
  const int* __restrict__ nz_begin;     // [n_nodes + 1]: the node's listed components are [nz_begin[n], nz_begin[n + 1])
  const int* __restrict__ nz_feat;      // feature ascending within a node
  const double* __restrict__ nz_val;
  const int* __restrict__ roots;
  int n_trees, n_nodes;
};
