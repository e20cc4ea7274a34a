// Lock-free union-find over an int parent[] in LDS or global memory, shared by the two clustering kernels (k_largest_cluster in postprocess.hip,
// k_isolate_cluster in isolation.hip).  A root is always the smallest index of its component, so parents only ever decrease and the numbering of the
// components by their first point comes out without a relabelling pass.
#pragma once

#ifdef __HIPCC__
__device__ __forceinline__ int sv_uf_find(volatile int* parent, int x) {
  int p = parent[x];
  while (p != x) {
    const int g = parent[p];
    if (g != p) parent[x] = g;       // path halving (parents only ever decrease)
    x = p, p = g;
  }
  return x;
}

// Joins the components of a and b: the larger root is hung under the smaller with a CAS, retried when another lane moved that root meanwhile.
__device__ __forceinline__ void sv_uf_union(int* parent, int a, int b) {
  while (true) {
    a = sv_uf_find(parent, a), b = sv_uf_find(parent, b);
    if (a == b) break;
    if (a > b) { const int t = a; a = b; b = t; }
    if (atomicCAS(&parent[b], b, a) == b) break;
  }
}
#endif
