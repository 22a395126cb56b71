// cluster_kernels.h -- connected components of the bond graph of a point configuration (gfx950, fp64 distances, int32
// labels): which points belong together.  ClusterOp is a policy of the pair-once frame (pair_once_kernels.h), as
// PairHistOp is; the first sweep whose result is a partition and not a sum.
//
// Points i and j of one frame are bonded when d_ij^2 < r_cut^2, strictly: the separation in the minimal image of every
// direction with a positive period (image<>, the pair histogram's formula, any number of periods away), d^2 =
// dx^2 + dy^2 + dz^2 formed as hist_pair forms it (plane xyz) or dx^2 + dy^2 (plane xy: z and L_z are ignored).  Coincident
// and -- under xy -- stacked points have d = 0 and ARE bonded.  A cluster is a connected component; its label is the
// smallest index in it.  With a selection (one byte per point) only bonds between two selected points exist.
//
// Three launches: cluster_init_kernel (parent = identity, sizes = 0), the sweep (cluster_kernel), cluster_finish_kernel.
//
// The record's .w carries the point's index in the flat `parent` array as a double (exact below 2^53; the host refuses
// more than 2^31 - 1 entries): frame * n + i in the BATCH layout, the CALLER's index in the resident layout (through `perm`
// when the sweep runs on the Morton-sorted copy).  An unselected point and a padding record carry -1 and are never united.
//
// The union-find (unite / find below) lives in global memory and takes no lock.
//   Invariant  parent[x] <= x at every moment, with equality exactly at roots.  It holds after the init launch.  The only
//              writes of the sweep are atomicCAS(&parent[hi], hi, lo) with lo < hi, which can only succeed while hi is a
//              root, and atomicMin(&parent[x], r) with r < x an ancestor of x, issued only for an x that has been seen
//              with a parent below itself.  Both lower a value, neither makes a root of a non-root: a point that has
//              stopped being a root never becomes one again.
//   Stale reads  Every read of `parent` in the sweep is a relaxed atomic load at agent scope (the waves of one launch sit
//              on eight XCDs; the compiler may not keep a parent in a register across the loop).  Since parent[x] only
//              ever decreases and every value it has held is an ancestor-or-self of x, a stale value is an OLDER
//              ancestor-or-self: the walk merely starts higher up the same path.  Harmless.
//   Termination  find follows strictly decreasing indices, so it ends.  In unite, a failed CAS returns the present parent
//              of hi, which is below hi; the loop goes on from that value, so max(a, b) strictly decreases over failed
//              attempts and the loop ends.  No lane waits for another lane's progress: a failed CAS means another lane HAS
//              hooked hi.  Lock-free, not a lock; lanes of one wave may diverge freely.
//   Determinism  A hook puts the larger root under the smaller, so by induction a root is the minimum of its set.  When the
//              sweep's kernel has ended every bonded pair has been united, the sets are the connected components, and the
//              root of every point -- what the finishing launch reads, with plain loads -- is the smallest index of its
//              component, whatever the interleaving, launch plan, point order or culling choice was.  The shape of the
//              trees differs from run to run; the roots do not.
//
// The finishing launch: one thread per point; labels[k] = find(k) - frame * n for a selected point (-1 otherwise) and one
// integer atomicAdd per selected point to sizes[root]: sizes[f][l] is the size of the cluster labelled l, 0 where l is
// nobody's label.  No floating-point atomic, no spin-wait anywhere.
//
// Culling (resident layout): an off-diagonal tile pair is skipped when the gap between the two bounding boxes exceeds
// r_cut^2.  Under plane xy the gap is taken WITHOUT its z term (tile_gap2 over two directions): a 3-D gap would drop the
// bonds between tiles stacked in z.  The gap is a lower bound of every d^2 of the unit formed by the same monotone
// roundings in the same order, so no bond is dropped.
#pragma once
#include "pair_once_kernels.h"

namespace rmb {

struct ClusterArgs : PairOnceArgs {      // pos, bounds, cull2 (r_cut^2, +inf = no culling): resident only
  double rc2;                    // r_cut^2
  int xy;                        // 1: d is the in-plane distance (Lz = 0)
  int* parent;                   // [total]
  const unsigned char* select;   // [total], caller's order; nullptr: every point
  const unsigned* perm;          // resident, sorted copy: perm[s] = caller's index of slot s; nullptr = caller's order
  // BATCH only (step_end = n_frames * units_per_frame * 64)
  const double* frames;          // (n_frames, n, 3)
  long units_per_frame;          // n_tiles (n_tiles + 1) / 2
  // init and finishing launches
  long total;                    // n_frames * n  (resident: n)
  int* labels;                   // [total]
  int* sizes;                    // [total]
};

__device__ __forceinline__ int cluster_load(const int* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x as this lane sees it now (a root of a moment ago may have been hooked since: unite's CAS is the judge)
__device__ __forceinline__ int cluster_find(const int* parent, int x) {
  for (;;) {
    const int p = cluster_load(parent, x);
    if (p == x) return x;
    x = p;
  }
}

// find with one step of path compression: the start point is moved up to the root that was found
__device__ __forceinline__ int cluster_find_compress(int* parent, int x) {
  const int p = cluster_load(parent, x);
  if (p == x) return x;
  const int r = cluster_find(parent, p);
  if (r < p) atomicMin(parent + x, r);      // x is not a root (p < x) and r is an ancestor of x
  return r;
}

__device__ __forceinline__ void cluster_unite(int* parent, int i, int j) {
  int a = cluster_find_compress(parent, i), b = cluster_find_compress(parent, j);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;                 // hi was a root and now hangs under lo
    a = cluster_find(parent, old);         // hi had been hooked by another lane: go on from its parent (old < hi)
    b = cluster_find(parent, lo);
  }
}

template <bool PERIODIC, bool BATCH>
struct ClusterOp {
  typedef ClusterArgs Args;
  struct Lane {};
  static constexpr bool FRAMES = BATCH;
  static constexpr double PAD_W = -1.0;      // no index: never united
  static __device__ __forceinline__ double4 fetch(const Args& a, long frame, long i) {
    if constexpr (BATCH) {
      const long k = frame * a.n + i;
      const double* p = a.frames + 3 * k;
      const bool sel = !a.select || a.select[k];
      return make_double4(p[0], p[1], p[2], sel ? (double)k : -1.0);
    } else {
      const double4 p = a.pos[i];
      const long o = a.perm ? (long)a.perm[i] : i;
      const bool sel = !a.select || a.select[o];
      return make_double4(p.x, p.y, p.z, sel ? (double)o : -1.0);
    }
  }
  static __device__ __forceinline__ bool culled(const Args& a, int I, int J) {
    if constexpr (BATCH) return false;      // no bounds
    else return tile_gap2(a.bounds, I, J, PERIODIC ? a.Lx : 0.0, PERIODIC ? a.Ly : 0.0, PERIODIC ? a.Lz : 0.0, a.xy ? 2 : 3) > a.cull2;
  }
  static __device__ __forceinline__ void diag_start(const Args&, Lane&, const double4&, bool) {}
  static __device__ __forceinline__ bool guarded(const Args&, int, int) { return false; }
  template <bool GUARDED>
  static __device__ __forceinline__ void pair(const Args& a, Lane&, const double4& self, const double4& q, bool take) {
    const double dx = image<PERIODIC>(a.Lx, a.iLx, self.x - q.x);
    const double dy = image<PERIODIC>(a.Ly, a.iLy, self.y - q.y);
    const double dz = a.xy ? 0.0 : image<PERIODIC>(a.Lz, a.iLz, self.z - q.z);
    const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));      // hist_pair's arithmetic
    if (take && r2 < a.rc2 && self.w >= 0.0 && q.w >= 0.0) cluster_unite(a.parent, (int)self.w, (int)q.w);
  }
};

__global__ __launch_bounds__(256) void cluster_init_kernel(const ClusterArgs a) {
  const long k = 256L * blockIdx.x + threadIdx.x;
  if (k < a.total) { a.parent[k] = (int)k; a.sizes[k] = 0; }
}

template <bool PERIODIC, bool BATCH>
__global__ __launch_bounds__(64 * kSymWaves) void cluster_kernel(const ClusterArgs a) {
  typedef ClusterOp<PERIODIC, BATCH> OP;
  __shared__ double4 rec_all[kSymWaves][64];
  typename OP::Lane st{};
  pair_once_sweep<OP>(a, st, rec_all[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
}

// after the sweep's kernel boundary: plain loads
__global__ __launch_bounds__(256) void cluster_finish_kernel(const ClusterArgs a) {
  const long k = 256L * blockIdx.x + threadIdx.x;
  if (k >= a.total) return;
  if (a.select && !a.select[k]) { a.labels[k] = -1; return; }
  int r = (int)k;
  for (int p = a.parent[r]; p != r; p = a.parent[r]) r = p;
  a.labels[k] = r - (int)((k / a.n) * a.n);
  atomicAdd(a.sizes + r, 1);
}

}  // namespace rmb
