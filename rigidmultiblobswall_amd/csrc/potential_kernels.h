// potential_kernels.h -- total potential energy of a blob configuration (gfx950, fp64): the equilibrium sampler's hot path.
//
// U = sum_i u1(z_i) + sum_{i<j} u2(r_ij), the reference's many_bodyMCMC/many_body_potential_pycuda.py:64-119 (one thread
// per blob, inner loop j > i over global memory).  Here every unordered pair is met once by the pair-once frame
// (pair_once_kernels.h: tile pairs I <= J, lane = blob of tile I, tile J rotated through the wave's LDS slab, strided
// chunks, tile bounds and exact-zero culling); this file holds the energy's policy of it and the kernel around the call.
// The result is a scalar, so there is nothing to transpose: every lane keeps two fp64 sums (one-blob, pair) for
// the whole launch, a wave reduces its lanes with a fixed butterfly and stores ONE pair of partials, and
// potential_finish_kernel adds the partials in a fixed order -- no atomic anywhere, bit-reproducible for a given launch
// plan and permutation.  The one-blob terms ride on step 0 of the diagonal units (the step the force kernel leaves empty),
// so the finishing kernel never touches the positions.
//
// Semantics of the reference kernel that are reproduced:
//   * a blob with z <= 0 contributes 1e5 (1 - z) and nothing else AS THE LOWER INDEX of a pair: the pair (i, j), i < j in
//     the caller's order, counts iff z_i > 0.  Record .w carries the caller's index (perm[s] of the Morton-sorted copy).
//     Units whose two tiles lie above the wall (zmin > 0, wave-uniform from the tile bounds) skip the test.
//   * minimal image in x and y only; distinct blobs at r = 0 give the finite contact value (soft) / inf (yukawa).
//
// BODY: the same sweep over body LOCATIONS, U_body = sum_{i<j} eps exp(-r_ij/b) / r_ij -- the energy whose gradient is
// BodyYukawaLaw (sym_force_kernels.h).  The yukawa pair expression with three differences: the minimal image in every direction
// with a positive period, z included (the image rule of the force law); no wall gate and no one-blob term (a centre with
// z <= 0 counts in full); one result.  Tile culling by 750 b with the z period in the tile gap.
//
// TABLE: the pair term is the context's tabulated radial law (pair_table_kernels.h) instead of the FORM's; the one-blob term,
// the wall gate and the x-y minimal image are the blob forms' own, FORM still chooses the one-blob expression.  Distinct
// blobs at r = 0 give the core's finite value c[0][0] - c[0][1] r0 / h.  Tile culling by r_cut.
#pragma once
#include "pair_once_kernels.h"
#include "pair_table_kernels.h"

namespace rmb {

enum PotentialForm : int { POT_SOFT = 0, POT_YUKAWA = 1 };

// bounds are always present; Lz, iLz: BODY only (the blob forms ignore periodic_length[2])
struct PotentialArgs : PairOnceArgs {
  const unsigned* perm; // sorted slot -> caller's index, or nullptr
  double eps, inv_b, two_a;              // pair term
  double eps_wall, inv_b_wall, a, weight;  // one-blob term
  ExpConsts ec;
  double* partial;      // [n_waves][2] = (one-blob, pair) sums of every wave of the launch
  long n_partial;       // n_waves
  double* out;          // {U_one_blob, U_pair}; BODY: {U_body}
  int n_out;            // 2, BODY: 1
  PairTableRef tab;     // TABLE: the context's pair table; cull2 is its r_cut^2
};

// exp of any argument from exp_nonpositive: 1 / exp(-x) for x > 0 (one more rounding; inf where exp overflows).  The
// library exp costs the whole kernel some twenty registers for N evaluations per sweep.
__device__ __forceinline__ double exp_any(const ExpConsts& ec, double x) {
  const double e = exp_nonpositive(ec, -fabs(x));
  return x > 0.0 ? 1.0 / e : e;
}

// gravity + wall repulsion of one blob above the wall (z > 0)
template <int FORM>
__device__ __forceinline__ double one_blob_potential(const PotentialArgs& a, double z) {
  double u = a.weight * z;
  if (a.eps_wall != 0.0) {
    if constexpr (FORM == POT_SOFT) {
      const double x = (a.a - z) * a.inv_b_wall;        // as the pair term: e_w (exp(min(x, 0)) + max(x, 0))
      u += a.eps_wall * (exp_nonpositive(a.ec, fmin(x, 0.0)) + fmax(x, 0.0));
    } else {
      u += a.eps_wall * a.a * exp_any(a.ec, (a.a - z) * a.inv_b_wall) / fabs(z - a.a);
      if (z < a.a) u += a.eps_wall * 1e12;
    }
  }
  return u;
}

// u2 of one pair from its separation (already the minimal image)
template <int FORM>
__device__ __forceinline__ double pair_potential(const PotentialArgs& a, double dx, double dy, double dz) {
  const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
  if constexpr (FORM == POT_SOFT) {
    // r = r2 rsqrt(r2) is 0 * inf at coincident blobs: the floor keeps rsqrt finite there (r = 0 * 1e150 = 0) and changes
    // no other r (r2 < 1e-300 gives r < 1e-150 either way)
    const double r = r2 * rsqrt_f64(fmax(r2, 1e-300));
    // r < 2a: eps + eps (2a - r)/b, else eps exp(-(r - 2a)/b); one expression, exp(0) = 1 exactly
    const double x = (a.two_a - r) * a.inv_b;
    return a.eps * (exp_nonpositive(a.ec, fmin(x, 0.0)) + fmax(x, 0.0));
  } else {
    // 1/r = inf at r = 0, as the reference's division (the refinement steps of rsqrt_f64 turn rsq(0) = inf into NaN)
    const double ir = r2 > 0.0 ? rsqrt_f64(r2) : __builtin_inf();
    const double r = r2 > 0.0 ? r2 * ir : 0.0;
    return a.eps * exp_nonpositive(a.ec, -r * a.inv_b) * ir;
  }
}

// u2 of one pair from the table (separation already the minimal image); r as the soft form takes it: finite at r2 = 0
__device__ __forceinline__ double table_potential(const PotentialArgs& a, double dx, double dy, double dz) {
  const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
  const double r = r2 * rsqrt_f64(fmax(r2, 1e-300));
  return pair_table_u(a.tab, r2, r);
}

// separation in z: the blob forms take it as it is, the body centres take its minimal image
template <bool PERIODIC, bool BODY>
__device__ __forceinline__ double image_z(const PotentialArgs& a, double d) {
  if constexpr (BODY) return image<PERIODIC>(a.Lz, a.iLz, d);
  return d;
}

// The energy as a policy of the pair-once frame (pair_once_kernels.h)
template <int FORM, bool PERIODIC, bool BODY, bool TABLE = false>
struct PotentialOp {
  static_assert(!BODY || FORM == POT_YUKAWA, "the body-body law is the yukawa pair expression");
  static_assert(!BODY || !TABLE, "the tabulated law is a blob-blob law");
  typedef PotentialArgs Args;
  struct Lane { double u_one, u_pair; };
  static constexpr bool FRAMES = false;
  static constexpr double PAD_W = 1e18;      // record .w: the caller's index; padding lies beyond every index
  static __device__ __forceinline__ double4 fetch(const Args& a, long, long i) {
    double4 p = a.pos[i];
    p.w = (double)(a.perm ? (long)a.perm[i] : i);
    return p;
  }
  // beyond the reach of the exponential every term of the unit is exactly zero
  static __device__ __forceinline__ bool culled(const Args& a, int I, int J) {
    return tile_gap2(a.bounds, I, J, PERIODIC ? a.Lx : 0.0, PERIODIC ? a.Ly : 0.0, PERIODIC && BODY ? a.Lz : 0.0) > a.cull2;
  }
  // the one-blob terms ride on step 0 of the diagonal units
  static __device__ __forceinline__ void diag_start(const Args& a, Lane& st, const double4& self, bool valid) {
    if constexpr (!BODY) {
      if (valid) st.u_one += (self.z > 0.0) ? one_blob_potential<FORM>(a, self.z) : 1e5 * (1.0 - self.z);
    }
  }
  // a tile that reaches the wall plane (zmin <= 0) needs the lower-index test of the reference's loop limits
  // (BODY: no gate at all -- padding sits 2e100 away, where the exponential is exactly 0)
  static __device__ __forceinline__ bool guarded(const Args& a, int I, int J) {
    return !BODY && !(a.bounds[6L * I + 2] > 0.0 && a.bounds[6L * J + 2] > 0.0);
  }
  template <bool GUARDED>
  static __device__ __forceinline__ void pair(const Args& a, Lane& st, const double4& self, const double4& q, bool take) {
    const double dx = image<PERIODIC>(a.Lx, a.iLx, self.x - q.x), dy = image<PERIODIC>(a.Ly, a.iLy, self.y - q.y);
    const double dz = image_z<PERIODIC, BODY>(a, self.z - q.z);
    double u;
    if constexpr (TABLE) u = table_potential(a, dx, dy, dz);
    else                 u = pair_potential<FORM>(a, dx, dy, dz);
    if constexpr (GUARDED) {
      const double z_low = self.w < q.w ? self.z : q.z;      // the blob with the lower caller's index decides
      const bool real = self.w < 1e17 && q.w < 1e17;         // padding carries index PAD_W
      st.u_pair += (!take || !real || !(z_low > 0.0)) ? 0.0 : u;
    } else {
      st.u_pair += take ? u : 0.0;
    }
  }
};

template <int FORM, bool PERIODIC, bool BODY = false, bool TABLE = false>
__global__ __launch_bounds__(64 * kSymWaves) void potential_kernel(const PotentialArgs a) {
  typedef PotentialOp<FORM, PERIODIC, BODY, TABLE> OP;
  __shared__ double4 rec_all[kSymWaves][64];
  if constexpr (TABLE) stage_pair_table(a.tab);      // once per workgroup, before any wave starts its walk
  typename OP::Lane st{0.0, 0.0};
  pair_once_sweep<OP>(a, st, rec_all[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
  // fixed butterfly over the lanes, one pair of partials per wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    st.u_one += __shfl_xor(st.u_one, off);
    st.u_pair += __shfl_xor(st.u_pair, off);
  }
  const long w = pair_once_wave(a);
  if ((threadIdx.x & 63) == 0) { a.partial[2 * w] = st.u_one; a.partial[2 * w + 1] = st.u_pair; }
}

// adds the per-wave partials in a fixed order (thread t: t, t + 256, ...; then a tree over the 256 threads)
static __global__ __launch_bounds__(256) void potential_finish_kernel(const PotentialArgs a) {
  __shared__ double s[2][256];
  double u0 = 0.0, u1 = 0.0;
  for (long k = threadIdx.x; k < a.n_partial; k += 256) { u0 += a.partial[2 * k]; u1 += a.partial[2 * k + 1]; }
  s[0][threadIdx.x] = u0; s[1][threadIdx.x] = u1;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) { s[0][threadIdx.x] += s[0][threadIdx.x + off]; s[1][threadIdx.x] += s[1][threadIdx.x + off]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (a.n_out == 1) a.out[0] = s[1][0];      // BODY: the one-blob sums are zeros
    else { a.out[0] = s[0][0]; a.out[1] = s[1][0]; }
  }
}

}  // namespace rmb
