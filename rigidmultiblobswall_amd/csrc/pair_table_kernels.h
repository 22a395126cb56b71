// pair_table_kernels.h -- a radial pair law given as a table (gfx950, fp64): what the force sweep (TableLaw, sym_force_kernels.h)
// and the energy sweep (the TABLE instance of PotentialOp, potential_kernels.h) share.  No kernel is defined.
//
// The law (include/rmb_mobility.h, rmb_ctx_set_pair_table): K uniform intervals of width h from r0, one cubic per interval,
//   r0 <= r < r_cut = r0 + K h:  x = (r - r0)/h, k = min(floor(x), K - 1), t = x - k
//                               U = c0 + t (c1 + t (c2 + t c3)),  U' = (c1 + t (2 c2 + 3 t c3)) / h
//   r < r0:                     U = c[0][0] + (c[0][1]/h)(r - r0), U' = c[0][1]/h      (interval 0 at t = 0, continued linearly)
//   r >= r_cut:                 U = U' = +0.0
// The coefficients are 32-byte records (c0, c1, c2, c3).  A workgroup stages the K records into dynamic LDS once, before
// its waves start their walk (stage_pair_table: the one __syncthreads() of the kernel); a lane then fetches the record of
// its interval with 16-byte LDS reads.  Neighbouring lanes meet unrelated distances, so the gather has bank conflicts;
// profiles/r27_pair_table.json has what they cost.
//
// No lane ever forms an address outside the K records: the interval comes from x clamped to [0, K] (fmax drops a NaN, so
// coincident points -- r = 0 * inf -- and NaN coordinates land in interval 0), and the zero beyond the reach is a select
// on r2 < r_cut^2, not a clamp: padding lanes 2e100 apart read record K - 1 and give +0.0.
#pragma once
#include <hip/hip_runtime.h>

namespace rmb {

constexpr int kPairTableMax = 1024;     // intervals; 32 KiB of LDS next to the frame's own 14 KiB

struct PairTableRef {
  const double4* rec;   // [k] records in device memory
  int k;                // intervals, >= 1
  double r0, inv_h;
  double k_top;         // (double)k
  double rcut2;         // (r0 + k h)^2
};

// the workgroup's copy of the records (dynamic LDS: the launch asks for k * 32 bytes)
__device__ __forceinline__ double4* pair_table_lds() {
  extern __shared__ double4 rmb_pair_table_lds[];
  return rmb_pair_table_lds;
}

// every thread of the workgroup, once, before anything reads the table
__device__ __forceinline__ void stage_pair_table(const PairTableRef& t) {
  double4* lds = pair_table_lds();
  for (int i = threadIdx.x; i < t.k; i += blockDim.x) lds[i] = t.rec[i];
  __syncthreads();
}

// interval and offset of a distance: idx in [0, k - 1] whatever r is; tt in [0, 1] (0 in the core); x as it is
__device__ __forceinline__ void pair_table_locate(const PairTableRef& t, double r, int& idx, double& tt, double& x) {
  x = (r - t.r0) * t.inv_h;
  const double xc = fmin(fmax(x, 0.0), t.k_top);      // NaN -> 0
  idx = (int)fmin(xc, t.k_top - 1.0);                 // xc >= 0: the conversion truncates = floor
  tt = xc - (double)idx;
}

// U'(r) min(1/r, 1e25), the f0 of the force frame; exactly +0.0 from r_cut on
__device__ __forceinline__ double pair_table_f0(const PairTableRef& t, double r2, double r, double ir) {
  int idx; double tt, x;
  pair_table_locate(t, r, idx, tt, x);
  const double4 c = pair_table_lds()[idx];
  const double du = __builtin_fma(tt, __builtin_fma(3.0 * tt, c.w, 2.0 * c.z), c.y) * t.inv_h;
  const double f0 = du * fmin(ir, 1e25);
  return r2 < t.rcut2 ? f0 : 0.0;
}

// U(r); exactly +0.0 from r_cut on.  r is finite (the energy's r = r2 rsqrt(max(r2, 1e-300)))
__device__ __forceinline__ double pair_table_u(const PairTableRef& t, double r2, double r) {
  int idx; double tt, x;
  pair_table_locate(t, r, idx, tt, x);
  const double4 c = pair_table_lds()[idx];
  const double lead = x < 0.0 ? x : tt;               // the core continues interval 0 linearly: tt = 0 there
  const double u = __builtin_fma(lead, __builtin_fma(tt, __builtin_fma(tt, c.w, c.z), c.y), c.x);
  return r2 < t.rcut2 ? u : 0.0;
}

}  // namespace rmb
