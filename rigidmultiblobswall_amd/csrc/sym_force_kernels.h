// sym_force_kernels.h -- symmetric pair-force sweep (gfx950, fp64): blob-blob forces and body-body forces.
//
// F_ij = -F_ji, so each unordered pair is evaluated once (one rsqrt + one exp) and applied with opposite signs.  Same
// tile-pair rotation, LDS accumulation and static step schedule (sym_schedule.h) as sym_kernel; tile culling by the
// range of the exponential.  The pair law is a policy of the one frame: BlobContactLaw (multi_bodies/forces_numba.py:12-55
// semantics), BodyYukawaLaw (multi_bodies_functions.py:359-384, a Yukawa repulsion between body locations) or TableLaw (a
// radial law the user supplies as a table of cubics, pair_table_kernels.h).
#pragma once
#include "pair_ops.h"
#include "pair_table_kernels.h"
#include "sym_schedule.h"
#include "sym_walk.h"

namespace rmb {

struct SymForceArgs {
  const double4* pos;
  double* acc;          // [3][n_pad], zero on entry, re-zeroed by the finalize kernel
  double* out;          // [n][3]
  long n, n_pad;
  int n_tiles;
  long n_units;
  int order, xcd;       // as SymArgs
  long chunk_steps;     // > 0: steps per strided chunk of a wave; 0: one contiguous range per wave
  double Lx, Ly, Lz, iLx, iLy, iLz;
  double eps_over_b, inv_b, two_a;
  ExpConsts ec;
  const double* radii;  // RADII variant: one radius per blob, contact distance a_i + a_j (forces_numba.py:73-122)
  long step_begin, step_end;   // rotation steps [begin, end) of the n_units * 64 this launch covers (pair shard)
  // Tile culling (uniform radius; open or pseudo-periodic): bounds[T] = (xmin, ymin, zmin, xmax, ymax, zmax) of tile T
  // (tile_bounds_kernel), cull2 = (2a + 750 b)^2.  A tile pair whose boxes are further apart than that holds only
  // pairs with (r - 2a)/b > 750, for which exp underflows to exactly 0 here (exp_nonpositive) and in the reference
  // (exp(-745.2) is the smallest denormal): skipping the unit changes no bit of the result.  nullptr = no culling.
  const double* bounds;
  double cull2;
  // Spatially sorted configuration (rmb_sort.hip): `pos` is then the sorted copy and perm[s] the caller's index of
  // sorted slot s; the finalize kernel writes slot s to out[perm[s]].  nullptr = the caller's order.
  const unsigned* perm;
  double eps;           // BodyYukawaLaw: the strength itself (eps_over_b serves both laws)
  PairTableRef tab;     // TableLaw: the context's pair table; cull2 is its r_cut^2
};

// Pair laws: f0 with (force ON i) = f0 dr, dr = r_j - r_i; r2 = |dr|^2, r = |dr| and ir = 1/r come from the frame (one rsqrt
// per pair).  STAGED: the law keeps a table in the workgroup's dynamic LDS, which the kernel stages before the walk begins.
// Padding lanes sit 2e100 apart from everything: exp_nonpositive returns exactly 0 there, and so does every law.
//
// Blob-blob contact law, two_a = contact distance of the pair:
//   far: -(eps/b) exp(-(r-2a)/b) / r ;  near (r <= 2a): -(eps/b) / max(r, 1e-25) = -(eps/b) min(1/r, 1e25)
// Branch-free: x = min((2a - r)/b, 0) is 0 exactly for r <= 2a (and for r = NaN at coincident points, fmin keeps
// the number), exp(0) = 1 exactly, and min(1/r, 1e25) = 1/r for every r > 2a -- one expression serves both ranges.
struct BlobContactLaw {
  static constexpr bool STAGED = false;
  static __device__ __forceinline__ double f0(const SymForceArgs& a, double two_a, double, double r, double ir) {
    const double x = fmin((two_a - r) * a.inv_b, 0.0);
    const double e = exp_nonpositive(a.ec, x);
    // the multiplier first, the exponential last: beyond (r - 2a)/b = 708 e is a denormal, and e min(1/r, 1e25) would be
    // rounded to the denormal grid before eps/b scales it up again -- r times the error of one rounding of the result
    return -((a.eps_over_b * fmin(ir, 1e25)) * e);
  }
};

// Body-body Yukawa law, U = eps exp(-r/b) / r between body locations (multi_bodies_functions.py:383):
//   F_on_i = -(eps/b + eps/r) exp(-r/b) dr / r^2 ,  no contact distance (two_a is unused), no torque.
// One more multiply by 1/r than the contact law, no division.  Coincident locations (r = 0) divide by zero in the
// reference; here ir is not finite then, fmin keeps the exponent a number, and the two bodies of that pair -- no
// others -- get non-finite sums.
struct BodyYukawaLaw {
  static constexpr bool STAGED = false;
  static __device__ __forceinline__ double f0(const SymForceArgs& a, double, double, double r, double ir) {
    const double e = exp_nonpositive(a.ec, fmin(-r * a.inv_b, 0.0));
    return -((__builtin_fma(a.eps, ir, a.eps_over_b) * (ir * ir)) * e);      // the denormal e last, as above
  }
};

// Tabulated radial law U(r) (pair_table_kernels.h): F_on_i = (U'(r)/r) dr, f0 = U'(r) min(1/r, 1e25) as the contact law's
// near branch, so coincident blobs (dr = 0, r = NaN) give a zero force; +0.0 exactly from r_cut on (padding included).
// No contact distance (two_a is unused), no exponential.
struct TableLaw {
  static constexpr bool STAGED = true;
  static __device__ __forceinline__ double f0(const SymForceArgs& a, double, double r2, double r, double ir) {
    return pair_table_f0(a.tab, r2, r, ir);
  }
};

// LAW::f0(r) dr for one pair; dr = r_j - r_i (minimal image in every direction with L > 0).
// Returns the force ON i; the force on j is minus it.
template <bool PERIODIC, class LAW>
__device__ __forceinline__ void pair_force(const SymForceArgs& a, double two_a, double dx, double dy, double dz, double& fx,
                                           double& fy, double& fz) {
  if constexpr (PERIODIC) {
    if (a.Lx > 0) dx = wrap_nearest_pad_safe(dx, a.Lx, a.iLx);
    if (a.Ly > 0) dy = wrap_nearest_pad_safe(dy, a.Ly, a.iLy);
    if (a.Lz > 0) dz = wrap_nearest_pad_safe(dz, a.Lz, a.iLz);
  }
  const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
  const double ir = rsqrt_f64(r2);
  const double r = r2 * ir;
  const double f0 = LAW::f0(a, two_a, r2, r, ir);
  fx = f0 * dx; fy = f0 * dy; fz = f0 * dz;
}

// steps per chunk of the force sweeps: the planned chunk, or one contiguous range per wave
__device__ __forceinline__ long sym_force_spw(const SymForceArgs& a, long n_waves) {
  return a.chunk_steps > 0 ? a.chunk_steps : (a.step_end - a.step_begin + n_waves - 1) / n_waves;
}

template <bool PERIODIC, bool RADII = false, class LAW = BlobContactLaw>
__global__ __launch_bounds__(64 * kSymWaves) void sym_force_kernel(const SymForceArgs a) {
  __shared__ double4 rec_all[kSymWaves][64];
  __shared__ double accj_all[kSymWaves][3 * 64];

  struct Body {
    const SymForceArgs& a;
    const int lane;
    double4* const rec;
    double* const accj;
    long i;
    bool vi_ok;
    double xi, yi, zi, ri;
    double ax, ay, az;

    __device__ __forceinline__ Body(const SymForceArgs& a, int lane, double4* rec, double* accj) : a(a), lane(lane), rec(rec), accj(accj) {}
    __device__ __forceinline__ void begin() {
      i = 0;
      vi_ok = false;
      xi = 0; yi = 0; zi = 0; ri = 0;
      ax = 0; ay = 0; az = 0;
    }
    // every pair of the unit is beyond the range of the exponential: contributes exactly zero
    __device__ __forceinline__ bool culled(int I, int J) const {
      return a.bounds != nullptr && I != J &&
             tile_gap2(a.bounds, I, J, PERIODIC ? a.Lx : 0.0, PERIODIC ? a.Ly : 0.0, PERIODIC ? a.Lz : 0.0) > a.cull2;
    }
    __device__ __forceinline__ void flush_row(long) {
      if (!vi_ok) return;
      __hip_atomic_fetch_add(&a.acc[i], ax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&a.acc[a.n_pad + i], ay, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&a.acc[2 * a.n_pad + i], az, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void load_row(int I) {
      i = 64L * I + lane;
      vi_ok = i < a.n;
      xi = 1e100; yi = 1e100; zi = 1e100;
      if (vi_ok) { const double4 p = a.pos[i]; xi = p.x; yi = p.y; zi = p.z; }
      if constexpr (RADII) ri = vi_ok ? a.radii[i] : 0.0;
      ax = 0.0; ay = 0.0; az = 0.0;
    }
    __device__ __forceinline__ void unit(int I, int J, int k0, int k1, long) {
      {
        const long j = 64L * J + lane;
        double4 p = make_double4(-1e100, -1e100, -1e100, 0.0);
        if (j < a.n) p = a.pos[j];
        if constexpr (RADII) p.w = (j < a.n) ? a.radii[j] : 0.0;   // w is free here: forces use unclamped positions (b = 1)
        rec[lane] = p;
        accj[lane] = 0.0; accj[64 + lane] = 0.0; accj[128 + lane] = 0.0;
      }
      wave_lds_sync();
      const bool diag = (I == J);
      for (int k = (diag && k0 < 1) ? 1 : k0; k < k1; ++k) {
        const int jj = (lane + k) & 63;
        const double4 q = rec[jj];
        double fx, fy, fz;
        pair_force<PERIODIC, LAW>(a, RADII ? ri + q.w : a.two_a, q.x - xi, q.y - yi, q.z - zi, fx, fy, fz);
        ax += fx; ay += fy; az += fz;
        if (!diag) {   // wave-uniform
          // the LDS slab collects +f (ds_add_f64 has no negate modifier: -f would cost a v_xor + v_mov per component
          // and step); the sign of the reaction goes into the flush below
          __hip_atomic_fetch_add(&accj[jj], fx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          __hip_atomic_fetch_add(&accj[64 + jj], fy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          __hip_atomic_fetch_add(&accj[128 + jj], fz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
      }
      if (!diag) {
        wave_lds_sync();
        const long j = 64L * J + lane;
        if (j < a.n) {
          __hip_atomic_fetch_add(&a.acc[j], -accj[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(&a.acc[a.n_pad + j], -accj[64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(&a.acc[2 * a.n_pad + j], -accj[128 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      __builtin_amdgcn_wave_barrier();   // accj / rec are rewritten by the next unit
    }
  };

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  Body body(a, threadIdx.x & 63, rec_all[wave], accj_all[wave]);
  if constexpr (LAW::STAGED) stage_pair_table(a.tab);      // once per workgroup, before any wave starts its walk
  const long n_waves = sym_n_waves();
  sym_walk(SymWalk{a.order, a.n_tiles, a.step_begin, a.step_end, sym_force_spw(a, n_waves), n_waves, sym_wave(a.xcd)}, body);
}

static __global__ __launch_bounds__(256) void sym_force_finalize_kernel(const SymForceArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const long o = a.perm ? (long)a.perm[i] : i;
  a.out[3 * o] = a.acc[i]; a.out[3 * o + 1] = a.acc[a.n_pad + i]; a.out[3 * o + 2] = a.acc[2 * a.n_pad + i];
  a.acc[i] = 0.0; a.acc[a.n_pad + i] = 0.0; a.acc[2 * a.n_pad + i] = 0.0;
}

}  // namespace rmb
