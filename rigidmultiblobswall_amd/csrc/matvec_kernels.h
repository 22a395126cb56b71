// matvec_kernels.h -- the O(N^2) pairwise mobility sweep and the blob-blob force sweep (gfx950), as policies of the
// one-sided frame (onesided_kernels.h: lane = target, sources streamed through an LDS tile, fixed-order reduction).
//
// Mobility: a record is (x, y, z, b*v) with the B-damping fused into the staging.  The pair loop has no self test:
// pairs with i == j contribute through `self_term` in the epilogue and are skipped only in the one tile that overlaps
// the workgroup's own targets.
#pragma once
#include "pair_blocks.h"
#include "onesided_kernels.h"

namespace rmb {

struct SweepArgs : OneSidedArgs {
  const double4* pos;   // [n_src]  (x, y, z_eff, b)   b = B-damping factor (1 if not overlapping / no wall); targets index it too
  const double* vec;    // [3 n_src] source vector (force or torque), AoS as the reference's (N,3)
  const double* vec2;   // [3 n_src] torque for the fused tt+tr kind, else nullptr
  int in_plane;             // zero v_z on load and u_z on store (in_plane_* kernels of the reference)
  double prefactor;         // 1/(8 pi eta)
  double Lx, Ly, Lz;        // pseudo-periodic lengths (<= 0: open)
  double iLx, iLy, iLz;     // 1/L (0 when open)
  PairConsts k;
};

template <int KIND> struct Rec { static constexpr int n2 = kind_has_torque(KIND) ? 5 : 3; };

template <int KIND, bool WALL, bool PERIODIC> struct SweepOp {
  typedef SweepArgs Args;
  typedef double4 Target;
  static constexpr int NOUT = 3, REC2 = Rec<KIND>::n2;
  static constexpr bool SHARDED = true, SKIP_OWN_TILE = true;

  static __device__ __forceinline__ Target load_target(const Args& a, long t) { return a.pos[t]; }

  static __device__ __forceinline__ void stage(const Args& a, long j, double2* rec) {
    const double4 p = a.pos[j];
    const double b = p.w;
    double vx = a.vec[3 * j] * b, vy = a.vec[3 * j + 1] * b, vz = a.vec[3 * j + 2] * b;
    if (a.in_plane) vz = 0.0;
    rec[0] = make_double2(p.x, p.y);
    rec[1] = make_double2(p.z, vx);
    rec[2] = make_double2(vy, vz);
    if constexpr (kind_has_torque(KIND)) {
      double wx = a.vec2[3 * j] * b, wy = a.vec2[3 * j + 1] * b, wz = a.vec2[3 * j + 2] * b;
      if (a.in_plane) wz = 0.0;
      rec[3] = make_double2(wx, wy);
      rec[4] = make_double2(wz, 0.0);
    }
  }

  template <bool SKIP_SELF>
  static __device__ __forceinline__ void tile_pairs(const Args& a, const double2* tile, int n, int wave, long j0, long ti,
                                                    const Target& tp, double* out) {
    const double xi = tp.x, yi = tp.y, zi = tp.z;
    Vec3 acc = {out[0], out[1], out[2]};
    for (int s = wave; s < n; s += kWaves) {
      const double2 q0 = tile[s * REC2 + 0];
      const double2 q1 = tile[s * REC2 + 1];
      const double2 q2 = tile[s * REC2 + 2];
      double wx = 0, wy = 0, wz = 0;
      if constexpr (kind_has_torque(KIND)) {
        const double2 q3 = tile[s * REC2 + 3];
        const double2 q4 = tile[s * REC2 + 4];
        wx = q3.x; wy = q3.y; wz = q4.x;
      }
      const double xj = q0.x, yj = q0.y, zj = q1.x, vx = q1.y, vy = q2.x, vz = q2.y;
      const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
      if constexpr (!PERIODIC) {
        if constexpr (SKIP_SELF) {
          if (j0 + s == ti) continue;
        }
        pair_apply<KIND, WALL>(a.k, dx, dy, dz, zi, zj, vx, vy, vz, wx, wy, wz, acc);
      } else {
        periodic_images(a, dx, dy, dz, [&](double ex, double ey, double ez, bool central) {
          if constexpr (SKIP_SELF) {
            if (j0 + s == ti && central) return;
          }
          pair_apply<KIND, WALL>(a.k, ex, ey, ez, zi, zj, vx, vy, vz, wx, wy, wz, acc);
        });
      }
    }
    out[0] = acc.x; out[1] = acc.y; out[2] = acc.z;
  }

  // self term, prefactor and B_i, AoS store
  static __device__ __forceinline__ void store(const Args& a, long ti, const Target& tp, const double* s) {
    Vec3 acc = {s[0], s[1], s[2]};
    const double b = tp.w;
    double vx = a.vec[3 * ti] * b, vy = a.vec[3 * ti + 1] * b, vz = a.vec[3 * ti + 2] * b;
    double wx = 0, wy = 0, wz = 0;
    if constexpr (kind_has_torque(KIND)) { wx = a.vec2[3 * ti] * b; wy = a.vec2[3 * ti + 1] * b; wz = a.vec2[3 * ti + 2] * b; }
    if (a.in_plane) { vz = 0.0; wz = 0.0; }
    kind_self_term<KIND, WALL>(a.k, tp.z, vx, vy, vz, wx, wy, wz, acc);
    const double sc = a.prefactor * b;
    const long o = 3 * (ti - a.tgt_begin);
    a.out[o] = acc.x * sc; a.out[o + 1] = acc.y * sc; a.out[o + 2] = a.in_plane ? 0.0 : acc.z * sc;
  }
};

template <int KIND, bool WALL, bool PERIODIC>
__global__ __launch_bounds__(kBlock) void sweep_kernel(const SweepArgs a) { one_sided_sweep<SweepOp<KIND, WALL, PERIODIC>>(a); }

template <int KIND, bool WALL>
__global__ __launch_bounds__(256) void finalize_kernel(const SweepArgs a) { one_sided_finalize<SweepOp<KIND, WALL, false>>(a); }

// Positions: caller's (N,3) -> (x, y, z_eff, b).  Fuses shift_heights (mobility/mobility.py:52-64,
// clamp with `<=`) and damping_matrix_B (mobility/mobility.py:67-84, factor z/a for `z < a`), which
// the reference runs as an interpreted Python loop over N on every matvec.
__global__ void pack_positions_kernel(const double* r, long n, double a, int wall, double4* pos) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = r[3 * i], y = r[3 * i + 1], z = r[3 * i + 2];
  double4 p;
  p.x = x; p.y = y;
  if (wall) {
    p.z = (z <= a) ? a : z;
    p.w = (z < a) ? z / a : 1.0;
  } else {
    p.z = z; p.w = 1.0;
  }
  pos[i] = p;
}

// ---------------------------------------------------------------------------------------------
// Blob-blob soft repulsion, all pairs, minimal image (multi_bodies/forces_numba.py:12-55; the
// reference GPU twin multi_bodies/forces_pycuda.py:66-118 is float32, this one is fp64).
// ---------------------------------------------------------------------------------------------
struct ForceArgs : OneSidedArgs {
  const double4* pos;
  double Lx, Ly, Lz, iLx, iLy, iLz;
  double eps_over_b, inv_b, two_a;
  ExpConsts ec;
  const double* radii;   // per-blob radii (RADII variant: contact distance a_i + a_j, forces_numba.py:73-122) or nullptr
};

template <bool PERIODIC, bool RADII> struct ForceOp {
  typedef ForceArgs Args;
  struct Target { double4 p; double ra; };
  static constexpr int NOUT = 3, REC2 = 2;
  static constexpr bool SHARDED = true, SKIP_OWN_TILE = false;   // the pair i == j is tested by index in every pair

  static __device__ __forceinline__ Target load_target(const Args& a, long t) { return {a.pos[t], RADII ? a.radii[t] : 0.0}; }

  static __device__ __forceinline__ void stage(const Args& a, long j, double2* rec) {
    const double4 p = a.pos[j];
    rec[0] = make_double2(p.x, p.y);
    rec[1] = make_double2(p.z, RADII ? a.radii[j] : p.w);   // w is free here: forces use unclamped positions (b = 1)
  }

  template <bool>
  static __device__ __forceinline__ void tile_pairs(const Args& a, const double2* tile, int n, int wave, long j0, long ti,
                                                    const Target& tg, double* acc) {
    double fx = acc[0], fy = acc[1], fz = acc[2];
    for (int s = wave; s < n; s += kWaves) {
      const double2 q0 = tile[s * 2], q1 = tile[s * 2 + 1];
      double dx = q0.x - tg.p.x, dy = q0.y - tg.p.y, dz = q1.x - tg.p.z;
      if constexpr (PERIODIC) {
        if (a.Lx > 0) dx = wrap_nearest(dx, a.Lx, a.iLx);
        if (a.Ly > 0) dy = wrap_nearest(dy, a.Ly, a.iLy);
        if (a.Lz > 0) dz = wrap_nearest(dz, a.Lz, a.iLz);
      }
      const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
      const double ir = rsqrt_f64(r2);
      const double r = r2 * ir;
      // far: -(eps/b) exp(-(r-2a)/b)/r ; near (r <= 2a): -(eps/b)/max(r,1e-25) = -(eps/b) min(1/r, 1e25)
      const double two_a = RADII ? tg.ra + q1.y : a.two_a;
      // branch-free (sym_force_kernels.h pair_force): x = 0 exactly for r <= 2a, exp(0) = 1, min(1/r, 1e25) = 1/r beyond
      // (eps/b) min(1/r, 1e25) first, the exponential last: e is a denormal beyond (r - 2a)/b = 708 and e / r would be
      // rounded to the denormal grid BEFORE it is scaled up by eps/b (sym_force_kernels.h, BlobContactLaw)
      const double e = exp_nonpositive(a.ec, fmin((two_a - r) * a.inv_b, 0.0));
      double f0 = -((a.eps_over_b * fmin(ir, 1e25)) * e);
      if (j0 + s == ti) f0 = 0.0;  // i == j (r2 = 0 -> ir = inf; select, do not multiply)
      if (j0 + s == ti) { dx = 0.0; dy = 0.0; dz = 0.0; }
      fx = __builtin_fma(f0, dx, fx); fy = __builtin_fma(f0, dy, fy); fz = __builtin_fma(f0, dz, fz);
    }
    acc[0] = fx; acc[1] = fy; acc[2] = fz;
  }

  static __device__ __forceinline__ void store(const Args& a, long ti, const Target&, const double* acc) {
    const long o = 3 * (ti - a.tgt_begin);
    a.out[o] = acc[0]; a.out[o + 1] = acc[1]; a.out[o + 2] = acc[2];
  }
};

template <bool PERIODIC, bool RADII = false>
__global__ __launch_bounds__(kBlock) void force_sweep_kernel(const ForceArgs a) { one_sided_sweep<ForceOp<PERIODIC, RADII>>(a); }

__global__ __launch_bounds__(256) void force_finalize_kernel(const ForceArgs a) { one_sided_finalize<ForceOp<false, false>>(a); }

}  // namespace rmb
