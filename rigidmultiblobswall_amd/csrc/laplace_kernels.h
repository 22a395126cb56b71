// laplace_kernels.h -- Laplace layer operators of phoretic (chemically active) bodies (gfx950, fp64).
//
// WHAT: the six O(N_s N_t) operators of Laplace_kernels/Laplace_kernels_numba.py, every one 1/(4 pi) sum_s w_s f_s K(r),
// r = x_t - x_s, with the image of a no-slip wall at z = 0 added for wall = 1 (image source (x, y, -z), image normal
// (n_x, n_y, -n_z); the image term is kept for the pair t == s):
//   single layer   S[f]   K = 1/|r|                                                          :12
//   double layer   D[f]   K = (r.n_s)/|r|^3                                                  :68
//   gradient of D  G[f]   K = (I - 3 r r^T/|r|^2) n_s/|r|^3   (3-vector)                     :138
//   dipole         P[f]   K = r/|r|^3                         (3-vector)                     :254
//   S and D source -> target                                                                 :329, :398
// The self operators (sources = targets) skip the free-space term of the pair t == s BY INDEX; the source -> target
// ones skip it when |r| < 1e-12.  Two FUSED sweeps carry the concentration solve of the phoretic slip:
//   operator   out_t = alpha c_t - D[p]_t + S[q]_t      (one pass: both terms share r, 1/r and the image distance)
//   gradient   out_t = 2 G[p]_t - 2 P[q]_t
// The reference-shaped single operators are the same template with one term compiled out (no pass over a zero field).
//
// HOW: policies of the one-sided frame (onesided_kernels.h).  A record holds the position, the normal and the two weighted
// fields w p, w q with their signs / factors folded in at staging, so the pair loop is a handful of FMAs around one inverse
// square root per distance (two with the wall).  The index test of the self operators runs only in the source tile that
// overlaps the workgroup's own 64 targets.
//
// VALU instructions per source-target pair of the pair loop in this build (tools/kernel_resources.py; free / with the
// wall images; of them fp64: one to three fewer):
//   self:            S 15 / 24   D 20 / 33   operator 20 / 33   G 28 / 49   P 19 / 33   gradient 29 / 51
//   source -> target: S 18 / 27   D 23 / 36   (the distance test is in every pair)
// The fused sweeps cost what their more expensive half costs: the operator one pass of D, the gradient one pass of G
// plus one FMA.
#pragma once
#include "onesided_kernels.h"

namespace rmb {

enum { LAP_S = 0, LAP_D = 1, LAP_OPERATOR = 2, LAP_GRAD_D = 3, LAP_DIPOLE = 4, LAP_GRADIENT = 5 };

struct LapArgs : OneSidedArgs {   // out: [nt] (S, D, operator) or [3 nt] (G, P, gradient)
  const double* src;    // [3 ns]
  const double* tgt;    // [3 nt]  (== src for the self operators)
  const double* nrm;    // normals at the sources [3 ns]   (D, G)
  const double* w;      // quadrature weights [ns]
  const double* p;      // field of the D / G term [ns]
  const double* q;      // field of the S / P term [ns]
  const double* c;      // operator: alpha c_t [nt], or nullptr
  double sp, sq;        // folded into the records: w p sp, w q sq
  double alpha;
  double prefactor;     // 1/(4 pi)
};

template <int OP> struct LapShape {
  static constexpr bool S = OP == LAP_S || OP == LAP_OPERATOR;        // scalar 1/r term on q
  static constexpr bool D = OP == LAP_D || OP == LAP_OPERATOR;        // scalar double layer on p
  static constexpr bool G = OP == LAP_GRAD_D || OP == LAP_GRADIENT;   // vector gradient of D on p
  static constexpr bool P = OP == LAP_DIPOLE || OP == LAP_GRADIENT;   // vector dipole on q
  static constexpr bool NORMALS = D || G;
  static constexpr int NOUT = (G || P) ? 3 : 1;
  static constexpr int REC2 = NORMALS ? 4 : 2;     // double2 per record: (x, y) (z, n_x) (n_y, n_z) (wp, wq) | (x, y) (z, wq)
};

// One source at (dx, dy, dz) = x_t - x_s, Rz = z_t + z_s.  SKIP: 0 = none, 1 = `skip` (index test), 2 = |r| < 1e-12.
template <int OP, bool WALL, int SKIP>
__device__ __forceinline__ void lap_pair(double dx, double dy, double dz, double Rz, double nx, double ny, double nz,
                                         double wp, double wq, bool skip, double* acc) {
  using Sh = LapShape<OP>;
  const double rho2 = __builtin_fma(dy, dy, dx * dx);
  const double r2 = __builtin_fma(dz, dz, rho2);
  double ir = rsqrt_f64(r2);
  if constexpr (SKIP == 1) ir = skip ? 0.0 : ir;
  if constexpr (SKIP == 2) ir = (r2 < 1e-24) ? 0.0 : ir;
  const double ir2 = ir * ir;
  if constexpr (Sh::NOUT == 1) {
    double k = 0.0;
    if constexpr (Sh::D) k = ir2 * __builtin_fma(dz, nz, __builtin_fma(dy, ny, dx * nx)) * wp;   // (r.n) w p / r^2
    if constexpr (Sh::S) k += wq;
    acc[0] = __builtin_fma(ir, k, acc[0]);
    if constexpr (WALL) {
      const double iR = rsqrt_f64(__builtin_fma(Rz, Rz, rho2));
      double kI = 0.0;
      if constexpr (Sh::D) kI = (iR * iR) * __builtin_fma(-Rz, nz, __builtin_fma(dy, ny, dx * nx)) * wp;
      if constexpr (Sh::S) kI += wq;
      acc[0] = __builtin_fma(iR, kI, acc[0]);
    }
  } else {
    // G: (n - 3 r (r.n)/r^2) w p / r^3;  P: r w q / r^3  ->  acc += cd r + cn n
    const double ir3 = ir2 * ir;
    double cd = 0.0, cn = 0.0;
    if constexpr (Sh::G) {
      const double rn = __builtin_fma(dz, nz, __builtin_fma(dy, ny, dx * nx));
      cn = ir3 * wp;
      cd = -3.0 * ir2 * rn * cn;
    }
    if constexpr (Sh::P) cd = __builtin_fma(ir3, wq, cd);
    acc[0] = __builtin_fma(cd, dx, acc[0]); acc[1] = __builtin_fma(cd, dy, acc[1]); acc[2] = __builtin_fma(cd, dz, acc[2]);
    if constexpr (Sh::G) {
      acc[0] = __builtin_fma(cn, nx, acc[0]); acc[1] = __builtin_fma(cn, ny, acc[1]); acc[2] = __builtin_fma(cn, nz, acc[2]);
    }
    if constexpr (WALL) {
      // image: R = (dx, dy, Rz), normal (n_x, n_y, -n_z)
      const double iR = rsqrt_f64(__builtin_fma(Rz, Rz, rho2));
      const double iR2 = iR * iR, iR3 = iR2 * iR;
      double cdI = 0.0, cnI = 0.0;
      if constexpr (Sh::G) {
        const double rnI = __builtin_fma(-Rz, nz, __builtin_fma(dy, ny, dx * nx));
        cnI = iR3 * wp;
        cdI = -3.0 * iR2 * rnI * cnI;
      }
      if constexpr (Sh::P) cdI = __builtin_fma(iR3, wq, cdI);
      acc[0] = __builtin_fma(cdI, dx, acc[0]); acc[1] = __builtin_fma(cdI, dy, acc[1]); acc[2] = __builtin_fma(cdI, Rz, acc[2]);
      if constexpr (Sh::G) {
        acc[0] = __builtin_fma(cnI, nx, acc[0]); acc[1] = __builtin_fma(cnI, ny, acc[1]); acc[2] = __builtin_fma(-cnI, nz, acc[2]);
      }
    }
  }
}

// The pairs of one LDS tile for this wave's sources (every kWaves-th); so = the tile slot of the lane's own target (SKIP 1).
template <int OP, bool WALL, int SKIP>
__device__ __forceinline__ void lap_tile(const double2* tile, int n, int wave, double xt, double yt, double zt, int so,
                                         double* acc) {
  constexpr int R2 = LapShape<OP>::REC2;
  for (int s = wave; s < n; s += kWaves) {
    const double2* rec = tile + s * R2;
    const double2 p0 = rec[0], p1 = rec[1];
    double nx = 0.0, ny = 0.0, nz = 0.0, wp = 0.0, wq;
    if constexpr (R2 == 4) {
      const double2 p2 = rec[2], p3 = rec[3];
      nx = p1.y; ny = p2.x; nz = p2.y; wp = p3.x; wq = p3.y;
    } else {
      wq = p1.y;
    }
    lap_pair<OP, WALL, SKIP>(xt - p0.x, yt - p0.y, zt - p1.x, zt + p1.x, nx, ny, nz, wp, wq, s == so, acc);
  }
}

template <int OP, bool WALL, bool SELF> struct LapOp {
  typedef LapArgs Args;
  using Sh = LapShape<OP>;
  struct Target { double x, y, z; };
  static constexpr int NOUT = Sh::NOUT, REC2 = Sh::REC2;
  static constexpr bool SHARDED = false, SKIP_OWN_TILE = SELF;   // source -> target: by distance, in every pair

  static __device__ __forceinline__ Target load_target(const Args& a, long t) { return {a.tgt[3 * t], a.tgt[3 * t + 1], a.tgt[3 * t + 2]}; }

  static __device__ __forceinline__ void stage(const Args& a, long j, double2* rec) {
    const double w = a.w[j];
    rec[0] = make_double2(a.src[3 * j], a.src[3 * j + 1]);
    if constexpr (REC2 == 4) {
      rec[1] = make_double2(a.src[3 * j + 2], a.nrm[3 * j]);
      rec[2] = make_double2(a.nrm[3 * j + 1], a.nrm[3 * j + 2]);
      rec[3] = make_double2(a.sp * (w * a.p[j]), (Sh::S || Sh::P) ? a.sq * (w * a.q[j]) : 0.0);
    } else {
      rec[1] = make_double2(a.src[3 * j + 2], a.sq * (w * a.q[j]));
    }
  }

  template <bool OWN>
  static __device__ __forceinline__ void tile_pairs(const Args&, const double2* tile, int n, int wave, long j0, long ti,
                                                    const Target& tg, double* acc) {
    if constexpr (OWN) {
      const int so = (ti >= j0 && ti < j0 + n) ? (int)(ti - j0) : -1;   // the tile slot of the lane's own target
      lap_tile<OP, WALL, 1>(tile, n, wave, tg.x, tg.y, tg.z, so, acc);
    } else {
      lap_tile<OP, WALL, SELF ? 0 : 2>(tile, n, wave, tg.x, tg.y, tg.z, -1, acc);
    }
  }

  static __device__ __forceinline__ void store(const Args& a, long t, const Target&, const double* acc) {
    if constexpr (NOUT == 1) {
      a.out[t] = a.c ? __builtin_fma(a.alpha, a.c[t], acc[0] * a.prefactor) : acc[0] * a.prefactor;
    } else {
#pragma unroll
      for (int c = 0; c < NOUT; ++c) a.out[NOUT * t + c] = acc[c] * a.prefactor;
    }
  }
};

template <int OP, bool WALL, bool SELF>
__global__ __launch_bounds__(kBlock) void laplace_sweep_kernel(const LapArgs a) { one_sided_sweep<LapOp<OP, WALL, SELF>>(a); }

// the epilogue depends on the operator through NOUT alone
template <int NOUT>
__global__ __launch_bounds__(256) void laplace_finalize_kernel(const LapArgs a) { one_sided_finalize<LapOp<NOUT == 1 ? LAP_S : LAP_DIPOLE, false, false>>(a); }

}  // namespace rmb
