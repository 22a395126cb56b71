// sym_kernels.h -- symmetric pair sweep for the translation-translation mobility (gfx950, fp64).
//
// The blob mobility is symmetric as a 3N x 3N matrix, M_ji = M_ij^T (for the wall part this is the
// Swan-Brady reciprocity the reference's C++ twin also relies on, mobility/mobility.cpp:407-424).
// sweep_kernel evaluates every ORDERED pair; here every UNORDERED pair is evaluated once and applied
// to both blobs:   u_i += M_ij v_j   and   u_j += M_ij^T v_i.
// The expensive part (two rsqrt, RPY coefficients, the five wall polynomials G1..G5) is shared; only the
// cheap contractions are done twice.  With W = f1 I + f2 e e^T + f3 e z^T + f4 z e^T + f5 z z^T,
//   W v   = f1 v + [f2 (e.v) + f3 v_z] e + [f4 (e.v) + f5 v_z] z
//   W^T v = f1 v + [f2 (e.v) + f4 v_z] e + [f3 (e.v) + f5 v_z] z          (f3 <-> f4)
// => 80 VALU instructions per unordered pair (76 fp64; pair_blocks.h: five-entry block + closed-form wall
// polynomials through H) instead of 2 x 67 in the bulk loop of the one-sided sweep.
//
// Work decomposition: blobs are cut into tiles of 64; a work unit is a tile pair (I <= J).  One wave64
// owns a unit: lane l holds blob i = 64 I + l in registers (position, its own vector v_i, accumulator u_i);
// tile J sits in the wave's private LDS slab.  At step k lane l meets blob j = 64 J + ((l + k) & 63): the
// "rotation" makes every lane touch a different j, so the transposed contribution is added to the
// per-wave LDS accumulator of j without conflicts (ds_add_f64) and source records are plain per-lane
// ds_read_b128 (48-byte records: conflict-free).  Diagonal units (I == J) run forward-only over
// k = 1..63 (every ordered pair exactly once).  After 64 steps u_i (registers) and u_J (LDS) are flushed
// to global SoA accumulators with global_atomic_add_f64; finalize adds the self term and scales.
// Schedule: static and exactly balanced -- the n_units x 64 rotation steps are cut into equal contiguous
// ranges, one per wave (a range may start/end inside a unit; >= 64 steps each; 8x more workgroups than are
// resident at once), so every SIMD gets the same number of steps and no work counter is needed (a single dequeue word saturates at ~88 dequeues/us, which is
// about the unit rate of this kernel at N = 1e4).  Consecutive units share the row tile I, whose
// accumulator stays in registers until the row changes.  The order in which the atomics land is not
// fixed: results agree with the deterministic sweep_kernel to rounding (~1e-15 relative) but are not
// bit-reproducible; the "deterministic" context option selects sweep_kernel instead.
#pragma once
#include "pair_blocks.h"
#include "sym_schedule.h"
#include "sym_walk.h"

namespace rmb {

struct SymArgs {
  const double4* pos;   // [n] packed positions
  const double* vec;    // [3n] source vector (AoS)
  double* acc;          // [3][n_pad] global SoA accumulators; zero on entry, re-zeroed by finalize
  double* out;          // [3n] final output (AoS)
  long n;
  long n_pad;           // 64 * n_tiles
  int n_tiles;
  long n_units;         // n_tiles (n_tiles + 1) / 2
  int order;            // unit order: 0 row-major, 1 blocked (unit_seek / unit_next); xcd != 0: XCD-aware workgroup numbering
  int xcd;
  long step_begin, step_end;  // rotation steps [begin, end) of the n_units*64 this launch covers (pair shard)
  long steps_per_wave;        // ceil((step_end - step_begin) / waves): wave w takes [begin + w spw, +spw)
  long self_begin, self_end;  // targets whose self term this launch adds (exactly one shard per target)
  double Lx, Ly, Lz, iLx, iLy, iLz;  // pseudo-periodic lengths (<= 0: open) and reciprocals
  double prefactor;
  int accumulate;         // finalize adds to `out` instead of overwriting it (second pass of the fused tt+tr product)
  int skip_pairs;         // diagnostics: run the schedule / loads / flushes but no pair arithmetic (timing only)
  long long* wave_clock;  // optional [n_waves][2] wall-clock stamps (start, end | placement bits) for schedule diagnostics, or nullptr
  PairConsts k;
};

constexpr int kSymRecBytes = 48;

// Both directions of one pair.  (vix..) = target's own vector, (vjx..) = source vector.
// Adds M_ij v_j to ui and returns M_ij^T v_i in (tx,ty,tz).  The block is built once in the form of pair_blocks.h
// (BlockM: F, P, Q3, Q4, Szz) and contracted with ten instructions per direction.
// ACC: the transposed rows are ADDED to (tx, ty, tz) instead of written -- the second target blob of sym2t_kernel folds its
// contribution into the first one's with the fused multiply-adds that build it (three v_add_f64 less per rotation step).
template <bool WALL, bool ACC = false, bool ZI2 = false>
__device__ __forceinline__ void pair_tt_sym(const PairConsts& k, double dx, double dy, double dz, double zi, double zj,
                                            double vix, double viy, double viz, double vjx, double vjy, double vjz,
                                            Vec3& ui, double& tx, double& ty, double& tz) {
  const Geom g = make_geom<WALL, ZI2>(dx, dy, dz, zi, zj);
  const TTc c = tt_coeffs<WALL, ZI2>(k, g, zi, zj);
  const double vi[3] = {vix, viy, viz}, vj[3] = {vjx, vjy, vjz};
  double u[3] = {ui.x, ui.y, ui.z}, t[3];
  if constexpr (ACC) { t[0] = tx; t[1] = ty; t[2] = tz; }
  tt_apply<WALL, ACC>(c, g, vi, vj, u, t);
  ui.x = u[0]; ui.y = u[1]; ui.z = u[2];
  tx = t[0]; ty = t[1]; tz = t[2];
}

// rr, both directions (same block form, pair_blocks.h: rr_coeffs).
template <bool WALL, bool ACC = false>
__device__ __forceinline__ void pair_rr_sym(const PairConsts& k, double dx, double dy, double dz, double zi, double zj,
                                            double vix, double viy, double viz, double vjx, double vjy, double vjz,
                                            Vec3& ui, double& tx, double& ty, double& tz) {
  const Geom g = make_geom<WALL>(dx, dy, dz, zi, zj);
  const RRc c = rr_coeffs<WALL>(k, g);
  const double vi[3] = {vix, viy, viz}, vj[3] = {vjx, vjy, vjz};
  double u[3] = {ui.x, ui.y, ui.z}, t[3];
  if constexpr (ACC) { t[0] = tx; t[1] = ty; t[2] = tz; }
  rr_apply<WALL, ACC>(c, g, vi, vj, u, t);
  ui.x = u[0]; ui.y = u[1]; ui.z = u[2];
  tx = t[0]; ty = t[1]; tz = t[2];
}

// Coupling blocks, both directions.  KIND_TR: u = M_tr tau, wall part anchored on the TARGET height of each
// direction (z_i forward, z_j transposed); KIND_RT: w = M_rt f, anchored on the SOURCE height (z_j forward,
// z_i transposed).  The two directions share both rsqrt, tau, e and differ only in g = z iR, which enters
// p, s, f3 linearly (pair_blocks.h: cpl_coeffs / tr_apply / rt_apply on the unnormalised separation).
template <bool TR, bool WALL, bool ACC = false>
__device__ __forceinline__ void pair_coupling_sym(const PairConsts& k, double dx, double dy, double dz, double zi, double zj,
                                                  double vix, double viy, double viz, double vjx, double vjy, double vjz,
                                                  Vec3& ui, double& tx, double& ty, double& tz) {
  const Geom g = make_geom<WALL>(dx, dy, dz, zi, zj);
  const CPc C = cpl_coeffs<WALL>(k, g, zi, zj);
  const double vi[3] = {vix, viy, viz}, vj[3] = {vjx, vjy, vjz};
  double u[3] = {ui.x, ui.y, ui.z}, t[3];
  if constexpr (ACC) { t[0] = tx; t[1] = ty; t[2] = tz; }
  if constexpr (TR) tr_apply<WALL, ACC>(C, g, vi, vj, u, t);
  else              rt_apply<WALL, ACC>(C, g, vi, vj, u, t);
  ui.x = u[0]; ui.y = u[1]; ui.z = u[2];
  tx = t[0]; ty = t[1]; tz = t[2];
}

// Doubled-height operands.  The wall tt block needs 2 z_i (Q3, pair_blocks.h: tt_block); at the 128-register cap the compiler
// rebuilt it for every pair.  The wall-tt instances of sym_kernel, sym_coop_kernel and sym2t_kernel therefore keep h = 2 z_i in the
// lane where the other kinds keep z_i (padding sentinel 2.0 for 1.0) and hand it on as `zi` with ZI2 set:
//   d_z = fma(h, 0.5, -z_j),  R_z = fma(h, 0.5, z_j),  the -2 z_i of Q3 = -h (a source modifier).
// 2 z and 0.5 (2 z) are exact and each fma rounds once, so every pair block is bit for bit what z_i gives.  tr / rt anchor on
// z_i itself and rr does not need 2 z_i: they keep z_i.
template <int KIND, bool WALL> constexpr bool kSymZi2 = KIND == KIND_TT && WALL;
template <bool ZI2> __device__ __forceinline__ double sym_height(double z) { return ZI2 ? z + z : z; }           // what the lane keeps
template <bool ZI2> __device__ __forceinline__ double sym_dz(double zi, double zj) { return ZI2 ? __builtin_fma(zi, 0.5, -zj) : zi - zj; }

// dispatcher
template <int KIND, bool WALL, bool ACC = false, bool ZI2 = false>
__device__ __forceinline__ void pair_sym(const PairConsts& k, double dx, double dy, double dz, double zi, double zj,
                                         double vix, double viy, double viz, double vjx, double vjy, double vjz,
                                         Vec3& ui, double& tx, double& ty, double& tz) {
  static_assert(!ZI2 || (KIND == KIND_TT && WALL), "doubled heights: wall tt only");
  if constexpr (KIND == KIND_TT) pair_tt_sym<WALL, ACC, ZI2>(k, dx, dy, dz, zi, zj, vix, viy, viz, vjx, vjy, vjz, ui, tx, ty, tz);
  if constexpr (KIND == KIND_RR) pair_rr_sym<WALL, ACC>(k, dx, dy, dz, zi, zj, vix, viy, viz, vjx, vjy, vjz, ui, tx, ty, tz);
  if constexpr (KIND == KIND_TR) pair_coupling_sym<true, WALL, ACC>(k, dx, dy, dz, zi, zj, vix, viy, viz, vjx, vjy, vjz, ui, tx, ty, tz);
  if constexpr (KIND == KIND_RT) pair_coupling_sym<false, WALL, ACC>(k, dx, dy, dz, zi, zj, vix, viy, viz, vjx, vjy, vjz, ui, tx, ty, tz);
}


template <int KIND, bool WALL, bool PERIODIC>
__global__ __launch_bounds__(64 * kSymWaves) __attribute__((amdgpu_waves_per_eu(kSymWavesPerEu, kSymWavesPerEu))) void sym_kernel(const SymArgs a) {
  __shared__ double2 rec_all[kSymWaves][64 * 3];
  __shared__ double accj_all[kSymWaves][3 * 64];
  static constexpr bool Z2 = kSymZi2<KIND, WALL>;      // wall tt: zi holds the doubled height 2 z_i (see pair_sym)

  struct Body {
    const SymArgs& a;
    const int lane;
    double2* const rec;
    double* const accj;
    long i;
    bool vi_ok;
    double xi, yi, zi, vix, viy, viz;
    Vec3 ui;

    __device__ __forceinline__ Body(const SymArgs& a, int lane, double2* rec, double* accj) : a(a), lane(lane), rec(rec), accj(accj) {}
    __device__ __forceinline__ void begin() {
      i = 0;
      vi_ok = false;
      xi = 0; yi = 0; zi = sym_height<Z2>(1.0); vix = 0; viy = 0; viz = 0;
      ui.x = 0.0; ui.y = 0.0; ui.z = 0.0;
    }
    __device__ __forceinline__ bool culled(int, int) const { return false; }
    __device__ __forceinline__ void flush_row(long) {
      if (!vi_ok) return;
      __hip_atomic_fetch_add(&a.acc[i], ui.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&a.acc[a.n_pad + i], ui.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&a.acc[2 * a.n_pad + i], ui.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void load_row(int I) {
      i = 64L * I + lane;
      vi_ok = i < a.n;
      xi = 1e100; yi = 1e100; zi = sym_height<Z2>(1.0); vix = 0; viy = 0; viz = 0;
      if (vi_ok) {
        const double4 p = a.pos[i];
        xi = p.x; yi = p.y; zi = sym_height<Z2>(p.z);
        vix = a.vec[3 * i] * p.w; viy = a.vec[3 * i + 1] * p.w; viz = a.vec[3 * i + 2] * p.w;
      }
      ui.x = 0.0; ui.y = 0.0; ui.z = 0.0;
    }
    __device__ __forceinline__ void unit(int I, int J, int k0, int k1, long) {
      const char* rec_bytes = reinterpret_cast<const char*>(rec);
      // tile J -> this wave's LDS slab (record l = blob 64 J + l), zero its accumulators
      {
        const long j = 64L * J + lane;
        double xj = -1e100, yj = -1e100, zj = 1.0, vjx = 0, vjy = 0, vjz = 0;
        if (j < a.n) {
          const double4 p = a.pos[j];
          xj = p.x; yj = p.y; zj = p.z;
          vjx = a.vec[3 * j] * p.w; vjy = a.vec[3 * j + 1] * p.w; vjz = a.vec[3 * j + 2] * p.w;
        }
        rec[lane * 3 + 0] = make_double2(xj, yj);
        rec[lane * 3 + 1] = make_double2(zj, vjx);
        rec[lane * 3 + 2] = make_double2(vjy, vjz);
        accj[lane] = 0.0; accj[64 + lane] = 0.0; accj[128 + lane] = 0.0;
      }
      wave_lds_sync();

      // Pseudo-periodic images (mobility_numba.py:170-197): nearest image once, then the 3^d neighbour boxes.
      // M_ji(box b) = M_ij(box -b)^T and the boxes are summed symmetrically, so both directions of every image
      // are still evaluated together.
      const int px = PERIODIC && a.Lx > 0, py = PERIODIC && a.Ly > 0, pz = PERIODIC && a.Lz > 0;
      if (I != J) {
        for (int k = (a.skip_pairs & 1) ? k1 : k0; k < k1; ++k) {
          const int jj = (lane + k) & 63;
          const double2* r = reinterpret_cast<const double2*>(rec_bytes + jj * kSymRecBytes);
          const double2 q0 = r[0], q1 = r[1], q2 = r[2];
          double dx = xi - q0.x, dy = yi - q0.y, dz = sym_dz<Z2>(zi, q1.x);
          double tx, ty, tz;
          if constexpr (!PERIODIC) {
            pair_sym<KIND, WALL, false, Z2>(a.k, dx, dy, dz, zi, q1.x, vix, viy, viz, q1.y, q2.x, q2.y, ui, tx, ty, tz);
          } else {
            if (px) dx = wrap_nearest_pad_safe(dx, a.Lx, a.iLx);
            if (py) dy = wrap_nearest_pad_safe(dy, a.Ly, a.iLy);
            if (pz) dz = wrap_nearest_pad_safe(dz, a.Lz, a.iLz);
            tx = 0.0; ty = 0.0; tz = 0.0;
            for (int bx = -px; bx <= px; ++bx)
              for (int by = -py; by <= py; ++by)
                for (int bz = -pz; bz <= pz; ++bz) {
                  pair_sym<KIND, WALL, true, Z2>(a.k, dx + bx * a.Lx, dy + by * a.Ly, dz + bz * a.Lz, zi, q1.x, vix, viy, viz, q1.y, q2.x,
                                             q2.y, ui, tx, ty, tz);      // accumulates (fused multiply-adds)
                }
          }
          __hip_atomic_fetch_add(&accj[jj], tx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          __hip_atomic_fetch_add(&accj[64 + jj], ty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          __hip_atomic_fetch_add(&accj[128 + jj], tz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        wave_lds_sync();
        const long j = 64L * J + lane;
        if (j < a.n && !(a.skip_pairs & 2)) {
          __hip_atomic_fetch_add(&a.acc[j], accj[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(&a.acc[a.n_pad + j], accj[64 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(&a.acc[2 * a.n_pad + j], accj[128 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      } else {
        // diagonal unit: every ordered pair of the tile once, forward only.  Step 0 is the blob itself: its
        // central-box term is the self term (finalize); its periodic images use the pair formula.
        for (int k = (a.skip_pairs & 1) ? k1 : ((PERIODIC || k0 > 1) ? k0 : 1); k < k1; ++k) {
          const int jj = (lane + k) & 63;
          const double2* r = reinterpret_cast<const double2*>(rec_bytes + jj * kSymRecBytes);
          const double2 q0 = r[0], q1 = r[1], q2 = r[2];
          double dx = xi - q0.x, dy = yi - q0.y, dz = sym_dz<Z2>(zi, q1.x);
          if constexpr (!PERIODIC) {
            pair_apply<KIND, WALL, Z2>(a.k, dx, dy, dz, zi, q1.x, q1.y, q2.x, q2.y, 0.0, 0.0, 0.0, ui);
          } else {
            if (px) dx = wrap_nearest_pad_safe(dx, a.Lx, a.iLx);
            if (py) dy = wrap_nearest_pad_safe(dy, a.Ly, a.iLy);
            if (pz) dz = wrap_nearest_pad_safe(dz, a.Lz, a.iLz);
            for (int bx = -px; bx <= px; ++bx)
              for (int by = -py; by <= py; ++by)
                for (int bz = -pz; bz <= pz; ++bz) {
                  if (k == 0 && bx == 0 && by == 0 && bz == 0) continue;
                  pair_apply<KIND, WALL, Z2>(a.k, dx + bx * a.Lx, dy + by * a.Ly, dz + bz * a.Lz, zi, q1.x, q1.y, q2.x, q2.y, 0.0, 0.0,
                                         0.0, ui);
                }
          }
        }
      }
      __builtin_amdgcn_wave_barrier();   // accj / rec are rewritten by the next unit
    }
  };

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  Body body(a, threadIdx.x & 63, rec_all[wave], accj_all[wave]);
  // Static, exactly balanced schedule: the n_units * 64 rotation steps are cut into equal contiguous ranges, one per
  // chunk of a wave; a range may begin and end inside a unit (sym_walk.h).
  const long w = sym_wave(a.xcd);
  const long long t_start = a.wave_clock ? wall_clock64() : 0;
  sym_walk(SymWalk{a.order, a.n_tiles, a.step_begin, a.step_end, a.steps_per_wave, sym_n_waves(), w}, body);
  if (a.wave_clock && body.lane == 0) {   // stamps go to a buffer nothing else reads
    // placement: HW_ID (reg 4: simd [5:4], cu [11:8], sh [12], se [15:13]) and XCC_ID (reg 20) in the top 24 bits
    const unsigned hw = __builtin_amdgcn_s_getreg((4) | (0 << 6) | ((16 - 1) << 11));
    const unsigned xcc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | ((4 - 1) << 11));
    a.wave_clock[2 * w] = t_start;
    a.wave_clock[2 * w + 1] = (wall_clock64() & 0xffffffffffLL) | ((long long)(hw & 0xffff) << 40) | ((long long)(xcc & 0xf) << 56);
  }
}

// AoS result of a workgroup's 256 blobs through LDS, so that every store instruction writes 2 KB of CONSECUTIVE addresses
// (thread t writes doubles t, t + 256, t + 512 of the workgroup's 768) instead of 8 bytes at a stride of 24: the same
// bytes with a third of the write transactions, and the only way the result can go straight into page-locked host memory
// at a useful rate (rmb_matvec's zero-copy hand-off: partial-line writes over PCIe are 2x slower than a copy from ~4000
// blobs on, profiles/r4_exp_host_staging_rejected.txt).  `tile` = 768 doubles of LDS; base = first blob of the workgroup.
__device__ __forceinline__ void store_aos_coalesced(double* tile, double* out, long base, long n, double x, double y, double z,
                                                    bool valid, bool accumulate) {
  const int t = threadIdx.x;
  if (valid) { tile[3 * t] = x; tile[3 * t + 1] = y; tile[3 * t + 2] = z; }
  __syncthreads();
  const long lim = 3 * n;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long g = 3 * base + c * 256 + t;
    if (g < lim) out[g] = accumulate ? out[g] + tile[c * 256 + t] : tile[c * 256 + t];
  }
  __syncthreads();          // the tile is reused by the caller's next output
}

template <int KIND, bool WALL>
__global__ __launch_bounds__(256) void sym_finalize_kernel(const SymArgs a) {
  __shared__ double tile[768];
  const long base = (long)blockIdx.x * blockDim.x;
  const long i = base + threadIdx.x;
  const bool valid = i < a.n;
  Vec3 acc = {0.0, 0.0, 0.0};
  double sc = 0.0;
  if (valid) {
    acc.x = a.acc[i]; acc.y = a.acc[a.n_pad + i]; acc.z = a.acc[2 * a.n_pad + i];
    a.acc[i] = 0.0; a.acc[a.n_pad + i] = 0.0; a.acc[2 * a.n_pad + i] = 0.0;   // ready for the next product
    const double4 p = a.pos[i];
    const double b = p.w;
    if (i >= a.self_begin && i < a.self_end)
      self_term<KIND, WALL>(a.k, p.z, a.vec[3 * i] * b, a.vec[3 * i + 1] * b, a.vec[3 * i + 2] * b, 0, 0, 0, acc);
    sc = a.prefactor * b;
  }
  store_aos_coalesced(tile, a.out, base, a.n, acc.x * sc, acc.y * sc, acc.z * sc, valid, a.accumulate != 0);
}


}  // namespace rmb
