// potential_kernels.h -- total potential energy of a blob configuration (gfx950, fp64): the equilibrium sampler's hot path.
//
// U = sum_i u1(z_i) + sum_{i<j} u2(r_ij), the reference's many_bodyMCMC/many_body_potential_pycuda.py:64-119 (one thread
// per blob, inner loop j > i over global memory).  Here every unordered pair is met once on the schedule of
// sym_force_kernel (sym_force_kernels.h): a work unit is a tile pair I <= J, lane = blob of tile I, tile J staged in the wave's
// LDS slab and read by rotation; the same unit_seek / unit_next, xcd_swizzle (sym_schedule.h), strided chunks, tile bounds and exact-zero
// culling.  The result is a scalar, so there is nothing to transpose: every lane keeps two fp64 sums (one-blob, pair) for
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
#pragma once
#include "pair_ops.h"
#include "sym_schedule.h"

namespace rmb {

enum PotentialForm : int { POT_SOFT = 0, POT_YUKAWA = 1 };

struct PotentialArgs {
  const double4* pos;   // packed raw positions (caller's order, or the sorted copy)
  const unsigned* perm; // sorted slot -> caller's index, or nullptr
  const double* bounds; // [n_tiles][6] tile bounding boxes of `pos` (always present)
  double cull2;         // squared reach of the pair term; +inf = no culling
  long n;
  int n_tiles;
  int order, xcd;
  long chunk_steps;     // > 0: steps per strided chunk of a wave; 0: one contiguous range per wave
  long step_end;        // n_units * 64
  double Lx, Ly, iLx, iLy;
  double eps, inv_b, two_a;              // pair term
  double eps_wall, inv_b_wall, a, weight;  // one-blob term
  ExpConsts ec;
  double* partial;      // [n_waves][2] = (one-blob, pair) sums of every wave of the launch
  long n_partial;       // n_waves
  double* out;          // {U_one_blob, U_pair}; BODY: {U_body}
  // BODY only (kept behind the fields every instance reads, whose offsets the blob forms' register allocation depends on)
  double Lz, iLz;       // the blob forms ignore periodic_length[2]
  int n_out;            // 2, BODY: 1
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

// minimal image of one separation component (L <= 0: open direction)
template <bool PERIODIC>
__device__ __forceinline__ double image(double L, double iL, double d) {
  if constexpr (PERIODIC) {
    if (L > 0) d = wrap_nearest_pad_safe(d, L, iL);
  }
  return d;
}

// separation in z: the blob forms take it as it is, the body centres take its minimal image
template <bool PERIODIC, bool BODY>
__device__ __forceinline__ double image_z(const PotentialArgs& a, double d) {
  if constexpr (BODY) return image<PERIODIC>(a.Lz, a.iLz, d);
  return d;
}

template <int FORM, bool PERIODIC, bool BODY = false>
__global__ __launch_bounds__(64 * kSymWaves) void potential_kernel(const PotentialArgs a) {
  static_assert(!BODY || FORM == POT_YUKAWA, "the body-body law is the yukawa pair expression");
  __shared__ double4 rec_all[kSymWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double4* rec = rec_all[wave];
  const long n_waves = (long)gridDim.x * kSymWaves;
  const long w = (a.xcd ? xcd_swizzle(blockIdx.x, gridDim.x) : (long)blockIdx.x) * kSymWaves + wave;
  const long spw = a.chunk_steps > 0 ? a.chunk_steps : (a.step_end + n_waves - 1) / n_waves;
  double u_one = 0.0, u_pair = 0.0;
  for (long chunk = w;; chunk += n_waves) {
    long s = chunk * spw;
    if (s >= a.step_end) break;
    long s_end = s + spw;
    if (s_end > a.step_end) s_end = a.step_end;
    int I = 0, J = 0;
    unit_seek(a.order, s >> 6, a.n_tiles, I, J);
    int I_cur = -1;
    double xi = 0, yi = 0, zi = 0, idx_i = 0;
    bool vi_ok = false;
    while (s < s_end) {
      const int k0 = (int)(s & 63);
      const long left = s_end - s;
      const int k1 = (left < 64 - k0) ? (int)(k0 + left) : 64;
      s += k1 - k0;
      const bool diag = (I == J);
      // diagonal unit: step 0 = the one-blob terms, steps 1..32 = every unordered pair of the tile once
      // (lane l meets l + k; at k = 32 both lanes of a pair would meet: the lower half takes it), 33..63 empty
      const bool idle = diag ? (k0 > 32) : (tile_gap2(a.bounds, I, J, PERIODIC ? a.Lx : 0.0, PERIODIC ? a.Ly : 0.0, PERIODIC && BODY ? a.Lz : 0.0) > a.cull2);
      if (idle) {   // beyond the reach of the exponential: every term of the unit is exactly zero
        if (k1 == 64) unit_next(a.order, a.n_tiles, I, J);
        continue;
      }
      if (I != I_cur) {
        I_cur = I;
        const long i = 64L * I + lane;
        vi_ok = i < a.n;
        xi = 1e100; yi = 1e100; zi = 1e100; idx_i = 1e18;
        if (vi_ok) {
          const double4 p = a.pos[i];
          xi = p.x; yi = p.y; zi = p.z;
          idx_i = (double)(a.perm ? (long)a.perm[i] : i);
        }
      }
      if (!diag) {
        const long j = 64L * J + lane;
        double4 p = make_double4(-1e100, -1e100, -1e100, 1e18);
        if (j < a.n) { p = a.pos[j]; p.w = (double)(a.perm ? (long)a.perm[j] : j); }
        rec[lane] = p;
      } else {
        rec[lane] = make_double4(vi_ok ? xi : -1e100, vi_ok ? yi : -1e100, vi_ok ? zi : -1e100, idx_i);
        if constexpr (!BODY) {
          if (k0 == 0 && vi_ok) u_one += (zi > 0.0) ? one_blob_potential<FORM>(a, zi) : 1e5 * (1.0 - zi);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int kb = (diag && k0 < 1) ? 1 : k0;
      const int ke = (diag && k1 > 33) ? 33 : k1;
      // a tile that reaches the wall plane (zmin <= 0) needs the lower-index test of the reference's loop limits
      // (BODY: no gate at all -- padding sits 2e100 away, where the exponential is exactly 0)
      const bool above = BODY || (a.bounds[6L * I + 2] > 0.0 && a.bounds[6L * J + 2] > 0.0);
      // step 32 of a diagonal unit is met from both of its lanes: it is peeled off the loop and taken by the lower half
      const bool peel = diag && kb <= 32 && ke > 32;
      const int kl = peel ? 32 : ke;
      if (above) {
        for (int k = kb; k < kl; ++k) {
          const double4 q = rec[(lane + k) & 63];
          u_pair += pair_potential<FORM>(a, image<PERIODIC>(a.Lx, a.iLx, xi - q.x), image<PERIODIC>(a.Ly, a.iLy, yi - q.y), image_z<PERIODIC, BODY>(a, zi - q.z));
        }
        if (peel) {
          const double4 q = rec[(lane + 32) & 63];
          const double u = pair_potential<FORM>(a, image<PERIODIC>(a.Lx, a.iLx, xi - q.x), image<PERIODIC>(a.Ly, a.iLy, yi - q.y), image_z<PERIODIC, BODY>(a, zi - q.z));
          u_pair += lane < 32 ? u : 0.0;
        }
      } else {
        for (int k = kb; k < ke; ++k) {
          const double4 q = rec[(lane + k) & 63];
          const double u = pair_potential<FORM>(a, image<PERIODIC>(a.Lx, a.iLx, xi - q.x), image<PERIODIC>(a.Ly, a.iLy, yi - q.y), image_z<PERIODIC, BODY>(a, zi - q.z));
          const double z_low = idx_i < q.w ? zi : q.z;       // the blob with the lower caller's index decides
          const bool real = idx_i < 1e17 && q.w < 1e17;      // padding carries index 1e18
          const bool skip = (peel && k == 32 && lane >= 32) || !real || !(z_low > 0.0);
          u_pair += skip ? 0.0 : u;
        }
      }
      __builtin_amdgcn_wave_barrier();   // rec is rewritten by the next unit
      if (k1 == 64) unit_next(a.order, a.n_tiles, I, J);
    }
  }
  // fixed butterfly over the lanes, one pair of partials per wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    u_one += __shfl_xor(u_one, off);
    u_pair += __shfl_xor(u_pair, off);
  }
  if (lane == 0) { a.partial[2 * w] = u_one; a.partial[2 * w + 1] = u_pair; }
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
