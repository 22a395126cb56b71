// mcmc_move_kernels.h -- single-body Metropolis moves (gfx950, fp64): the energy difference of ONE moved body in O(n_b N)
// and the launch that decides and commits it.
//
// E(r) = sum_i u1(z_i) + sum_{i<j, z_i>0} u2(r_ij) is what potential_kernel computes (potential_kernels.h; its device
// functions are used here by inclusion).  A body owns the contiguous blob range [first, first + count); r' differs from r
// only there, so E(r') - E(r) is a sum over the pairs that touch the range plus the body's own one-blob terms:
//   j < first            the pair (j, i): gate z_j > 0, the same before and after
//   j >= first + count   the pair (i, j): gate z'_i > 0 for the new term, z_i > 0 for the old one
//   j inside the body    the pair (i, j), i < j, once: gates as the row above, both ends moved (met by the lane of the
//                        LOWER blob, whose chunk is then the first one it needs: it takes its proposed row from the slab)
// body_delta_kernel: one lane per blob j of the whole configuration (its row of r read once), the body's old and new
// coordinates staged in LDS, kMoveChunk blobs at a time; every lane subtracts per pair (new - old) before it accumulates, the
// lane whose j lies in the body adds u1(z'_j) - u1(z_j); a wave reduces with a fixed butterfly and stores one pair of
// partials.  No culling, no sort, no atomic: the pass is O(n_b N) and its sum has one order, so a seeded chain repeats to
// the bit.  COMPOSE: the proposed coordinates are not read but composed from the draws of this body (the arithmetic of
// mcmc_propose_kernel, rmb_potential.hip); workgroup 0 leaves them, with the proposed location and quaternion, in `prop`.
// move_finish_kernel (one workgroup; a kernel boundary, not a grid barrier) adds the partials in a fixed order and either
// stores the two differences (the stateless entry) or decides u < exp(-dE/kT) with numpy's comparison (NaN rejects, -inf
// accepts) and commits in place: the body's rows of r, its location and quaternion, the running {U_one, U_pair}, the flag.
// A rejected move writes the flag and nothing else.
//
// BODY: E gains U_body = sum_{i<j} eps_b exp(-|x_i - x_j|/b_b) / |x_i - x_j| over the body LOCATIONS (potential_kernel's BODY
// instance: minimal image in all three directions, no wall gate).  Moving body k touches its n_bodies - 1 centre pairs: the
// lane whose global index j is a body other than k reads loc[j] (committed in place by the earlier moves of the sweep) and
// adds u(|loc_j - x'_k|) - u(|loc_j - x_k|) to a third running sum; x'_k is the pose every lane composes (COMPOSE) or the
// caller's triple.  One more partial per wave through the same butterfly, three sums in the finishing launch, a running
// energy of three doubles.  Bodies from n_free on are never moved but take part in the pairs.  The grid covers
// max(n_blobs, n_bodies) lanes.
#pragma once
#include "potential_kernels.h"

namespace rmb {

constexpr int kMoveChunk = 256;      // body blobs staged per round: 2 x 256 x 3 doubles = 12 KB
constexpr int kMoveWaves = kMoveChunk / 64;

struct MoveArgs {
  PotentialArgs p;          // the potential's parameters, box and exp constants (what one_blob_potential / pair_potential read)
  const double* r;          // (n, 3) raw blob coordinates, caller's order
  long n, first, count;     // the moved body's blob range
  const double* body_new;   // (count, 3) proposed coordinates of the body (!COMPOSE)
  // COMPOSE: body k of the sampler's state
  long body;
  const int* blob_ref;      // [n] row of `ref` of every blob
  const double* ref;        // (rows, 3)
  const double *loc, *quat; // (n_bodies, 3), (n_bodies, 4)
  const double* draws;      // (n_free, 7): displacement, rotation vector / max_angle_shift, uniform
  double max_angle_shift;
  double* prop;             // [3 count] proposed coordinates, then [3] location, [4] quaternion (COMPOSE: written by workgroup 0)
  // BODY: the centre term
  long n_bodies;
  const double* loc_new3;   // [3] proposed location of the moved body (!COMPOSE)
  double body_eps, body_inv_b;
  double* partial;          // [n_waves][2], BODY: [n_waves][3]
  long n_partial;
  // finishing launch
  double* out;              // {dU_one, dU_pair} (decide == 0); BODY: {dU_one, dU_pair, dU_body}
  int decide;
  double kT;
  double *r_rw, *loc_rw, *quat_rw;   // committed in place on acceptance
  double* energy;           // running {U_one, U_pair}; BODY: {U_one, U_pair, U_body}
  int* accepted;            // [n_free] flag of every move of the sweep
};

struct MovePose { double x, y, z, s, p0, p1, p2; };

// many_body_MCMC.py:160-169 for one body: x' = x + du, q' = quaternion(dphi) q -- mcmc_propose_kernel's arithmetic
__device__ __forceinline__ MovePose proposed_pose(const MoveArgs& a) {
  const long b = a.body;
  const double* d = a.draws + 7 * b;
  MovePose m;
  m.x = a.loc[3 * b] + d[0]; m.y = a.loc[3 * b + 1] + d[1]; m.z = a.loc[3 * b + 2] + d[2];
  const double s = a.quat[4 * b], p0 = a.quat[4 * b + 1], p1 = a.quat[4 * b + 2], p2 = a.quat[4 * b + 3];
  const double px = d[3] * a.max_angle_shift, py = d[4] * a.max_angle_shift, pz = d[5] * a.max_angle_shift;
  const double nrm = sqrt(px * px + py * py + pz * pz);
  const double qs = cos(0.5 * nrm), f = nrm != 0.0 ? sin(0.5 * nrm) / nrm : 0.0;
  const double qx = f * px, qy = f * py, qz = f * pz;
  m.s = qs * s - (qx * p0 + qy * p1 + qz * p2);
  m.p0 = qs * p0 + s * qx + (qy * p2 - qz * p1);
  m.p1 = qs * p1 + s * qy + (qz * p0 - qx * p2);
  m.p2 = qs * p2 + s * qz + (qx * p1 - qy * p0);
  return m;
}

// r = R(q') ref + x' of blob `id` (body.py:64-78), as mcmc_propose_kernel
__device__ __forceinline__ void proposed_blob(const MoveArgs& a, const MovePose& m, long id, double& x, double& y, double& z) {
  const double* rf = a.ref + 3L * a.blob_ref[id];
  const double s = m.s, p0 = m.p0, p1 = m.p1, p2 = m.p2;
  const double d = s * s - 0.5;
  const double rx = 2.0 * ((p0 * p0 + d) * rf[0] + (p0 * p1 - s * p2) * rf[1] + (p0 * p2 + s * p1) * rf[2]);
  const double ry = 2.0 * ((p1 * p0 + s * p2) * rf[0] + (p1 * p1 + d) * rf[1] + (p1 * p2 - s * p0) * rf[2]);
  const double rz = 2.0 * ((p2 * p0 - s * p1) * rf[0] + (p2 * p1 + s * p0) * rf[1] + (p2 * p2 + d) * rf[2]);
  x = rx + m.x; y = ry + m.y; z = rz + m.z;
}

// u1 with the rule behind the wall
template <int FORM>
__device__ __forceinline__ double one_blob_full(const PotentialArgs& p, double z) {
  return z > 0.0 ? one_blob_potential<FORM>(p, z) : 1e5 * (1.0 - z);
}

// u of one pair of body centres from their separation: the yukawa pair expression on the body law's parameters, imaged in
// every direction with a positive period
template <bool PERIODIC>
__device__ __forceinline__ double centre_potential(const MoveArgs& a, double dx, double dy, double dz) {
  dx = image<PERIODIC>(a.p.Lx, a.p.iLx, dx); dy = image<PERIODIC>(a.p.Ly, a.p.iLy, dy); dz = image<PERIODIC>(a.p.Lz, a.p.iLz, dz);
  const double r2 = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
  const double ir = r2 > 0.0 ? rsqrt_f64(r2) : __builtin_inf();
  const double r = r2 > 0.0 ? r2 * ir : 0.0;
  return a.body_eps * exp_nonpositive(a.p.ec, -r * a.body_inv_b) * ir;
}

template <int FORM, bool PERIODIC, bool COMPOSE, bool BODY = false>
__global__ __launch_bounds__(kMoveChunk) void body_delta_kernel(const MoveArgs a) {
  __shared__ double s_old[kMoveChunk][3];
  __shared__ double s_new[kMoveChunk][3];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const long j = (long)blockIdx.x * kMoveChunk + t;
  const long end = a.first + a.count;
  const bool valid = j < a.n;
  const bool in_body = valid && j >= a.first && j < end;
  const bool j_low = j < a.first;      // j is the lower index of every pair it forms with the body
  MovePose m;
  if constexpr (COMPOSE) {
    m = proposed_pose(a);
    if (blockIdx.x == 0 && t == 0) {
      double* q = a.prop + 3 * a.count;
      q[0] = m.x; q[1] = m.y; q[2] = m.z; q[3] = m.s; q[4] = m.p0; q[5] = m.p1; q[6] = m.p2;
    }
  }
  // this lane's end of the pairs: its row of r; a lane of the body takes its proposed row from the slab of its own chunk
  // (staged ONCE per workgroup: the pairs inside the body and the committed rows see the same numbers)
  double xo = 0.0, yo = 0.0, zo = 1.0, xn = 0.0, yn = 0.0, zn = 1.0;
  if (valid) {
    xo = a.r[3 * j]; yo = a.r[3 * j + 1]; zo = a.r[3 * j + 2];
    xn = xo; yn = yo; zn = zo;
  }
  double d_one = 0.0, d_pair = 0.0;
  [[maybe_unused]] double d_body = 0.0;
  if constexpr (BODY) {
    if (j < a.n_bodies && j != a.body) {      // this lane's centre against the moved one, before and after
      const double lx = a.loc[3 * j], ly = a.loc[3 * j + 1], lz = a.loc[3 * j + 2];
      const double ox = a.loc[3 * a.body], oy = a.loc[3 * a.body + 1], oz = a.loc[3 * a.body + 2];
      double nx, ny, nz;
      if constexpr (COMPOSE) { nx = m.x; ny = m.y; nz = m.z; }
      else { nx = a.loc_new3[0]; ny = a.loc_new3[1]; nz = a.loc_new3[2]; }
      d_body = centre_potential<PERIODIC>(a, lx - nx, ly - ny, lz - nz) - centre_potential<PERIODIC>(a, lx - ox, ly - oy, lz - oz);
    }
  }
  // the lane's own height gates the pairs in which it is the lower index: j below the body, and j inside it (which meets
  // the body blobs ABOVE it, so that its own chunk is the first it needs)
  const bool own_gate = j_low || in_body;
  for (long c0 = a.first; c0 < end; c0 += kMoveChunk) {
    const long left = end - c0;
    const int len = left < kMoveChunk ? (int)left : kMoveChunk;
    if (t < len) {
      const long i = c0 + t;
      const double x = a.r[3 * i], y = a.r[3 * i + 1], z = a.r[3 * i + 2];
      s_old[t][0] = x; s_old[t][1] = y; s_old[t][2] = z;
      double x1, y1, z1;
      if constexpr (COMPOSE) {
        proposed_blob(a, m, i, x1, y1, z1);
        if (blockIdx.x == 0) {
          double* q = a.prop + 3 * (i - a.first);
          q[0] = x1; q[1] = y1; q[2] = z1;
        }
      } else {
        const double* q = a.body_new + 3 * (i - a.first);
        x1 = q[0]; y1 = q[1]; z1 = q[2];
      }
      s_new[t][0] = x1; s_new[t][1] = y1; s_new[t][2] = z1;
    }
    __syncthreads();
    int start = 0;
    if (in_body) {
      const long own = j - c0;      // this lane's slot in the chunk (>= len: its chunk is still to come; negative: it is past)
      if (own >= 0 && own < len) {
        xn = s_new[own][0]; yn = s_new[own][1]; zn = s_new[own][2];
        d_one = one_blob_full<FORM>(a.p, zn) - one_blob_full<FORM>(a.p, zo);
      }
      start = own < 0 ? 0 : (own + 1 < len ? (int)(own + 1) : len);      // only the body blobs above it: the pair counts once
    }
    if (!valid) start = len;
    for (int k = start; k < len; ++k) {
      const double ox = s_old[k][0], oy = s_old[k][1], oz = s_old[k][2];
      const double nx = s_new[k][0], ny = s_new[k][1], nz = s_new[k][2];
      const double u_new = pair_potential<FORM>(a.p, image<PERIODIC>(a.p.Lx, a.p.iLx, nx - xn), image<PERIODIC>(a.p.Ly, a.p.iLy, ny - yn), nz - zn);
      const double u_old = pair_potential<FORM>(a.p, image<PERIODIC>(a.p.Lx, a.p.iLx, ox - xo), image<PERIODIC>(a.p.Ly, a.p.iLy, oy - yo), oz - zo);
      const bool g_new = own_gate ? zn > 0.0 : nz > 0.0;
      const bool g_old = own_gate ? zo > 0.0 : oz > 0.0;
      d_pair += (g_new ? u_new : 0.0) - (g_old ? u_old : 0.0);
    }
    __syncthreads();      // the next chunk rewrites the slabs
  }
  // fixed butterfly over the lanes, one pair (BODY: triple) of partials per wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    d_one += __shfl_xor(d_one, off);
    d_pair += __shfl_xor(d_pair, off);
    if constexpr (BODY) d_body += __shfl_xor(d_body, off);
  }
  if (lane == 0) {
    const long w = (long)blockIdx.x * kMoveWaves + (t >> 6);
    if constexpr (BODY) { a.partial[3 * w] = d_one; a.partial[3 * w + 1] = d_pair; a.partial[3 * w + 2] = d_body; }
    else { a.partial[2 * w] = d_one; a.partial[2 * w + 1] = d_pair; }
  }
}

// One workgroup: the partials in a fixed order (thread t: t, t + 256, ...; then a tree over the 256 threads, as
// potential_finish_kernel), then the result (decide == 0) or the Metropolis decision and the commit.  BODY: three sums.
template <bool BODY = false>
__global__ __launch_bounds__(256) void move_finish_kernel(const MoveArgs a) {
  constexpr int NS = BODY ? 3 : 2;
  __shared__ double s[NS][256];
  __shared__ int s_ok;
  const int t = threadIdx.x;
  double u[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) u[q] = 0.0;
  for (long k = t; k < a.n_partial; k += 256) {
#pragma unroll
    for (int q = 0; q < NS; ++q) u[q] += a.partial[NS * k + q];
  }
#pragma unroll
  for (int q = 0; q < NS; ++q) s[q][t] = u[q];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int q = 0; q < NS; ++q) s[q][t] += s[q][t + off];
    }
    __syncthreads();
  }
  if (!a.decide) {
    if (t == 0) {
#pragma unroll
      for (int q = 0; q < NS; ++q) a.out[q] = s[q][0];
    }
    return;
  }
  if (t == 0) {
    // numpy's  u < exp(-dE/kT): a NaN compares false (reject), dE = -inf gives exp(inf) = inf (accept)
    double dE = s[0][0] + s[1][0];
    if constexpr (BODY) dE += s[2][0];
    const double u01 = a.draws[7 * a.body + 6];
    const int ok = u01 < exp(-dE / a.kT) ? 1 : 0;
    a.accepted[a.body] = ok;
    if (ok) {
#pragma unroll
      for (int q = 0; q < NS; ++q) a.energy[q] += s[q][0];
    }
    s_ok = ok;
  }
  __syncthreads();
  if (!s_ok) return;
  for (long k = t; k < 3 * a.count; k += 256) a.r_rw[3 * a.first + k] = a.prop[k];
  const double* q = a.prop + 3 * a.count;
  if (t < 3) a.loc_rw[3 * a.body + t] = q[t];
  else if (t < 7) a.quat_rw[4 * a.body + (t - 3)] = q[t];
}

}  // namespace rmb
