// rmb_sweep.hip -- the one-sided kernels (onesided_kernels.h: lane = target, sources streamed through an LDS tile, source
// chunks + fixed-order reduction, atomic-free), each "fill the arguments, pick the instance, one_sided_launch": the pair
// sweep of every kind, the force sweep, the source->target operators with per-blob radii, Stokeslet pressure / Stokes
// double layer; the dense per-body blocks; position packing.
#include "rmb_internal.h"

#include <cmath>

#include "matvec_kernels.h"
#include "dense_kernels.h"
#include "st_kernels.h"
#include "aux_kernels.h"
#include "diag_kernels.h"

namespace rmbi {

namespace {
typedef int (*sweep_launch_fn)(rmb_ctx*, rmb::SweepArgs);

template <int KIND, bool WALL, bool PER>
constexpr sweep_launch_fn sweep_launch() {
  return one_sided_launch<rmb::sweep_kernel<KIND, WALL, PER>, rmb::finalize_kernel<KIND, WALL>, 3, rmb::SweepArgs>;
}

// [kind][wall][periodic]
const sweep_launch_fn g_sweeps[rmb::KIND_COUNT][2][2] = {
#define RMB_ROW(K) {{sweep_launch<K, false, false>(), sweep_launch<K, false, true>()}, {sweep_launch<K, true, false>(), sweep_launch<K, true, true>()}}
    RMB_ROW(rmb::KIND_TT), RMB_ROW(rmb::KIND_TR), RMB_ROW(rmb::KIND_RT), RMB_ROW(rmb::KIND_RR), RMB_ROW(rmb::KIND_TT_TR),
    RMB_ROW(rmb::KIND_TT_FREE),
    // rotational free-surface kinds: raw heights, the wall = 0 instance serves both columns
#define RMB_ROW_RAW(K) {{sweep_launch<K, false, false>(), sweep_launch<K, false, true>()}, {sweep_launch<K, false, false>(), sweep_launch<K, false, true>()}}
    RMB_ROW_RAW(rmb::KIND_TR_FREE), RMB_ROW_RAW(rmb::KIND_RT_FREE), RMB_ROW_RAW(rmb::KIND_RR_FREE), RMB_ROW_RAW(rmb::KIND_TT_TR_FREE)
#undef RMB_ROW_RAW
#undef RMB_ROW
};

// pseudo-periodic lengths (<= 0 or L == nullptr: open) and their inverses into a.Lx .. a.iLz; whether any axis is periodic
template <class Args>
bool set_box(Args& a, const double* L) {
  a.Lx = L ? L[0] : 0.0; a.Ly = L ? L[1] : 0.0; a.Lz = L ? L[2] : 0.0;
  a.iLx = inv_length(a.Lx); a.iLy = inv_length(a.Ly); a.iLz = inv_length(a.Lz);
  return a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
}
}  // namespace

// One-sided sweep of targets [tgt_begin, tgt_end) against all n sources (every ordered pair, fixed summation order).
int sweep_device(rmb_ctx* c, int kind, int in_plane, const double* v, const double* v2, double eta, double* out) {
  rmb::SweepArgs a{};
  a.out = out; a.n_src = c->n; a.tgt_begin = c->tgt_begin; a.tgt_end = c->tgt_end;
  a.pos = (const double4*)c->pos.p;
  a.vec = v;
  a.vec2 = v2;
  a.in_plane = in_plane ? 1 : 0;
  a.prefactor = 1.0 / (8.0 * M_PI * eta);
  const bool periodic = set_box(a, c->L);
  a.k = make_pair_consts(c->a);
  return g_sweeps[kind][c->wall ? 1 : 0][periodic ? 1 : 0](c, a);
}

// One-sided force sweep of the context's target range (multi_bodies/forces_numba.py:12-55), atomic-free.
int force_sweep_device(rmb_ctx* c, double eps, double b, double blob_radius, double* out, const double* radii) {
  rmb::ForceArgs a{};
  a.out = out; a.n_src = c->n; a.tgt_begin = c->tgt_begin; a.tgt_end = c->tgt_end;
  a.pos = (const double4*)c->pos.p;
  const bool periodic = set_box(a, c->L);
  a.eps_over_b = eps / b;
  a.inv_b = 1.0 / b;
  a.two_a = 2.0 * blob_radius;
  a.ec = exp_consts();
  a.radii = radii;
#define RMB_FORCE(PER, RAD) one_sided_launch<rmb::force_sweep_kernel<PER, RAD>, rmb::force_finalize_kernel, 3>(c, a)
  return radii ? (periodic ? RMB_FORCE(true, true) : RMB_FORCE(false, true)) : (periodic ? RMB_FORCE(true, false) : RMB_FORCE(false, false));
#undef RMB_FORCE
}

int pack_positions(rmb_ctx* c, const double* r_dev, long n, double a, const double* L, int wall) {
  // option "free_surface": the boundary at z = 0 is a stress-free surface instead of a no-slip wall -- raw heights, no
  // clamp, no B damping; every kernel instance chosen by c->wall is then the unbounded one, the image comes from the
  // free-surface operation (c->free_surface)
  const bool free_surface = wall && c->opt_free_surface;
  if (int rc = c->pos.reserve((size_t)(n > 0 ? n : 1) * sizeof(double4))) return rc;
  if (n > 0) {
    hipLaunchKernelGGL(rmb::pack_positions_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, r_dev, n,
                       a, wall && !free_surface ? 1 : 0, (double4*)c->pos.p);
    RMB_HIP(hipGetLastError());
  }
  c->n = n;
  c->a = a;
  c->tile_bounds_valid = false;
  for (int k = 0; k < 3; ++k) c->L[k] = L ? L[k] : 0.0;
  c->wall = wall && !free_surface ? 1 : 0;
  c->free_surface = free_surface ? 1 : 0;
  c->tgt_begin = 0;
  c->tgt_end = n;
  c->have_positions = true;
  return 0;
}

int pack_positions_radii(rmb_ctx* c, const double* r_dev, const double* rad_dev, long n, int wall, double4* dst) {
  hipLaunchKernelGGL(rmb::pack_positions_radii_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, r_dev,
                     rad_dev, n, wall, dst);
  RMB_HIP(hipGetLastError());
  return 0;
}

namespace {
__global__ void add_inplace_kernel(double* y, const double* x, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] += x[i];
}
}  // namespace

namespace {
// dst (device memory) = src (page-locked host memory mapped into the device's address space): 16 bytes per lane,
// consecutive lanes consecutive addresses -- the upload of rmb_matvec's input vectors as a kernel of the SAME queue
__global__ __launch_bounds__(256) void pull_mapped_kernel(double* dst, const double* src, long n) {
  const long i = 2 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (i + 1 < n) *reinterpret_cast<double2*>(dst + i) = *reinterpret_cast<const double2*>(src + i);
  else if (i < n) dst[i] = src[i];
}
}  // namespace

int pull_mapped(rmb_ctx* c, double* dst_dev, const double* src_mapped_dev, long n) {
  hipLaunchKernelGGL(pull_mapped_kernel, dim3((unsigned)((n / 2 + 256) / 256)), dim3(256), 0, c->stream, dst_dev, src_mapped_dev, n);
  RMB_HIP(hipGetLastError());
  return 0;
}

int add_inplace(rmb_ctx* c, double* y, const double* x, long n) {
  hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, y, x, n);
  RMB_HIP(hipGetLastError());
  return 0;
}

int body_dense_device(rmb_ctx* c, const long* first_blob_dev, long n_bodies, int n_b, double eta, double* out_dev) {
  rmb::DenseArgs a;
  a.pos = (const double4*)c->pos.p;
  a.first_blob = first_blob_dev;
  a.out = out_dev;
  a.n_b = n_b;
  a.n_bodies = n_bodies;
  a.prefactor = 1.0 / (8.0 * M_PI * eta);
  a.k = make_pair_consts(c->a);
  // blockIdx.y splits the n_b^2 blob pairs of a body so that one big "body" (the dense builders) still fills the chip
  long ysplit = ((long)n_b * n_b + 256L * 16 - 1) / (256L * 16);   // 256 threads x 16 blob pairs each
  if (ysplit < 1) ysplit = 1;
  if (ysplit > 4096) ysplit = 4096;
  const dim3 grid((unsigned)n_bodies, (unsigned)ysplit);
  if (c->free_surface) hipLaunchKernelGGL(rmb::body_dense_tt_kernel<rmb::BND_FREE>, grid, dim3(256), 0, c->stream, a);
  else if (c->wall)    hipLaunchKernelGGL(rmb::body_dense_tt_kernel<rmb::BND_WALL>, grid, dim3(256), 0, c->stream, a);
  else                 hipLaunchKernelGGL(rmb::body_dense_tt_kernel<rmb::BND_NONE>, grid, dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}


// One-sided source -> target sweep with per-blob radii (st_kernels.h); positions already packed (clamped when wall = 1).
int st_sweep_device(rmb_ctx* c, long ns, const double4* src_packed, const double* rad_s, const double* force, long nt,
                    const double4* tgt_packed, const double* rad_t, double eta, const double* L, int wall, double* out) {
  rmb::StArgs a{};
  a.out = out; a.n_src = ns; a.tgt_end = nt;
  a.src = src_packed; a.rad_s = rad_s; a.force = force;
  a.tgt = tgt_packed; a.rad_t = rad_t;
  a.prefactor = 1.0 / (8.0 * M_PI * eta);
  const bool periodic = set_box(a, L);
#define RMB_ST(MODE) (periodic ? one_sided_launch<rmb::st_sweep_kernel<MODE, true>, rmb::st_finalize_kernel, 3>(c, a) \
                               : one_sided_launch<rmb::st_sweep_kernel<MODE, false>, rmb::st_finalize_kernel, 3>(c, a))
  return wall == 2 ? RMB_ST(2) : (wall ? RMB_ST(1) : RMB_ST(0));
#undef RMB_ST
}

namespace {
template <int MODE>
int aux_launch(rmb_ctx* c, const rmb::AuxArgs& a) {
  constexpr int NOUT = rmb::AuxShape<MODE>::NOUT;
  return one_sided_launch<rmb::aux_sweep_kernel<MODE>, rmb::aux_finalize_kernel<NOUT>, NOUT>(c, a);
}
}  // namespace

int pressure_device(rmb_ctx* c, long ns, const double* src_dev, long nt, const double* tgt_dev, const double* force_dev,
                    int wall, double* out_dev) {
  rmb::AuxArgs a{};
  a.src = src_dev; a.tgt = tgt_dev; a.v0 = force_dev; a.v1 = nullptr; a.w = nullptr; a.out = out_dev;
  a.n_src = ns; a.tgt_end = nt; a.prefactor = 1.0 / (4.0 * M_PI); a.a2 = 0.0;
  return wall ? aux_launch<rmb::AUX_P_WALL>(c, a) : aux_launch<rmb::AUX_P_FREE>(c, a);
}

int double_layer_device(rmb_ctx* c, long ns, const double* src_dev, long nt, const double* tgt_dev,
                        const double* normals_dev, const double* vector_dev, const double* weights_dev, int wall,
                        double blob_radius, double* out_dev) {
  rmb::AuxArgs a{};
  a.src = src_dev; a.tgt = tgt_dev; a.v0 = normals_dev; a.v1 = vector_dev; a.w = weights_dev; a.out = out_dev;
  a.n_src = ns; a.tgt_end = nt; a.prefactor = -3.0 / (4.0 * M_PI); a.a2 = blob_radius >= 0.0 ? blob_radius * blob_radius : 0.0;
  if (blob_radius >= 0.0) return aux_launch<rmb::AUX_DL_RPY>(c, a);
  return wall ? aux_launch<rmb::AUX_DL_WALL>(c, a) : aux_launch<rmb::AUX_DL_FREE>(c, a);
}

int ubench_fp64_issue(rmb_ctx* c, int launches, double* g_wave_instr_per_s) {
  RMB_HIP(hipSetDevice(c->device));
  const long blocks = c->n_cu * 4;                    // 4 workgroups of 4 waves per CU = 4 waves per SIMD
  if (int rc = c->tmp3n.reserve((size_t)blocks * 256 * sizeof(double))) return rc;
  hipEvent_t e0, e1;
  RMB_HIP(hipEventCreate(&e0));
  RMB_HIP(hipEventCreate(&e1));
  hipLaunchKernelGGL(rmb::ubench_fma64_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, (double*)c->tmp3n.p, 1.0000001, 1e-9);
  RMB_HIP(hipEventRecord(e0, c->stream));
  for (int i = 0; i < launches; ++i)
    hipLaunchKernelGGL(rmb::ubench_fma64_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, (double*)c->tmp3n.p, 1.0000001, 1e-9);
  RMB_HIP(hipEventRecord(e1, c->stream));
  RMB_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  RMB_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  const double instr = (double)launches * blocks * 4 * rmb::kUbenchIters * rmb::kUbenchFmaPerIter;
  *g_wave_instr_per_s = instr / (ms * 1e-3) / 1e9;
  return 0;
}

}  // namespace rmbi
