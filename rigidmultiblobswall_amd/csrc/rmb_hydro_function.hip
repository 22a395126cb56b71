// rmb_hydro_function.hip -- the hydrodynamic function H(k) (hydro_function_kernels.h): the raw sums S_self and S_dist of a
// batch of caller-owned frames, and of the resident configuration; what hydrofunction.py streams a trajectory through.
#include "rmb_internal.h"

#include <cmath>

#include "hydro_function_kernels.h"

namespace rmbi {
namespace {

typedef rmb::HydroArgs A;
constexpr long kHydroMaxK = 16384, kHydroMaxN = 32768;      // the scattering entries' limits
constexpr size_t kHydroPartBytes = 64u << 20;               // what the per-chunk records of one launch may take

// everything that can be said without the context or the device
int check_hydro_args(const std::string& w, double a, double eta, const double* mob_L, const double* L, const int* kint, const double* pol,
                     long K, bool out_ok) {
  if (K < 0) return fail(RMB_ERR_ARG, w + ": negative size");
  if (K > kHydroMaxK) return fail(RMB_ERR_ARG, w + ": at most 16384 wavevectors per call");
  if (!L || !mob_L) return fail(RMB_ERR_ARG, w + ": null length pointer");
  if (K > 0 && (!kint || !pol)) return fail(RMB_ERR_ARG, w + ": null wavevector or polarisation pointer");
  if (!out_ok) return fail(RMB_ERR_ARG, w + ": null out pointer");
  if (!(a > 0.0) || !std::isfinite(a)) return fail(RMB_ERR_ARG, w + ": the radius must be positive and finite");
  if (!(eta > 0.0) || !std::isfinite(eta)) return fail(RMB_ERR_ARG, w + ": eta must be positive and finite");
  for (long i = 0; i < 3 * K; ++i) {
    const long n = kint[i];
    if (n > kHydroMaxN || n < -kHydroMaxN) return fail(RMB_ERR_ARG, w + ": |n_d| must be at most 32768");
    if (n != 0 && !(L[i % 3] > 0.0)) return fail(RMB_ERR_ARG, w + ": n_d != 0 needs a positive length L_d");
    if (!std::isfinite(pol[i])) return fail(RMB_ERR_ARG, w + ": a polarisation is not finite");
  }
  // the phase factor of a pair must not depend on the image: the mobility's period is the wavevector's length
  for (int d = 0; d < 3; ++d)
    if (mob_L[d] > 0.0 && mob_L[d] != L[d])
      return fail(RMB_ERR_ARG, w + ": the mobility's period must equal the wavevector length in every periodic direction");
  return 0;
}

// an instance as the plan sees it (SymKernel: handle, LDS, occupancy cache) and its launch on the two-dimensional grid
struct HydroKernel {
  SymKernel k;
  void (*launch)(const A& a, unsigned blocks, unsigned k_chunks, hipStream_t s);
  void (*launch_self)(const A& a, hipStream_t s);      // the self sums, one workgroup per frame
};
template <bool WALL, bool PERIODIC, bool BATCH>
void hydro_kernel_launch(const A& a, unsigned blocks, unsigned k_chunks, hipStream_t s) {
  hipLaunchKernelGGL((rmb::hydro_function_kernel<WALL, PERIODIC, BATCH>), dim3(blocks, k_chunks), dim3(64 * rmb::kSymWaves), 0, s, a);
}
template <bool WALL, bool PERIODIC, bool BATCH>
void hydro_self_launch(const A& a, hipStream_t s) {
  hipLaunchKernelGGL((rmb::hydro_self_kernel<WALL, PERIODIC, BATCH>), dim3((unsigned)a.n_frames), dim3(256), 0, s, a);
}
template <bool WALL, bool PERIODIC, bool BATCH>
HydroKernel hydro_instance() {
  const size_t lds = (sizeof(double4) + sizeof(double2) * rmb::kHydroKC) * 64 * rmb::kSymWaves;
  return HydroKernel{sym_kernel_of<A, rmb::hydro_function_kernel<WALL, PERIODIC, BATCH>>(lds), hydro_kernel_launch<WALL, PERIODIC, BATCH>,
                     hydro_self_launch<WALL, PERIODIC, BATCH>};
}
template <bool BATCH>
HydroKernel hydro_kernel_of(bool wall, bool periodic) {
  if (wall) return periodic ? hydro_instance<true, true, BATCH>() : hydro_instance<true, false, BATCH>();
  return periodic ? hydro_instance<false, true, BATCH>() : hydro_instance<false, false, BATCH>();
}

// `a` comes with the configuration (n, n_tiles, frames or pos, units_per_frame, n_frames, step_end, periods, radius); the
// rest -- coefficients, plan, workspace, the sweep and the finishing launch -- is the same for both entries
template <bool BATCH>
int hydro_launch(rmb_ctx* c, A& a, bool wall, double eta, const double* L, const int* kint, const double* pol, long K, double* out_dev) {
  const long ny = (K + rmb::kHydroKC - 1) / rmb::kHydroKC, k_pad = ny * rmb::kHydroKC;
  a.k = make_pair_consts(a.radius);
  a.prefactor = 1.0 / (8.0 * M_PI * eta);
  a.K = K; a.out = out_dev;
  a.order = 0; a.xcd = 0;
  a.iLx = inv_length(a.Lx); a.iLy = inv_length(a.Ly); a.iLz = inv_length(a.Lz);
  const bool periodic = a.Lx > 0 || a.Ly > 0 || a.Lz > 0;
  const HydroKernel k = hydro_kernel_of<BATCH>(wall, periodic);
  // How a frame is cut must not depend on the frames it comes with (a trajectory gives the same sums however it is
  // streamed), so the chunk length comes from the plan of ONE frame: the plan of the culling sweeps ("sym_oversub" rounds, a
  // quarter of "sym_chunk_steps" per strided chunk; its workgroups are shared by the chunks of wavevectors), or one range
  // per wave of that plan.  Every chunk of steps leaves a record per chunk of wavevectors: the chunk is lengthened until
  // the records of a frame fit kHydroPartBytes, and a call takes as many frames per launch as fit.
  const long spf = a.units_per_frame * 64, n_frames = a.n_frames;
  long blocks1, chunk1;
  plan_cull_sweep(c, k.k, spf, &blocks1, &chunk1);
  const long waves1 = (blocks1 + ny - 1) / ny * rmb::kSymWaves;
  a.spw = chunk1 > 0 ? chunk1 : (spf + waves1 - 1) / waves1;
  const long max_chunks = (long)(kHydroPartBytes / ((size_t)ny * rmb::kHydroKC * sizeof(double)));      // >= 512
  if (a.spw < (spf + max_chunks - 1) / max_chunks) a.spw = (spf + max_chunks - 1) / max_chunks;
  a.chunk_steps = a.spw;
  a.chunks_per_frame = (spf + a.spw - 1) / a.spw;
  long batch = max_chunks / a.chunks_per_frame;      // frames per launch
  if (batch > n_frames) batch = n_frames;
  if (ny > 65535 || batch * a.chunks_per_frame > 0x7fffffffL) return fail(RMB_ERR_ARG, "hydrodynamic function: too many pairs for one launch");

  const size_t coef_bytes = (size_t)k_pad * 3 * sizeof(double), e6_bytes = (size_t)k_pad * 6 * sizeof(double);
  const size_t self_bytes = (size_t)batch * 6 * sizeof(double);
  const size_t part_bytes = (size_t)ny * batch * a.chunks_per_frame * rmb::kHydroKC * sizeof(double);
  if (int rc = c->hydro_ws.reserve(coef_bytes + e6_bytes + self_bytes + part_bytes)) return rc;
  double* coef = (double*)c->hydro_ws.p;
  double* e6 = coef + 3 * k_pad;
  a.coef = coef; a.e6 = e6;
  a.self6 = e6 + 6 * k_pad;
  a.part = a.self6 + 6 * batch;
  // wavevectors past K (the last chunk's padding) read zeros: every term of theirs is an exact zero nobody reads
  RMB_HIP(hipMemsetAsync(coef, 0, coef_bytes + e6_bytes, c->stream));
  for (long k0 = 0; k0 < K; k0 += rmb::kHydroCoefBatch) {      // integers and polarisations by value: no host memory is read later
    rmb::HydroCoefArgs ca{};
    ca.count = K - k0 < rmb::kHydroCoefBatch ? K - k0 : rmb::kHydroCoefBatch;
    for (long i = 0; i < 3 * ca.count; ++i) { ca.n[i] = kint[3 * k0 + i]; ca.e[i] = pol[3 * k0 + i]; }
    for (int d = 0; d < 3; ++d) ca.L[d] = L[d];
    ca.coef = coef + 3 * k0; ca.e6 = e6 + 6 * k0;
    hipLaunchKernelGGL(rmb::hydro_coef_kernel, dim3(1), dim3(rmb::kHydroCoefBatch), 0, c->stream, ca);
    RMB_HIP(hipGetLastError());
  }
  // launched directly: of the context only the device, the stream and the workspace are used
  const double* frames = a.frames;
  for (long f0 = 0; f0 < n_frames; f0 += batch) {
    a.n_frames = n_frames - f0 < batch ? n_frames - f0 : batch;
    if constexpr (BATCH) a.frames = frames + 3 * a.n * f0;
    a.out = out_dev + 2 * K * f0;
    a.step_end = a.n_frames * spf;
    a.n_seg = a.n_frames * a.chunks_per_frame;
    long blocks, unused;      // workgroups of the whole launch, shared by the chunks of wavevectors; no more waves than chunks
    plan_cull_sweep(c, k.k, a.step_end, &blocks, &unused);
    blocks = (blocks + ny - 1) / ny;
    if (blocks > (a.n_seg + rmb::kSymWaves - 1) / rmb::kSymWaves) blocks = (a.n_seg + rmb::kSymWaves - 1) / rmb::kSymWaves;
    k.launch_self(a, c->stream);
    RMB_HIP(hipGetLastError());
    k.launch(a, (unsigned)blocks, (unsigned)ny, c->stream);
    RMB_HIP(hipGetLastError());
    hipLaunchKernelGGL(rmb::hydro_finish_kernel, dim3((unsigned)((a.n_frames * K + 255) / 256)), dim3(256), 0, c->stream, a);
    RMB_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace rmbi

using rmbi::fail;

extern "C" {

int rmb_hydro_function_frames_device(rmb_ctx* c, const double* frames_dev, long n_frames, long n, double a, double eta, int wall,
                                     const double* mob_L, const double* L, const int* kint, const double* pol, long K, double* out_dev) {
  const std::string w("hydrodynamic function");
  if (n_frames < 0 || n < 0) return fail(RMB_ERR_ARG, w + ": negative size");
  const bool nothing = n_frames == 0 || K == 0;      // an empty out may be null
  if (int rc = rmbi::check_hydro_args(w, a, eta, mob_L, L, kint, pol, K, nothing || out_dev)) return rc;
  if (wall != 0 && wall != 1) return fail(RMB_ERR_ARG, w + ": wall must be 0 or 1");
  if (!nothing && n > 0 && !frames_dev) return fail(RMB_ERR_ARG, w + ": null frames pointer");
  if (!c) return fail(RMB_ERR_ARG, "null context");
  if (c->opt_precision == 32) return fail(RMB_ERR_STATE, w + ": fp64 only (option \"precision\" is 32)");
  if (nothing) return 0;
  RMB_HIP(hipSetDevice(c->device));
  if (n == 0) {      // no point, no term
    RMB_HIP(hipMemsetAsync(out_dev, 0, (size_t)n_frames * K * 2 * sizeof(double), c->stream));
    return 0;
  }
  const long tiles = (n + 63) / 64;
  if (tiles > 0x7fffffffL) return fail(RMB_ERR_ARG, w + ": too many points per frame");
  const long upf = tiles * (tiles + 1) / 2;
  if ((double)upf * (double)n_frames * 64.0 > 9.0e18) return fail(RMB_ERR_ARG, w + ": too many pairs for one launch");
  rmbi::A arg{};
  arg.n = n; arg.n_tiles = (int)tiles;
  arg.frames = frames_dev; arg.units_per_frame = upf; arg.n_frames = n_frames;
  arg.step_end = upf * n_frames * 64;
  arg.Lx = mob_L[0]; arg.Ly = mob_L[1]; arg.Lz = mob_L[2];
  arg.radius = a;
  return rmbi::hydro_launch<true>(c, arg, wall != 0, eta, L, kint, pol, K, out_dev);
}

int rmb_hydro_function_device(rmb_ctx* c, double eta, const double* L, const int* kint, const double* pol, long K, double* out_dev) {
  const std::string w("hydrodynamic function");
  if (int rc = rmbi::check_ready(c)) return rc;
  if (c->free_surface) return fail(RMB_ERR_STATE, w + ": no free-surface configurations (wall or unbounded only)");
  if (c->opt_precision == 32) return fail(RMB_ERR_STATE, w + ": fp64 only (option \"precision\" is 32)");
  if (c->tgt_begin != 0 || c->tgt_end != c->n) return fail(RMB_ERR_STATE, w + ": runs over all points: reset the target range");
  if (int rc = rmbi::check_hydro_args(w, c->a, eta, c->L, L, kint, pol, K, K == 0 || out_dev)) return rc;
  if (K == 0) return 0;
  RMB_HIP(hipSetDevice(c->device));
  if (c->n == 0) {
    RMB_HIP(hipMemsetAsync(out_dev, 0, (size_t)K * 2 * sizeof(double), c->stream));
    return 0;
  }
  const long tiles = (c->n + 63) / 64;
  if (tiles > 0x7fffffffL) return fail(RMB_ERR_ARG, w + ": too many points");
  rmbi::A arg{};
  arg.n = c->n; arg.n_tiles = (int)tiles;
  arg.pos = (const double4*)c->pos.p;      // packed (x, y, clamped z, b); the caller's order: nothing is culled, nothing sorted
  arg.units_per_frame = tiles * (tiles + 1) / 2; arg.n_frames = 1;
  arg.step_end = arg.units_per_frame * 64;
  arg.Lx = c->L[0]; arg.Ly = c->L[1]; arg.Lz = c->L[2];
  arg.radius = c->a;
  return rmbi::hydro_launch<false>(c, arg, c->wall != 0, eta, L, kint, pol, K, out_dev);
}

}  // extern "C"
