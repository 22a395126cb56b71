// rmb_internal.h -- what the translation units of librmb_mobility.so share (never installed; the boundary is
// include/rmb_mobility.h).
//
//   rmb_context.hip  error state, context life cycle, streams, the option table (kOptions: every key, its member of rmb_ctx
//                    and how a set value is normalised), DevBuf / MappedBuf, timing ring, diagnostics, default context
//   rmb_plan.hip     launch plans: source chunks, residency, the balanced step schedule of the symmetric kernels,
//                    pair-shard ranges, kernel-uniform constants
//   rmb_sym.hip      the symmetric (each unordered pair once) fp64 sweeps: one launch path (fill_sym_args, choose_sym,
//                    sym_launch below) under sym / sym2 / symx / the symmetric force kernel; symx_det
//   rmb_sym32.hip    their single-precision twins (handed over as SymKernel thunks)
//   rmb_symx_coop.hip  workgroup-cooperative instances of the generic symmetric skeleton (SymKernel thunks too)
//   rmb_symx2t.hip, rmb_symx2t_per.hip  two-targets-per-lane instances of the generic skeleton, open / pseudo-periodic
//   rmb_sort.hip     Morton ordering of the blobs for the force kernel's tile culling (rocPRIM radix sort)
//   rmb_sweep.hip    the one-sided kernels (one frame, onesided_kernels.h; one launcher, one_sided_launch below): sweep,
//                    force sweep, source->target, pressure / double layer; dense body blocks, position packing
//   rmb_entry.hip    the extern "C" products: argument checks, routing between the two families, host staging (aux_stage /
//                    download; rmb_matvec's mapped hand-off)
//   rmb_multi.hip    the single-process multi-device engine (rmb_multi_*)
//   rmb_rigid.hip    per-body geometry (positions, K) and the per-body factors of the block-diagonal preconditioner
//   rmb_krylov.hip   O(N) helpers of the rigid-body solve: batched 2 x 2 block product, fused Gram-Schmidt step
//   rmb_gmres.hip    the whole right-preconditioned GMRES of the rigid-body problem and the Lanczos forcings as one call each
//                    (host loop native too); one workspace layout for both (krylov_workspace)
//   rmb_potential.hip  total potential energy of a blob configuration (potential_kernels.h: a policy of the pair-once frame,
//                    pair_once_kernels.h; atomic-free) and the Metropolis proposal of the equilibrium sampler
//   rmb_mcmc_moves.hip  single-body Metropolis moves (mcmc_move_kernels.h): energy difference of one moved body, and a
//                    whole sweep of moves decided and committed on the device
//   rmb_pair_hist.hip  histogram of pair distances (pair_hist_kernels.h: the other policy of that frame, integer counters
//                    in LDS, integer atomics to the caller's uint64 bins): resident points, and a batch of caller-owned frames
//   rmb_laplace.hip  Laplace layer operators of phoretic bodies (laplace_kernels.h): the six reference-shaped host entry
//                    points and the two fused device sweeps of the concentration solve
//   rmb_msd.hip      6 x 6 mean-square displacement sums of caller-owned rigid-body frames (msd_kernels.h: a policy of the
//                    lag-sweep frame, lag_sweep_kernels.h -- a lane owns a lag): record pass, lag sweep, finishing launch
//   rmb_scattering.hip  density modes rho_k(f) of caller-owned frames (scattering_kernels.h: a lane owns a wavevector) and the
//                    lag sums of S(k), F(k, t), F_s(k, t) (the other policy of that frame, over the modes or per-point phase
//                    records)
//   rmb_van_hove.hip  lag histograms behind the van Hove functions G_s(r, t), G_d(r, t) of caller-owned frames
//                    (van_hove_kernels.h): self sweep (a lane owns a point; counts and the moments sum r^2, sum r^4, finishing
//                    launch) and distinct sweep over ordered pairs (a workgroup owns a lag; the rotation of the pair-once frame)
//   rmb_bond_order.hip  bond-orientational order of caller-owned frames (bond_order_kernels.h): the neighbour sums behind psi_m
//                    (a policy of the one-sided frame, launched here with the frame as a grid dimension) and the pair correlation
//                    of a quantised per-point field behind g_m(r) (a policy of the pair-once frame, integer accumulators)
//   rmb_clusters.hip  connected components of the bond graph (cluster_kernels.h: a policy of the pair-once frame whose pair term
//                    is a lock-free union-find in global memory), of caller-owned frames and of the resident raw positions:
//                    init, sweep and finishing launch
//   rmb_hydro_function.hip  the hydrodynamic function H(k) (hydro_function_kernels.h: a policy of the pair-once frame that keeps
//                    the phase factors of the staged tile in a second LDS slab; the tt pair block built once per pair and
//                    contracted with a chunk of wavevectors), of caller-owned frames and of the resident configuration:
//                    coefficients, sweep on a (walk, wavevector chunk) grid, finishing launch
//   pair_table_kernels.h (a header) the tabulated radial pair law: what TableLaw of the force sweep (rmb_sym.hip) and the TABLE
//                    instances of the energy sweep (rmb_potential.hip) share -- LDS staging, interval lookup, the two cubics;
//                    rmb_ctx_set_pair_table and the force entry points are in rmb_entry.hip
//   sym_walk.h (a header) the walk of a wave over its step range, written once (strided chunks, unit_seek at the chunk start,
//                    the [k0, k1) part of a unit, row change and flush, cull skip, unit_next): sym_kernel, sym2_kernel and
//                    sym_force_kernel are body structs under it; wave numbering (sym_wave) and wave_lds_sync
//                    for the whole family; plain arithmetic, run on the host by tests/test_sym_walk_host.py
//   lag_sweep_host.h (a header, included by the three units above) the checks of a batch of frames and of a lag / origin
//                    range, pad256, and the one launch plan of the lag sweeps (plan_lag_sweep)
#pragma once
#include "../../include/rmb_mobility.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "pair_ops.h"
#include "pair_table_kernels.h"

namespace rmbi {

// ---- errors ------------------------------------------------------------------------------------------------
int fail(int code, const std::string& msg);   // stores the message for rmb_last_error() of this thread, returns code

#define RMB_HIP(call)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return rmbi::fail(RMB_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));     \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes);
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Page-locked host memory mapped into the device's address space (the ONE place that allocates it): the host reads / writes
// `host`, kernels use `dev`.  reserve() allocates exactly `bytes` when bytes > cap (the caller passes the size it wants, slack
// included) and frees what was there, contents and all.  Nothing queued may still touch the old memory: `drain` is the stream
// to wait for before the free; without one the caller says at the call why the stream is already idle.
struct MappedBuf {
  void* host = nullptr;
  void* dev = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes, const hipStream_t* drain = nullptr);
  void release() { if (host) (void)hipHostFree(host); host = dev = nullptr; cap = 0; }
};

constexpr int kTimingRing = 8192;

// Device memory a context owns: DevBufs only, each listed in kCtxBufs (the static_assert counts them).  rmb_ctx_destroy and the
// "buffers_signature" hash that validates captured graphs walk that one list (for_each_buffer), so a buffer added here can
// neither leak nor go missing from the hash.  A DevBuf of the context belongs HERE, not among the other members of rmb_ctx.
// (The native Krylov loops' workspace behind gmres_ws is not part of it: graphs do not capture those calls.)
struct CtxBuffers {
  DevBuf pos;      // double4[n]
  DevBuf r_stage;  // raw positions staging (host entry)
  DevBuf vec, vec2, out, partial, tmp3n;
  DevBuf tile_bounds;      // bounding boxes of the 64-blob tiles (force kernel's tile culling); valid for the packed positions
  // spatially sorted copy of the configuration for the force kernel (rmb_sort.hip): valid together with tile_bounds
  DevBuf fpos, fperm, fsort_keys, fsort_vals, fsort_tmp, fsort_box;
  DevBuf pot_ws;           // potential energy (rmb_potential.hip): per-wave partial sums + the two results
  DevBuf mcmc_ws;          // single-body moves (rmb_mcmc_moves.hip): per-wave partial differences + the proposed body
  DevBuf msd_ws;           // mean-square displacement (rmb_msd.hip): body-major records + per-workgroup partial sums
  DevBuf scat_ws;          // scattering (rmb_scattering.hip): n / L of the wavevectors, series-major records, partial sums
  DevBuf vh_ws;            // van Hove self sweep (rmb_van_hove.hip): per-workgroup partial moments
  DevBuf cluster_ws;       // cluster labels (rmb_clusters.hip): the parent array of the union-find
  DevBuf hydro_ws;         // hydrodynamic function (rmb_hydro_function.hip): n / L and e6 of the wavevectors, per-chunk partial sums
  DevBuf pair_table;       // records (c0, c1, c2, c3) of the tabulated pair law (rmb_ctx_set_pair_table)
  DevBuf det_ws;           // per-unit partials of the deterministic symmetric pass
  DevBuf wave_clock;  // optional per-wave (start, end) wall-clock stamps of the symmetric kernel
  DevBuf krylov;   // partial sums of rmb_krylov_orthogonalize_device
  DevBuf symbuf;   // acc[3][n_pad] doubles for the symmetric tt kernel (kept zero between calls)
  DevBuf st[8];    // scratch of the source->target entry point
};
using CB = CtxBuffers;
constexpr DevBuf CB::* kCtxBufs[] = {&CB::pos, &CB::r_stage, &CB::vec, &CB::vec2, &CB::out, &CB::partial, &CB::tmp3n, &CB::tile_bounds,
                                     &CB::fpos, &CB::fperm, &CB::fsort_keys, &CB::fsort_vals, &CB::fsort_tmp, &CB::fsort_box,
                                     &CB::pot_ws, &CB::mcmc_ws, &CB::msd_ws, &CB::scat_ws, &CB::vh_ws, &CB::cluster_ws, &CB::hydro_ws, &CB::pair_table, &CB::det_ws, &CB::wave_clock, &CB::krylov, &CB::symbuf};      // + st[8]
static_assert(sizeof(CtxBuffers) == (sizeof(kCtxBufs) / sizeof(kCtxBufs[0]) + 8) * sizeof(DevBuf),
              "a DevBuf of CtxBuffers is missing from kCtxBufs (or st[] changed its length)");
template <class Bufs, class F>      // Bufs: CtxBuffers or const CtxBuffers (an rmb_ctx converts)
void for_each_buffer(Bufs& b, F f) {
  for (auto m : kCtxBufs) f(b.*m);
  for (auto& s : b.st) f(s);
}

}  // namespace rmbi

struct rmb_ctx : rmbi::CtxBuffers {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t stream_switch = nullptr;  // orders a newly set stream after the work queued on the previous one
  // device properties (hipDeviceProp_t): a partitioned (CPX) device or another SKU changes both
  long n_cu = 256;               // multiProcessorCount
  size_t lds_per_cu = 160 * 1024;  // maxSharedMemoryPerMultiProcessor
  // resident configuration
  long n = 0;
  double a = 0.0;
  double L[3] = {0, 0, 0};
  int wall = 0;
  int free_surface = 0;          // the configuration was loaded with wall != 0 under option "free_surface": raw heights (wall = 0 above),
                                 // kind tt is the free-surface product
  bool have_positions = false;
  long tgt_begin = 0, tgt_end = 0;
  // state of the device memory in CtxBuffers
  bool tile_bounds_valid = false;
  bool force_sorted = false;     // tile_bounds / fpos / fperm describe the SORTED configuration
  long fperm_n = -1;             // number of blobs fperm is a permutation of (force_sort_positions), -1 = none
  // (potential energy: the Morton permutation is kept and rebuilt every opt_potential_resort-th evaluation -- a Metropolis proposal moves a blob by a tenth of its radius)
  long pot_sort_age = -1;        // evaluations since the permutation was built, -1 = build it now
  // tabulated pair law (rmb_ctx_set_pair_table): K intervals of width h from r0, records in `pair_table`; K = 0: none
  long tab_k = 0;
  double tab_r0 = 0.0, tab_h = 0.0;
  long wave_clock_n = 0;
  long symbuf_zeroed_for = -1;
  void* gmres_ws = nullptr;   // workspace of the native Krylov loops (rmb_gmres.hip), freed by gmres_release
  // hand-off of the synchronous host entry point (rmb_matvec): memory the finalize kernel stores the result into directly
  // (coalesced), for results up to opt_host_zero_copy bytes, and the same for its input vectors (two of them: RMB_TT_TR)
  rmbi::MappedBuf host_out, host_in;
  // options: one member per row of the option table (kOptions, rmb_context.hip), in its order; set / read by key only there
  long opt_chunks = 0;
  long opt_timing = 0;
  long opt_symmetric = 1;      // use the symmetric (each unordered pair once) kernel where applicable
  long opt_fused_symmetric = 1;  // tt+tr: 1 = single symmetric pass (symx_kernels.h), 2 = two symmetric passes, 0 = one-sided fused sweep
  long opt_symx_single = 0;      // route tt / tr / rt / rr through the generic skeleton (A/B against sym_kernel)
  long opt_deterministic = 0;  // force the atomic-free sweep kernel everywhere
  long opt_det_workspace_mb = 8192;   // cap on the partial-result workspace of deterministic = 2 (symx_det_device)
  long opt_sym_wps = 0;        // cap on resident workgroups per CU for the symmetric kernel (0 = occupancy limit)
  long opt_sym_pin = 1;        // pad dynamic LDS so residency is exactly that number
  long opt_free_surface = 0;     // rmb_set_positions*(wall != 0) means a stress-free surface at z = 0, not a no-slip wall
  long opt_free_surface_rotation = 0;   // a free-surface configuration also serves tr / rt / rr / tt_tr and the multi-block operations
                                        // (mirror-image blocks beyond the reference; 0: refused, as the reference has none)
  long opt_precision = 64;     // 32: M_tt f (open boundaries) in single precision (sym32_kernels.h); everything else fp64
  long opt_force_precision = 0;  // blob-blob forces: 0 = follow "precision", 32 / 64 = pinned
  long opt_force_cull = 1;       // blob-blob forces: skip tile pairs beyond the range of the exponential (bit-exact)
  long opt_force_sort = 1;       // sort the blobs along a Morton curve for the force kernel's tile culling
  long opt_potential_resort = 16;   // measured: -25 % per evaluation at 1e4 blobs, -5 % at 1e5, -3 % at 262 144; 64 adds nothing
  long opt_sym_fine_steps = 0;   // floor on steps per wave when less than one resident round is left (pair shards, small N); 0 = 16 or 32, chosen in plan_sym
  long opt_sym_coop = 1;       // workgroup-cooperative symmetric kernel (sym_coop_kernels.h): 0 = never, 1 = launches of at most
                               // kCoopMaxRounds resident rounds (small suspensions, pair shards, up to ~1e4 blobs), 2 = always
  long opt_sym_chunk_steps = 1024;  // symmetric kernels: a wave's steps are cut into strided chunks of about this many (0 = one range)
  long opt_sym_two_targets = 1;   // sym2t_kernel (two target blobs per lane) for tt / tr / rt / rr, open boundaries: 0 off, 1 from one resident round on, 2 always
  long opt_host_zero_copy_in = 1;   // inputs of rmb_matvec through mapped memory + a pull kernel (sizes as host_zero_copy)
  long opt_gmres_fuse_pc = 1;       // rmb_rigid_gmres_device: the normalisation launch also applies the preconditioner for the next step
  long opt_gmres_fuse_dots = 1;     // rmb_rigid_gmres_device: the operator's finishing launch also takes the first Gram-Schmidt dots (<= 256 bodies)
  long opt_krylov_low_sync = 1;     // native GMRES / Lanczos steps: second update + norm (by Pythagoras) + normalisation in one launch
  long opt_lanczos_fuse_finish = 1; // rmb_rigid_lanczos_device, every step: finalize of the sweep + L_b^-1 product in one launch
  long opt_host_zero_copy = 768 << 10;   // bytes (32 768 blobs: level at 43 000, +1 % at 1e5); 0 = always a device-to-host copy command
  long opt_sym_order = 1;      // unit order of the symmetric kernels: 1 = blocked (32 x 32 tile super-blocks), 0 = row-major
  long opt_sym_xcd = 1;        // XCD-aware workgroup numbering (each XCD a contiguous eighth of the step range)
  long opt_sym_oversub = 8;    // launch this many times the resident workgroup count (measured: -4..8 % kernel time;
                               // waves of one SIMD finish oldest-first, more rounds keep every SIMD at >= 3 active waves)
  long opt_sym_min_steps = 64; // floor on rotation steps per wave (a unit is 64 steps)
  long opt_wave_clock = 0;     // diagnostics build only, as the next
  long opt_skip_pairs = 0;
  // timing ring (events around the sweep kernel)
  std::vector<hipEvent_t> ev0, ev1;
  int ev_count = 0;  // events recorded since last reset (capped at ring size)
  long timing_launches = 0;  // sweeps seen since the last reset (sampling stride of the "timing" option)
  // last launch
  long last_krylov_partials = 0;   // first-pass partials per basis row a finishing launch left for the last Gram-Schmidt step (0: its own dots launch ran)
  int last_path = 0;           // 0 = sweep, 1 = symmetric (per wave), 2 = deterministic symmetric, 3 = symmetric, workgroup-cooperative,
                               // 4 = symmetric, two target blobs per lane
  long last_tiles = 0, last_chunks = 0, last_wgs = 0;
  double host_us[4] = {0, 0, 0, 0};   // last rmb_matvec: upload, launch, wait + download, whole call (host wall clock, us)
};

namespace rmbi {

// ---- rmb_context.hip ---------------------------------------------------------------------------------------
int timing_begin(rmb_ctx* c, int* slot);
int timing_end(rmb_ctx* c, int slot);
int check_ready(rmb_ctx* c);
// the library's default context (stateless entry points); created on first use on the device RMB_DEVICE names (0)
extern std::mutex g_default_mu;
int default_ctx(rmb_ctx** out);   // call with g_default_mu held

// ---- rmb_gmres.hip ----------------------------------------------------------------------------------------
void gmres_release(rmb_ctx* c);
// ---- rmb_krylov.hip / rmb_rigid.hip: pieces the native GMRES composes ------------------------------------------------
// Per-body blocks (the preconditioner's four of the saddle-point system, or L_b^-T alone for the Lanczos forcing: r2 = 0,
// absent blocks with p = nullptr) and where z = blocks * v goes: handed to the Gram-Schmidt step, its LAST launch
// (normalisation, workgroup = body instead of chunk) also applies the blocks to the vector it has just normalised -- the
// next iteration's first launch.  The vector is laid out as [n_bodies x r1; n_bodies x r2].
struct BlockRef { const double* p; long bs, rs, cs; };       // one batched block: entry b at p + b * bs, element (r, c) at + r * rs + c * cs
struct PcBlocks { long n_bodies, r1, r2; BlockRef a11, a12, a21, a22; double* z; };      // square: r1 x r1, r1 x r2, r2 x r1, r2 x r2
// part1_bodies > 0: the first pass's partial dots are already there, one per body and basis row (krylov_body_partials'
// buffer, written by the operator's finishing launch): the step starts with the first update launch
int krylov_orthogonalize_impl(rmb_ctx* c, long n, long rows, const double* V_dev, long ldv, double* w_dev, double* col_dev,
                              double* v_next_dev, double* col_mapped_dev, const PcBlocks* pc, long part1_bodies = 0, bool low_sync = false);
constexpr long kKrBodyPartialsMax = 256;      // bodies up to which the finishing launch takes the first dots (every update workgroup re-sums them)
int krylov_body_partials(rmb_ctx* c, long n, double** part_out);
// the basis and where the partial dots of the vector the operator has just produced go: part[r * n_bodies + body]
struct DotsFuse { const double* V; long ldv, rows; double* part; };
int plain_tt_with_dots(rmb_ctx* c, const double* v_dev, double eta, double* out_dev, const double* V_dev, long ldv, long rows, long* tiles_done);
int rigid_operator_impl(rmb_ctx* c, long n_bodies, long n_b, const double* K_dev, const double* x_dev, double eta, double* out_dev,
                        const DotsFuse* dots, bool* dots_done);
// z_ready: z_dev already holds P^-1 v_j (the previous step's fused launch); fuse_pc: leave P^-1 v_{j+1} in z_dev
// One step of the preconditioned Lanczos forcing.  pv: P v_i (input of the sweep; pv_ready: left there by the previous step's
// fused launch), mw: the sweep's result, d: P^T M P v_i, the vector that is orthogonalised (d may be pv when fuse_next is
// false); fuse_next: the normalisation launch also leaves P v_{i+1} in pv.
int lanczos_step_impl(rmb_ctx* c, long n_bodies, long n_b, const double* Linv_dev, double* V_dev, long ldv, long i, double eta, double* pv_dev,
                      double* mw_dev, double* d_dev, double* col_dev, double* col_mapped_dev, bool pv_ready, bool fuse_next);
int arnoldi_step_impl(rmb_ctx* c, long n_bodies, long n_b, const double* A11_dev, const double* A12_dev, const double* A21_dev,
                      const double* A22_dev, const double* K_dev, double* V_dev, long ldv, long j, double eta, double* z_dev, double* w_dev,
                      double* col_dev, double* col_mapped_dev, bool z_ready, bool fuse_pc);

// ---- rmb_plan.hip ------------------------------------------------------------------------------------------
rmb::PairConsts make_pair_consts(double a);
rmb::ExpConsts exp_consts();
void choose_chunks(long n_tgt, long n_src, long forced, long slots, long* n_chunks, long* chunk_len);
int resident_blocks(const void* fn, int* cache);   // workgroups of 256 threads per CU, capped at 8
// The launch of every one-sided sweep (onesided_kernels.h): chunk plan from the residency of this instance, workspace
// of the chunk partials, bookkeeping, the sweep between the timing events, the finalize kernel when there are chunks.
// `a` comes with the operator's own fields, n_src and the target range filled in.
template <auto SWEEP, auto FINALIZE, int NOUT, class Args>
int one_sided_launch(rmb_ctx* c, Args a) {
  static int occ = 0;   // resident workgroups per CU of SWEEP
  const long n_tgt = a.tgt_end - a.tgt_begin;
  const long tiles = (n_tgt + 63) / 64;
  const long slots = c->n_cu * resident_blocks((const void*)SWEEP, &occ);
  long n_chunks, chunk_len;
  choose_chunks(n_tgt, a.n_src, c->opt_chunks, slots, &n_chunks, &chunk_len);
  if (tiles > 0x7fffffffL || n_chunks > 65535) return fail(RMB_ERR_ARG, "problem too large for one launch");
  a.n_tgt_pad = 64 * tiles;
  a.chunk_len = chunk_len;
  a.n_chunks = (int)n_chunks;
  a.partial = nullptr;
  if (n_chunks > 1) {
    if (int rc = c->partial.reserve((size_t)n_chunks * NOUT * a.n_tgt_pad * sizeof(double))) return rc;
    a.partial = (double*)c->partial.p;
  }
  c->last_path = 0; c->last_tiles = tiles; c->last_chunks = n_chunks; c->last_wgs = tiles * n_chunks;
  int slot;
  if (int rc = timing_begin(c, &slot)) return rc;
  hipLaunchKernelGGL(SWEEP, dim3((unsigned)tiles, (unsigned)n_chunks), dim3(rmb::kBlock), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  if (int rc = timing_end(c, slot)) return rc;
  if (n_chunks > 1) {
    hipLaunchKernelGGL(FINALIZE, dim3((unsigned)((n_tgt + 255) / 256)), dim3(256), 0, c->stream, a);
    RMB_HIP(hipGetLastError());
  }
  return 0;
}
// Launch plan of a symmetric sweep: `total` rotation steps over `blocks` workgroups of 4 waves.
struct SymPlan { long blocks; long steps_per_wave; size_t dyn_lds; bool sub_round; long round; };   // round: resident workgroups; sub_round: less work than that
int plan_sym(rmb_ctx* c, const void* fn, int* occ_cache, size_t static_lds, long total, bool pin, SymPlan* out,
             int declared_waves = 0, long fine_auto = 0);
// A symmetric sweep kernel as the launch path sees it: every instance, in whichever translation unit it is compiled
// (fp64 and fp32, per wave, workgroup-cooperative, two targets per lane, forces, potential), is handed over in this shape.
struct SymKernel {
  const void* fn = nullptr;   // host handle of the kernel (occupancy / attributes); nullptr = the operation has no such instance
  size_t static_lds = 0;
  int* occ = nullptr;         // cache of resident_blocks(fn)
  int waves_per_eu = 0;       // the amdgpu_waves_per_eu bound plan_sym caps the residency with (its `declared_waves`), 0 = none
  // `args` points to the argument struct of the fp64 kernel (rmb::SymArgs / Sym2Args / SymXArgs / SymForceArgs /
  // PotentialArgs); the fp32 twins convert the kernel-uniform constants `k` to float, the others ignore them
  void (*launch)(const void* args, const rmb::PairConsts& k, unsigned blocks, size_t dyn_lds, hipStream_t s) = nullptr;
  explicit operator bool() const { return fn != nullptr; }
};
template <class Args, void (*KERNEL)(Args)>
void sym_kernel_launch(const void* args, const rmb::PairConsts&, unsigned blocks, size_t dyn_lds, hipStream_t s) {
  hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(64 * rmb::kSymWaves), dyn_lds, s, *static_cast<const Args*>(args));
}
// the thunk of a kernel that takes its argument struct and nothing else (one occupancy cache per kernel)
template <class Args, void (*KERNEL)(Args)>
SymKernel sym_kernel_of(size_t static_lds, int waves_per_eu = 0) {
  static int occ = 0;
  return SymKernel{(const void*)KERNEL, static_lds, &occ, waves_per_eu, sym_kernel_launch<Args, KERNEL>};
}
// The non-pinned plan of the culling sweeps (blob-blob forces, potential energy, pair histogram): `rounds` resident rounds
// (0: "sym_oversub") capped by one workgroup per 256 steps, and a quarter of "sym_chunk_steps" per strided chunk -- the
// surviving units are few and uneven, shorter chunks balance them (3D cloud of 1e5 blobs 3.36 -> 3.05 ms, monolayer
// unchanged; tools/experiments/exp_force_ab.py).  *chunk_steps = 0: one contiguous range per wave.
// `dyn_lds` > 0: the residency is asked for with that much dynamic LDS (every time: it is the caller's number).
// `wg_pair_cap` > 0: the workgroups are doubled until the busiest one meets fewer pairs than that (64 per step and wave),
// and the plan is refused in `who`'s name if that takes more workgroups than one launch has.  Without a cap it cannot fail.
int plan_cull_sweep(rmb_ctx* c, const SymKernel& k, long total_steps, long* blocks, long* chunk_steps, long rounds = 0,
                    size_t dyn_lds = 0, double wg_pair_cap = 0.0, const char* who = "");
void shard_ranges(long n, long n_units, long shard, long nshards, long* step_begin, long* step_end, long* self_begin,
                  long* self_end);
int sym_accumulators(rmb_ctx* c, long n_pad);
// Steps per strided chunk: `spw` = steps per schedule unit (wave, or workgroup of the cooperative kernels) of a plan over
// `n_sched` units; cut into R >= 1 equal chunks of about `target` steps (exactly balanced: every unit gets R chunks).
long chunked_steps(const rmb_ctx* c, long total, long n_sched, long spw, long target);
// whether the symmetric (each unordered pair once) path applies to the resident configuration
bool sym_applies(const rmb_ctx* c);
inline double inv_length(double L) { return L > 0 ? 1.0 / L : 0.0; }   // reciprocal of a pseudo-periodic length (<= 0: open)

// ---- rmb_sym.hip -------------------------------------------------------------------------------------------
// SX_K2 + 4 (k - 2) + kind: one block on k = 2..4 vectors
// SX_FREE_*: the rotational products above a free surface (option "free_surface_rotation"): per-wave fp64 kernel only
enum SymXOp { SX_TT = 0, SX_TR, SX_RT, SX_RR, SX_FUSED, SX_GRAND, SX_COLF, SX_FREE, SX_RADII,
              SX_FREE_TR, SX_FREE_RT, SX_FREE_RR, SX_FREE_FUSED, SX_FREE_GRAND, SX_FREE_COLF, SX_K2, SX_COUNT = SX_K2 + 12 };
// Configuration a symmetric pass runs on: the context's resident one, or a caller-packed one (per-blob radii)
struct SymConf { const double4* pos; long n; double L[3]; int wall; const double* extra; };
template <class A, class = void> struct HasNPad : std::false_type {};
template <class A> struct HasNPad<A, std::void_t<decltype(A::n_pad)>> : std::true_type {};
template <class A, class = void> struct HasPrefactor : std::false_type {};
template <class A> struct HasPrefactor<A, std::void_t<decltype(A::prefactor)>> : std::true_type {};
// Fills the fields the argument structs of the symmetric sweeps share by name: configuration, tile count, unit order,
// box, and on the unit grid of the chosen kernel (`n_units`) the step range of pair shard `shard` of `nshards`; with
// global accumulators (every struct but the potential's) also n_pad / n_units / the z period; for the mobility sweeps
// (the structs with a prefactor) the self-term ownership and the kernel-uniform constants.  Call after sym_accumulators.
template <class Args>
void fill_sym_args(Args& a, const SymConf& cf, const rmb_ctx* c, double eta, long n_units, long shard, long nshards) {
  const long tiles = (cf.n + 63) / 64;
  long step_begin, step_end, self_begin, self_end;
  shard_ranges(cf.n, n_units, shard, nshards, &step_begin, &step_end, &self_begin, &self_end);
  a.pos = cf.pos;
  a.n = cf.n; a.n_tiles = (int)tiles;
  a.order = (int)c->opt_sym_order; a.xcd = (int)c->opt_sym_xcd;
  a.step_end = step_end;
  a.Lx = cf.L[0]; a.Ly = cf.L[1];
  a.iLx = inv_length(cf.L[0]); a.iLy = inv_length(cf.L[1]);
  if constexpr (HasNPad<Args>::value) {
    a.acc = (double*)c->symbuf.p;
    a.n_pad = 64 * tiles; a.n_units = n_units;
    a.step_begin = step_begin;
    a.Lz = cf.L[2]; a.iLz = inv_length(cf.L[2]);
  }
  if constexpr (HasPrefactor<Args>::value) {
    a.self_begin = self_begin; a.self_end = self_end;
    a.prefactor = 1.0 / (8.0 * M_PI * eta);
    a.k = make_pair_consts(c->a > 0.0 ? c->a : 1.0);   // unused by the per-blob-radii operation
  }
}
// The launch of every symmetric sweep: bookkeeping of the last launch (`path` = the last_path code), the wave_clock
// buffer when the argument struct has one (`wave_clock` points at its field), the sweep between the timing events,
// then the finishing kernel `fin` on `fin_blocks` workgroups of 256 (nullptr: the caller finishes the sums itself).
template <class Args>
int sym_launch(rmb_ctx* c, const SymKernel& k, int path, long blocks, size_t dyn_lds, Args& a, const rmb::PairConsts& pk,
               void (*fin)(Args), long fin_blocks, long long** wave_clock = nullptr) {
  c->last_path = path; c->last_tiles = a.n_tiles; c->last_chunks = 0; c->last_wgs = blocks;
  if (wave_clock) {
    *wave_clock = nullptr;
    if (c->opt_wave_clock) {
      // [waves][2] stamps (start, end | placement); sym2t_kernel adds a second region [waves][2] of per-wave phase totals in
      // shader-clock cycles (staging incl. its wait, everything) -- rmb_wave_clock_collect hands out both as 2 x waves rows
      c->wave_clock_n = blocks * rmb::kSymWaves * (path == 4 ? 2 : 1);
      if (int rc = c->wave_clock.reserve((size_t)2 * c->wave_clock_n * sizeof(long long))) return rc;
      *wave_clock = (long long*)c->wave_clock.p;
    }
  }
  int slot;
  if (int rc = timing_begin(c, &slot)) return rc;
  k.launch(&a, pk, (unsigned)blocks, dyn_lds, c->stream);
  RMB_HIP(hipGetLastError());
  if (int rc = timing_end(c, slot)) return rc;
  if (!fin) return 0;
  hipLaunchKernelGGL(fin, dim3((unsigned)fin_blocks), dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}
// Tile bounds of the culling sweeps (forces, potential, pair histogram): the Morton-sorted copy (rmb_sort.hip; `keep_perm`:
// along the permutation that is already there) or the bounds of the caller's order; use_tile_bounds points the arguments
// at them (and at the permutation, where the sweep wants the caller's indices).
int build_tile_bounds(rmb_ctx* c, bool sorted, bool keep_perm);
template <class A, class = void> struct HasPerm : std::false_type {};
template <class A> struct HasPerm<A, std::void_t<decltype(A::perm)>> : std::true_type {};
template <class Args>
void use_tile_bounds(const rmb_ctx* c, Args& a) {
  if (c->force_sorted) {
    a.pos = (const double4*)c->fpos.p;
    if constexpr (HasPerm<Args>::value) a.perm = (const unsigned*)c->fperm.p;
  }
  a.bounds = (const double*)c->tile_bounds.p;
}
// Resident preparation of the pair-once sweeps (pair_once_kernels.h: potential energy, pair histogram), all of it before
// the launch plan: the state and size checks in the caller's words, then spatial order and tile bounds (pair_once_resident,
// rmb_sym.hip), then the arguments the frame reads.  `reuse_perm`: the Morton permutation may be kept by the
// "potential_resort" rule; else it is rebuilt.  *empty: fewer than `n_min` points -- nothing was prepared, nothing to launch.
// The caller sets Lz / iLz (who sees the z period differs), cull2 and its own fields.
struct PairOnceErrors { const char *wall, *range, *size; };
int pair_once_resident(rmb_ctx* c, const PairOnceErrors& msg, long n_min, bool reuse_perm, bool* empty);
template <class Args>
int pair_once_prepare(rmb_ctx* c, Args& a, const PairOnceErrors& msg, long n_min, bool reuse_perm, bool* empty) {
  if (int rc = pair_once_resident(c, msg, n_min, reuse_perm, empty)) return rc;
  if (*empty) return 0;
  const long tiles = (c->n + 63) / 64;
  fill_sym_args(a, SymConf{(const double4*)c->pos.p, c->n, {c->L[0], c->L[1], c->L[2]}, 0, nullptr}, c, 0.0, tiles * (tiles + 1) / 2, 0, 1);
  a.order = 0; a.xcd = 0;      // as the force sweep (rmb_sym.hip): after culling the surviving units hug the diagonal
  if constexpr (HasPerm<Args>::value) a.perm = nullptr;
  use_tile_bounds(c, a);
  return 0;
}
// no_finalize: leave the raw sums in the accumulators (c->symbuf: [3][n_pad], unscaled, no self term) -- the caller
// launches its own finishing kernel (rmb_rigid_operator_device); not for the pseudo-periodic / fp32 routes
int sym_device(rmb_ctx* c, int kind, const double* v, double eta, double* out, long shard = 0, long nshards = 1,
               bool accumulate = false, bool no_finalize = false);
int sym2_device(rmb_ctx* c, const double* va, const double* vb, double eta, double* out_a, double* out_b, long shard = 0,
                long nshards = 1);
int symx_device(rmb_ctx* c, int op, const double* const* in, double* const* out, double eta, int in_plane, long shard,
                long nshards, int accumulate_mask = 0, const SymConf* conf_in = nullptr, bool no_finalize = false);
// the raw sums of the resident boundary's tt product left in the accumulators (sym_device / symx_device with no_finalize):
// KIND_TT, or SX_FREE on a free-surface context
int tt_raw_sums_device(rmb_ctx* c, const double* v, double eta, double* out);
int symx_det_device(rmb_ctx* c, int op, const double* const* in, double* const* out, double eta, int in_plane,
                    long shard = 0, long nshards = 1);
enum ForceLaw { FORCE_LAW_BLOB = 0, FORCE_LAW_BODY = 1, FORCE_LAW_TABLE = 2 };   // the pair law of sym_force_kernel (sym_force_kernels.h)
// the context's pair table as the kernels take it (tab_k > 0), and its reach
rmb::PairTableRef pair_table_ref(const rmb_ctx* c);
inline double pair_table_rcut(const rmb_ctx* c) { return c->tab_r0 + (double)c->tab_k * c->tab_h; }
int sym_force_device(rmb_ctx* c, double eps, double b, double blob_radius, double* out, const double* radii, long shard,
                     long nshards, ForceLaw law = FORCE_LAW_BLOB);

// ---- rmb_sort.hip ------------------------------------------------------------------------------------------
int force_sort_positions(rmb_ctx* c);
int force_regather_positions(rmb_ctx* c);   // sorted copy + tile bounds with the permutation already there

// ---- rmb_sym32.hip / rmb_symx_coop.hip / rmb_symx2t*.hip: instances compiled in translation units of their own --------
// nullptr handle when the operation has no such instance
SymKernel sym32_tt(bool wall);
SymKernel symx32(int sx, bool wall);
SymKernel sym_force32(bool radii);
SymKernel symx_coop(int sx, bool wall, bool periodic);
SymKernel symx_two_open(int sx, bool wall);
SymKernel symx_two_periodic(int sx, bool wall);

// ---- rmb_sweep.hip -----------------------------------------------------------------------------------------
int pack_positions(rmb_ctx* c, const double* r_dev, long n, double a, const double* L, int wall);
int pack_positions_radii(rmb_ctx* c, const double* r_dev, const double* rad_dev, long n, int wall, double4* dst);
int sweep_device(rmb_ctx* c, int kind, int in_plane, const double* v, const double* v2, double eta, double* out);
int force_sweep_device(rmb_ctx* c, double eps, double b, double blob_radius, double* out, const double* radii);
int add_inplace(rmb_ctx* c, double* y, const double* x, long n);
int pull_mapped(rmb_ctx* c, double* dst_dev, const double* src_mapped_dev, long n);
int body_dense_device(rmb_ctx* c, const long* first_blob_dev, long n_bodies, int n_b, double eta, double* out_dev);
int st_sweep_device(rmb_ctx* c, long ns, const double4* src_packed, const double* rad_s, const double* force, long nt,
                    const double4* tgt_packed, const double* rad_t, double eta, const double* L, int wall, double* out);
int pressure_device(rmb_ctx* c, long ns, const double* src, long nt, const double* tgt, const double* force, int wall,
                    double* out);
int double_layer_device(rmb_ctx* c, long ns, const double* src, long nt, const double* tgt, const double* normals,
                        const double* vector, const double* weights, int wall, double blob_radius, double* out);
int ubench_fp64_issue(rmb_ctx* c, int launches, double* g_wave_instr_per_s);

// ---- rmb_entry.hip (used by the multi-device engine too) ------------------------------------------------------
int matvec_device_impl(rmb_ctx* c, int kind, int in_plane, const double* v, const double* v2, double eta, double* out);
int matvec_pairshard_impl(rmb_ctx* c, int kind, int in_plane, const double* v, double eta, double* out, long shard, long nshards);
int matvec_op_impl(rmb_ctx* c, int op, int in_plane, int n_in, const double* const* in, int n_out, double* const* out,
                   double eta, long shard, long nshards);
int force_device_impl(rmb_ctx* c, double eps, double b, double blob_radius, double* out, const double* radii = nullptr,
                      long shard = 0, long nshards = 1);

}  // namespace rmbi
