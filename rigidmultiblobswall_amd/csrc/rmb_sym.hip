// rmb_sym.hip -- the symmetric (each unordered pair once, both blobs updated) fp64 sweeps: sym_kernel (tt / tr / rt / rr),
// sym2_kernel (two vectors), symx_kernel (multi-block / multi-vector operations, the deterministic variant with its
// ordered reduction) and the symmetric blob-blob force kernel.  One launch path: fill_sym_args and sym_launch
// (rmb_internal.h), and choose_sym below -- the one place where the variant of a sweep is picked.
#include "rmb_internal.h"

#include <cmath>

#include "sym_kernels.h"
#include "sym_coop_kernels.h"
#include "sym2t_kernels.h"
#include "sym2_kernels.h"
#include "sym_force_kernels.h"
#include "sym_schedule.h"
#include "symx_kernels.h"

namespace rmbi {

namespace {
SymConf conf_of(const rmb_ctx* c) {
  return SymConf{(const double4*)c->pos.p, c->n, {c->L[0], c->L[1], c->L[2]}, c->wall, nullptr};
}
bool is_periodic(const SymConf& cf) { return cf.L[0] > 0 || cf.L[1] > 0 || cf.L[2] > 0; }

// ---- the variant rule -----------------------------------------------------------------------------------------
struct SymCandidates { SymKernel plain, coop, two, f32; };   // what an operation has; all but `plain` may be absent
struct SymChoice {
  SymKernel kernel;
  SymPlan plan;
  int path;                     // the last_path code: 1 per wave, 3 workgroup-cooperative, 4 two target blobs per lane
  long n_units;                 // unit grid of the chosen kernel: tile pairs, or (row pair, tile) for two targets
  long step_begin, step_end, self_begin, self_end;     // shard_ranges on that grid
  long steps_per_wave;          // steps per strided chunk of a schedule unit ...
  bool per_workgroup;           // ... which is the WORKGROUP for the cooperative kernels, the wave otherwise
};
constexpr long kCoopMaxRounds = 4;          // sym_coop_kernel by default: launches of up to this many resident rounds
constexpr long kCoopAnySize = 1L << 40;

// Which kernel runs pair shard `shard` of `nshards` of a sweep over n blobs, and its plan.
//  * the fp32 twin when the caller hands one over ("precision" = 32), per wave, nothing else;
//  * two target blobs per lane ("sym_two_targets"; sym2t_kernels.h, symx2t_kernels.h): units are (row pair, tile) -- half
//    as many steps, two pairs per step.  From half a unit (32 steps) per resident wave on: 6000 blobs on a whole MI355X
//    (59.4 vs 60.3 us; 76.4 vs 80.4 at 7000, 97.2 vs 101.8 at 8000; below, the cooperative kernel wins: 50.7 vs 44.5 us
//    at 5000 -- tools/experiments/exp_sym2t_threshold.py); 2 = always;
//  * workgroup-cooperative ("sym_coop"; sym_coop_kernels.h, symx_coop_kernels.h): the workgroup owns the step range, its
//    four waves share one staged tile J and one flush per tile.  Below one resident round, and up to `coop_max_rounds`
//    rounds (the callers say why); 2 = always.  Steps per wave below one resident round: 8, and 4 for the smallest
//    launches (<= 12288 rotation steps, i.e. up to ~1200 blobs: 1000 blobs 8.98 -> 8.26 us; profiles/r4_coop_kernel_ab.txt);
//  * else the plain per-wave kernel.
// `pin`: plan_sym pads dynamic LDS to the planned residency.
int choose_sym(rmb_ctx* c, const SymCandidates& k, long n, long shard, long nshards, long coop_max_rounds, bool pin, SymChoice* out) {
  const long tiles = (n + 63) / 64;
  const bool f32 = (bool)k.f32;
  const auto on_grid = [&](const SymKernel& kernel, int path, long n_units, SymChoice* ch) {
    ch->kernel = kernel; ch->path = path; ch->n_units = n_units;
    shard_ranges(n, n_units, shard, nshards, &ch->step_begin, &ch->step_end, &ch->self_begin, &ch->self_end);
  };
  const auto plan = [&](SymChoice* ch, long fine) {
    return plan_sym(c, ch->kernel.fn, ch->kernel.occ, ch->kernel.static_lds, ch->step_end - ch->step_begin, pin, &ch->plan,
                    ch->kernel.waves_per_eu, fine);
  };
  SymChoice ch;
  on_grid(f32 ? k.f32 : k.plain, 1, tiles * (tiles + 1) / 2, &ch);
  if (int rc = plan(&ch, 0)) return rc;
  if (k.two && !f32 && c->opt_sym_two_targets && c->opt_sym_coop != 2 && tiles >= 4) {
    SymChoice t;
    on_grid(k.two, 4, rmb::units2_total(tiles), &t);
    if (int rc = plan(&t, 0)) return rc;
    if (!t.plan.sub_round || (t.step_end - t.step_begin) >= 32 * t.plan.round * rmb::kSymWaves || c->opt_sym_two_targets == 2) ch = t;
  }
  if (ch.path == 1 && k.coop && !f32 &&
      (c->opt_sym_coop == 2 || (c->opt_sym_coop == 1 && (ch.plan.sub_round || ch.plan.blocks <= coop_max_rounds * ch.plan.round)))) {
    ch.kernel = k.coop; ch.path = 3;
    if (int rc = plan(&ch, (ch.step_end - ch.step_begin) <= 12288 ? 4 : 8)) return rc;
  }
  const long total = ch.step_end - ch.step_begin, blocks = ch.plan.blocks;
  ch.per_workgroup = ch.path == 3;
  ch.steps_per_wave = ch.per_workgroup ? (total + blocks - 1) / blocks : ch.plan.steps_per_wave;
  ch.steps_per_wave = chunked_steps(c, total, ch.per_workgroup ? blocks : blocks * rmb::kSymWaves, ch.steps_per_wave,
                                    c->opt_sym_chunk_steps * (ch.per_workgroup ? rmb::kSymWaves : 1));
  *out = ch;
  return 0;
}

// ---- sym_kernel and its variants: [kind tt,tr,rt,rr][wall][periodic] ----------------------------------------------------
typedef void (*sym_fn)(rmb::SymArgs);
struct SymEntry { SymCandidates k; sym_fn fin; };
template <int KIND, bool WALL, bool PER> SymEntry make_sym_entry() {
  constexpr size_t lds = sizeof(double2) * rmb::kSymWaves * 64 * 3 + sizeof(double) * rmb::kSymWaves * 3 * 64;
  constexpr size_t coop_lds = sizeof(double2) * 64 * 3 + sizeof(double) * 2 * 3 * 64;
  SymEntry e{{sym_kernel_of<rmb::SymArgs, rmb::sym_kernel<KIND, WALL, PER>>(lds, rmb::kSymWavesPerEu),
              sym_kernel_of<rmb::SymArgs, rmb::sym_coop_kernel<KIND, WALL, PER>>(coop_lds, rmb::kSymWavesPerEu), SymKernel{}, SymKernel{}},
             rmb::sym_finalize_kernel<KIND, WALL>};
  // two target blobs per lane: open boundaries only (the pseudo-periodic instance is symx2t_kernel's, see sym_device)
  if constexpr (!PER) e.k.two = sym_kernel_of<rmb::SymArgs, rmb::sym2t_kernel<KIND, WALL>>(lds, rmb::kSymWavesPerEu);
  return e;
}
#define RMB_SYM_ROW(K) {{make_sym_entry<K, false, false>(), make_sym_entry<K, false, true>()}, {make_sym_entry<K, true, false>(), make_sym_entry<K, true, true>()}}
SymEntry g_sym[4][2][2] = {RMB_SYM_ROW(rmb::KIND_TT), RMB_SYM_ROW(rmb::KIND_TR), RMB_SYM_ROW(rmb::KIND_RT), RMB_SYM_ROW(rmb::KIND_RR)};
#undef RMB_SYM_ROW
}  // namespace

int sym_device(rmb_ctx* c, int kind, const double* v, double eta, double* out, long shard, long nshards, bool accumulate,
               bool no_finalize) {
  const SymConf cf = conf_of(c);
  const bool periodic = is_periodic(cf);
  const SymEntry& se = g_sym[kind][c->wall ? 1 : 0][periodic ? 1 : 0];
  const long n = c->n;
  if (int rc = sym_accumulators(c, 64 * ((n + 63) / 64))) return rc;
  if (periodic && no_finalize) return fail(RMB_ERR_STATE, "sym_device: no_finalize is for open boundaries (internal)");
  SymCandidates k = se.k;
  // Pseudo-periodic single-vector products: their two-targets-per-lane kernel is an instance of the generic skeleton
  // (symx2t_kernels.h: one record read and one set of LDS adds for the 2 x 3^d image pairs of a step).  Where the rule
  // picks it the product is handed over to symx_device, which picks it again; smaller launches stay here (cooperative
  // kernel).  The wave_clock diagnostic lives in sym_kernel / sym2t_kernel: no hand-over and no cooperative kernel then.
  if (periodic && !c->opt_wave_clock) k.two = symx_two_periodic(SX_TT + kind, c->wall != 0);
  if (c->opt_wave_clock) k.coop = SymKernel{};
  // single-precision mode (mobility_pycuda.py:7-19 `precision = 'single'`): tt with open boundaries only
  if (c->opt_precision == 32 && kind == RMB_TT && !periodic) {
    if (c->opt_wave_clock || c->opt_skip_pairs)
      return fail(RMB_ERR_STATE, "the \"wave_clock\" / \"skip_pairs\" diagnostics exist in the fp64 kernels only: set \"precision\" = 64");
    k.f32 = sym32_tt(c->wall != 0);
  }
  // The cooperative kernel is faster below one resident round (1/8 pair shard of 1e4 blobs 29.6 -> 25.0 us, 1000 blobs
  // 10.4 -> 9.0 us), the same time up to a few rounds with HALF the atomic flush traffic (1e4 blobs: WRITE_SIZE
  // 54.4 -> 27.4 MB per launch, 146.7 vs 147.8 us), 0.5-1 % slower at >= 8 rounds (profiles/r4_coop_kernel_ab.txt)
  SymChoice ch;
  if (int rc = choose_sym(c, k, n, shard, nshards, kCoopMaxRounds, true, &ch)) return rc;
  if (periodic && ch.path == 4) {
    const double* in[2] = {v, nullptr};
    double* outs[1] = {out};
    return symx_device(c, SX_TT + kind, in, outs, eta, 0, shard, nshards, accumulate ? 1 : 0);
  }
  rmb::SymArgs a;
  fill_sym_args(a, cf, c, eta, ch.n_units, shard, nshards);
  a.vec = v;
  a.out = out;
  a.steps_per_wave = ch.steps_per_wave;
  a.skip_pairs = (int)c->opt_skip_pairs;
  a.accumulate = accumulate ? 1 : 0;
  // no_finalize: the caller finishes the accumulators itself
  return sym_launch(c, ch.kernel, ch.path, ch.plan.blocks, ch.plan.dyn_lds, a, a.k, no_finalize ? nullptr : se.fin, (n + 255) / 256,
                    &a.wave_clock);
}

// Two source vectors, one pass over the unordered pairs (sym2_kernels.h): one target per lane, per wave, no pinned LDS.
int sym2_device(rmb_ctx* c, const double* va, const double* vb, double eta, double* out_a, double* out_b, long shard,
                long nshards) {
  const SymConf cf = conf_of(c);
  const bool periodic = is_periodic(cf);
  const long n = c->n;
  if (int rc = sym_accumulators(c, 64 * ((n + 63) / 64))) return rc;
  typedef rmb::Sym2Args A;
  const SymKernel k = c->wall ? (periodic ? sym_kernel_of<A, rmb::sym2_kernel<true, true>>(0, rmb::kSymWavesPerEu)
                                          : sym_kernel_of<A, rmb::sym2_kernel<true, false>>(0, rmb::kSymWavesPerEu))
                              : (periodic ? sym_kernel_of<A, rmb::sym2_kernel<false, true>>(0, rmb::kSymWavesPerEu)
                                          : sym_kernel_of<A, rmb::sym2_kernel<false, false>>(0, rmb::kSymWavesPerEu));
  SymChoice ch;
  if (int rc = choose_sym(c, SymCandidates{k, SymKernel{}, SymKernel{}, SymKernel{}}, n, shard, nshards, 0, false, &ch)) return rc;
  A a;
  fill_sym_args(a, cf, c, eta, ch.n_units, shard, nshards);
  a.vec_a = va; a.vec_b = vb;
  a.out_a = out_a; a.out_b = out_b;
  a.steps_per_wave = ch.steps_per_wave;
  return sym_launch(c, k, ch.path, ch.plan.blocks, ch.plan.dyn_lds, a, a.k,
                    c->wall ? rmb::sym2_finalize_kernel<true> : rmb::sym2_finalize_kernel<false>, (n + 255) / 256);
}

// ---- generic symmetric operations (symx_kernels.h) ---------------------------------------------------------
namespace {
typedef void (*symx_fn)(rmb::SymXArgs);
typedef void (*symx_combine_fn)(const rmb::SymXArgs, int);
struct SymXEntry { SymKernel sweep; symx_fn fin; int n_in, n_out; symx_fn det_sweep; symx_fn det_reduce; symx_combine_fn det_combine; int det_occ; };
template <class OP, bool WALL, bool PER> SymXEntry make_symx_entry() {
  return SymXEntry{sym_kernel_of<rmb::SymXArgs, rmb::symx_kernel<OP, WALL, PER, false>>(
                       sizeof(double2) * rmb::kSymWaves * 64 * rmb::SymXRec<OP::NIN, rmb::SymXExtra<OP>::value>::d2 +
                       sizeof(double) * rmb::kSymWaves * 3 * OP::NOUT * 64),
                   rmb::symx_finalize_kernel<OP, WALL>, OP::NIN, OP::NOUT, rmb::symx_kernel<OP, WALL, PER, true>,
                   rmb::symx_det_reduce_kernel<OP::NOUT>, rmb::symx_det_combine_kernel<OP::NOUT>, 0};
}
// [op][wall][periodic]
#define RMB_SX_ROW(OP) {{make_symx_entry<OP, false, false>(), make_symx_entry<OP, false, true>()}, {make_symx_entry<OP, true, false>(), make_symx_entry<OP, true, true>()}}
SymXEntry g_symx[SX_COUNT][2][2] = {
    RMB_SX_ROW(rmb::OpSingle<rmb::KIND_TT>), RMB_SX_ROW(rmb::OpSingle<rmb::KIND_TR>), RMB_SX_ROW(rmb::OpSingle<rmb::KIND_RT>),
    RMB_SX_ROW(rmb::OpSingle<rmb::KIND_RR>), RMB_SX_ROW(rmb::OpFusedRow), RMB_SX_ROW(rmb::OpGrand), RMB_SX_ROW(rmb::OpColumnF),
    // the free-surface operation takes raw heights: only the wall = 0 column is ever launched
    {{make_symx_entry<rmb::OpFreeSurface, false, false>(), make_symx_entry<rmb::OpFreeSurface, false, true>()},
     {make_symx_entry<rmb::OpFreeSurface, false, false>(), make_symx_entry<rmb::OpFreeSurface, false, true>()}},
    RMB_SX_ROW(rmb::OpRadiiTT),
    // rotational free-surface operations: raw heights as well, per-wave kernel only (symx_coop / symx_two_* / symx32 have none)
#define RMB_SX_RAW(OP) {{make_symx_entry<OP, false, false>(), make_symx_entry<OP, false, true>()}, {make_symx_entry<OP, false, false>(), make_symx_entry<OP, false, true>()}}
    RMB_SX_RAW(rmb::OpFreeTR), RMB_SX_RAW(rmb::OpFreeRT), RMB_SX_RAW(rmb::OpFreeRR), RMB_SX_RAW(rmb::OpFreeFusedRow),
    RMB_SX_RAW(rmb::OpFreeGrand), RMB_SX_RAW(rmb::OpFreeColumnF),
#undef RMB_SX_RAW
#define RMB_SX_K(K) RMB_SX_ROW(RMB_SX_KIND(rmb::KIND_TT, K)), RMB_SX_ROW(RMB_SX_KIND(rmb::KIND_TR, K)), \
                    RMB_SX_ROW(RMB_SX_KIND(rmb::KIND_RT, K)), RMB_SX_ROW(RMB_SX_KIND(rmb::KIND_RR, K))
#define RMB_SX_KIND(KIND, K) rmb::OpKindK<KIND, K>
    RMB_SX_K(2), RMB_SX_K(3), RMB_SX_K(4)};
#undef RMB_SX_K
#undef RMB_SX_KIND
#undef RMB_SX_ROW


// the argument fields of a generic operation that are not the shared ones
void fill_symx_io(rmb::SymXArgs& a, const SymXEntry& se, const SymConf& cf, const double* const* in, double* const* out, int in_plane) {
  a.extra = cf.extra;
  for (int v = 0; v < 4; ++v) { a.in[v] = v < se.n_in ? in[v] : nullptr; a.out[v] = v < se.n_out ? out[v] : nullptr; }
  a.in_plane = in_plane ? 1 : 0;
}
}  // namespace

int symx_device(rmb_ctx* c, int op, const double* const* in, double* const* out, double eta, int in_plane, long shard,
                long nshards, int accumulate_mask, const SymConf* conf_in, bool no_finalize) {
  const SymConf cf = conf_in ? *conf_in : conf_of(c);
  const bool periodic = is_periodic(cf);
  const SymXEntry& se = g_symx[op][cf.wall ? 1 : 0][periodic ? 1 : 0];
  const long n = cf.n;
  if (int rc = sym_accumulators(c, 64 * ((n + 63) / 64))) return rc;
  if (periodic && no_finalize) return fail(RMB_ERR_STATE, "symx_device: no_finalize is for open boundaries (internal)");
  // Two target blobs per lane (symx2t_kernels.h): fused row, grand, force column, one block on two vectors, and every
  // pseudo-periodic single-vector product.
  SymCandidates k{se.sweep, symx_coop(op, cf.wall != 0, periodic),
                  periodic ? symx_two_periodic(op, cf.wall != 0) : symx_two_open(op, cf.wall != 0), SymKernel{}};
  // "precision" = 32: the operation's single-precision twin where it has one (open boundaries)
  if (c->opt_precision == 32 && !periodic) k.f32 = symx32(op, cf.wall != 0);
  if (k.f32 && c->opt_skip_pairs)
    return fail(RMB_ERR_STATE, "the \"skip_pairs\" diagnostic exists in the fp64 kernels only: set \"precision\" = 64");
  // Workgroup-cooperative instance (symx_coop_kernels.h).  Measured (profiles/r4_coop_kernel_ab.txt): faster below one
  // resident round (pair shards, small suspensions); for the three-vector passes at every size (their per-wave slabs,
  // 47 KB per workgroup, hold residency at three workgroups per CU where the registers allow four: -7 % at 1e4 blobs,
  // -1.6 % at 1e5); no gain for the other operations above one round, and 2-7 % SLOWER for four vectors at 1e5 blobs
  // (those passes are bound by the LDS pipe itself -- 20 LDS instructions per step -- and a third wave per SIMD only
  // adds contention).
  const bool three_vectors = op >= SX_K2 + 4 && op < SX_K2 + 8;
  SymChoice ch;
  if (int rc = choose_sym(c, k, n, shard, nshards, three_vectors ? kCoopAnySize : 0, true, &ch)) return rc;
  rmb::SymXArgs a;
  fill_sym_args(a, cf, c, eta, ch.n_units, shard, nshards);
  fill_symx_io(a, se, cf, in, out, in_plane);
  a.steps_per_wave = ch.steps_per_wave;
  a.accumulate = accumulate_mask;
  a.skip_pairs = (int)c->opt_skip_pairs;
  // no_finalize: the caller finishes the accumulators itself (as sym_device)
  return sym_launch(c, ch.kernel, ch.path, ch.plan.blocks, ch.plan.dyn_lds, a, a.k, no_finalize ? nullptr : se.fin, (n + 255) / 256);
}

int tt_raw_sums_device(rmb_ctx* c, const double* v, double eta, double* out) {
  if (!c->free_surface) return sym_device(c, rmb::KIND_TT, v, eta, out, 0, 1, false, true);
  const double* in[2] = {v, nullptr};
  double* outs[1] = {out};
  return symx_device(c, SX_FREE, in, outs, eta, 0, 0, 1, 0, nullptr, true);
}

// Deterministic symmetric pass ("deterministic" = 2): same pair arithmetic as symx_device, but whole units per wave and
// per-unit partial results in a bounded workspace instead of atomics, summed in a fixed order by
// symx_det_reduce_kernel; the unit list is processed in chunks that fit the workspace ("det_workspace_mb").
// Pair shard `shard` of `nshards`: whole units [n_units shard / nshards, n_units (shard + 1) / nshards) -- the fixed order
// then holds per rank, and a G-rank run is bit-reproducible as long as the all-reduce is (same ranks, same algorithm).
int symx_det_device(rmb_ctx* c, int op, const double* const* in, double* const* out, double eta, int in_plane,
                    long shard, long nshards) {
  const SymConf cf = conf_of(c);
  SymXEntry& se = g_symx[op][c->wall ? 1 : 0][is_periodic(cf) ? 1 : 0];
  const long n = c->n, tiles = (n + 63) / 64;
  if (int rc = sym_accumulators(c, 64 * tiles)) return rc;
  rmb::SymXArgs a;
  fill_sym_args(a, cf, c, eta, tiles * (tiles + 1) / 2, shard, nshards);     // the step range is set per chunk below
  fill_symx_io(a, se, cf, in, out, in_plane);
  a.order = 0; a.xcd = 0;        // the ordered reduction enumerates the units row-major
  const long shard_ub = (long)((__int128)a.n_units * shard / nshards), shard_ue = (long)((__int128)a.n_units * (shard + 1) / nshards);
  a.accumulate = 0;
  a.skip_pairs = 0;
  // Chunk = as many units as the workspace holds; whole units per wave, as many waves PER CHUNK LAUNCH as `sym_oversub`
  // resident rounds (so that every chunk fills the chip), never less than one unit each.
  const int wps = resident_blocks((const void*)se.det_sweep, &se.det_occ);
  const long max_waves = c->n_cu * wps * rmb::kSymWaves * c->opt_sym_oversub;
  const size_t slot = (size_t)3 * se.n_out * 64 * sizeof(double);
  long chunk_units = (long)(((size_t)c->opt_det_workspace_mb << 20) / (2 * slot));
  if (chunk_units > shard_ue - shard_ub) chunk_units = shard_ue - shard_ub;
  if (chunk_units < 1) chunk_units = 1;
  const long upw = (chunk_units + max_waves - 1) / max_waves;
  chunk_units = ((chunk_units + upw - 1) / upw) * upw;
  // slices per tile in the ordered reduction: enough workgroups to fill the chip when there are few tiles
  long segs = (4 * c->n_cu + tiles - 1) / tiles;
  if (segs > 32) segs = 32;
  if (segs < 1) segs = 1;
  if (int rc = c->det_ws.reserve((size_t)2 * chunk_units * slot + (size_t)tiles * segs * slot)) return rc;
  a.part_I = (double*)c->det_ws.p;
  a.part_J = a.part_I + chunk_units * (3L * se.n_out * 64);
  a.det_seg = a.part_J + chunk_units * (3L * se.n_out * 64);
  a.units_per_wave = upw;
  a.steps_per_wave = 64 * upw;
  c->last_path = 2; c->last_tiles = tiles; c->last_chunks = 0; c->last_wgs = 0;
  for (long ub = shard_ub; ub < shard_ue; ub += chunk_units) {
    const long ue = ub + chunk_units < shard_ue ? ub + chunk_units : shard_ue;
    a.unit_begin = ub; a.unit_end = ue;
    a.step_begin = 64 * ub; a.step_end = 64 * ue;
    a.first_chunk = ub == shard_ub ? 1 : 0;
    const long waves = (ue - ub + upw - 1) / upw;
    const long blocks = (waves + rmb::kSymWaves - 1) / rmb::kSymWaves;
    c->last_wgs += blocks;
    int slot_t;
    if (int rc = timing_begin(c, &slot_t)) return rc;
    hipLaunchKernelGGL(se.det_sweep, dim3((unsigned)blocks), dim3(64 * rmb::kSymWaves), 0, c->stream, a);
    RMB_HIP(hipGetLastError());
    hipLaunchKernelGGL(se.det_reduce, dim3((unsigned)tiles, (unsigned)segs), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(se.det_combine, dim3((unsigned)tiles), dim3(256), 0, c->stream, a, (int)segs);
    RMB_HIP(hipGetLastError());
    if (int rc = timing_end(c, slot_t)) return rc;
  }
  hipLaunchKernelGGL(se.fin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
  RMB_HIP(hipGetLastError());
  return 0;
}

int build_tile_bounds(rmb_ctx* c, bool sorted, bool keep_perm) {
  if (sorted) return keep_perm ? force_regather_positions(c) : force_sort_positions(c);
  const long tiles = (c->n + 63) / 64;
  if (int rc = c->tile_bounds.reserve((size_t)6 * tiles * sizeof(double))) return rc;
  hipLaunchKernelGGL(rmb::tile_bounds_kernel, dim3((unsigned)tiles), dim3(64), 0, c->stream, (const double4*)c->pos.p, c->n,
                     (double*)c->tile_bounds.p);
  RMB_HIP(hipGetLastError());
  return 0;
}

int pair_once_resident(rmb_ctx* c, const PairOnceErrors& msg, long n_min, bool reuse_perm, bool* empty) {
  if (c->wall) return fail(RMB_ERR_STATE, msg.wall);
  if (c->tgt_begin != 0 || c->tgt_end != c->n) return fail(RMB_ERR_STATE, msg.range);
  const long n = c->n, tiles = (n + 63) / 64;
  if (n > 0xffffffffL) return fail(RMB_ERR_ARG, msg.size);
  RMB_HIP(hipSetDevice(c->device));
  *empty = n < n_min;
  if (*empty) return 0;
  // Spatial order and tile bounds.  The bounds are recomputed for every evaluation (the culling is correct for ANY
  // order); the Morton permutation is rebuilt, or with `reuse_perm` kept and rebuilt on every "potential_resort"-th evaluation.
  const bool sorted = c->opt_force_sort && tiles >= 32;
  bool rebuild = true;
  if (sorted && reuse_perm) rebuild = c->fperm_n != n || c->pot_sort_age < 0 || c->pot_sort_age + 1 >= c->opt_potential_resort;
  if (int rc = build_tile_bounds(c, sorted, !rebuild)) return rc;
  if (sorted) c->pot_sort_age = rebuild ? 0 : c->pot_sort_age + 1;
  // What the force path finds (sym_force_device): after a full sort, or bounds in the caller's order, exactly what it would have
  // built itself for this configuration -- it may use them; a sorted copy along a REUSED permutation is correct too, but
  // not the order the forces alone would sum in, so the force path is told to build its own.
  c->tile_bounds_valid = rebuild;
  c->force_sorted = sorted;
  return 0;
}

// Symmetric pair-force sweep (sym_force_kernels.h: each unordered pair once, F_ji = -F_ij) of pair shard `shard` of
// `nshards` into a full-length result; atomic flushes.  Tile culling and the fp32 twin as the options say.
// `law`: the blob-blob contact law, or the body-body Yukawa law on the resident points (FORCE_LAW_BODY: fp64 only, no
// contact distance -- blob_radius and radii are not read), or the context's tabulated law on them (FORCE_LAW_TABLE: the
// same, eps and b are not read either; reach r_cut, records staged in tab_k * 32 bytes of dynamic LDS).
rmb::PairTableRef pair_table_ref(const rmb_ctx* c) {
  const double rc = pair_table_rcut(c);
  return rmb::PairTableRef{(const double4*)c->pair_table.p, (int)c->tab_k, c->tab_r0, 1.0 / c->tab_h, (double)c->tab_k, rc * rc};
}

int sym_force_device(rmb_ctx* c, double eps, double b, double blob_radius, double* out, const double* radii, long shard,
                     long nshards, ForceLaw law) {
  const bool table = law == FORCE_LAW_TABLE;
  const bool body = law == FORCE_LAW_BODY;
  if (body || table) { blob_radius = 0.0; radii = nullptr; }
  if (table) { eps = 0.0; b = 1.0; }
  const SymConf cf = conf_of(c);
  const bool periodic = is_periodic(cf);
  const long n = c->n, tiles = (n + 63) / 64;
  if (int rc = sym_accumulators(c, 64 * tiles)) return rc;
  rmb::SymForceArgs a;
  fill_sym_args(a, cf, c, 0.0, tiles * (tiles + 1) / 2, shard, nshards);
  a.out = out;
  // Row-major units and plain workgroup numbering, whatever "sym_order" / "sym_xcd" say: with tile culling most units cost
  // nothing and the ones that do sit next to the diagonal (after the Morton sort), so the blocked order hands neighbouring
  // waves equally heavy runs of super-block rows; measured 3.37 vs 5.01 ms on a 3D cloud of 1e5 blobs, 2.39 vs 2.64 ms on
  // the 262 144-roller monolayer (tools/experiments/exp_force_ab.py).  The strided chunks stay.
  a.order = 0; a.xcd = 0;
  a.eps = eps; a.eps_over_b = eps / b; a.inv_b = 1.0 / b; a.two_a = 2.0 * blob_radius;
  a.ec = exp_consts();
  a.radii = radii;
  a.tab = table ? pair_table_ref(c) : rmb::PairTableRef{};
  // "precision" = 32, open boundaries: the single-precision kernel -- the arithmetic of the reference's own GPU force
  // kernel (forces_pycuda.py:14-21)
  const bool f32 = !body && !table && (c->opt_force_precision ? c->opt_force_precision : c->opt_precision) == 32 && !periodic;
  // Tile culling: the force has the range of its exponential.  exp(-(r - 2a)/b) is exactly 0 in double precision
  // beyond (r - 2a)/b = 745.2 (750 here; 110 for the float kernel), so a tile pair whose bounding boxes are further
  // apart contributes nothing, bit for bit.  In a 262 144-roller monolayer that is 99 % of the tile pairs -- the
  // reference's own answer to this is a k-d tree (`blob_blob_force_implementation tree_numba`).  The Yukawa law between
  // body locations has the same range with 2a = 0: exp(-r/b) is exactly 0 beyond r = 750 b.
  a.bounds = nullptr; a.cull2 = 0.0; a.perm = nullptr;
  if (c->opt_force_cull && !radii && tiles > 1) {
    // Spatial order first ("force_sort"): how much the culling skips depends on how compact a 64-blob tile is, i.e. on
    // the order in which the caller lists the blobs; from 32 tiles on the blobs are sorted along a Morton curve once
    // per configuration (rmb_sort.hip) and the kernel runs on the sorted copy.
    const bool want_sorted = c->opt_force_sort && tiles >= 32;
    if (!c->tile_bounds_valid || c->force_sorted != want_sorted) {
      if (int rc = build_tile_bounds(c, want_sorted, false)) return rc;
      c->force_sorted = want_sorted;
      c->tile_bounds_valid = true;
    }
    use_tile_bounds(c, a);
    const double reach = 2.0 * blob_radius + (f32 ? 110.0 : 750.0) * b;
    a.cull2 = table ? a.tab.rcut2 : reach * reach;      // the table is exactly zero from r_cut on
  }
  typedef rmb::SymForceArgs A;
  const size_t dyn_lds = table ? (size_t)c->tab_k * sizeof(double4) : 0;
  const SymKernel k = table ? (periodic ? sym_kernel_of<A, rmb::sym_force_kernel<true, false, rmb::TableLaw>>(0)
                                        : sym_kernel_of<A, rmb::sym_force_kernel<false, false, rmb::TableLaw>>(0))
                      : body ? (periodic ? sym_kernel_of<A, rmb::sym_force_kernel<true, false, rmb::BodyYukawaLaw>>(0)
                                       : sym_kernel_of<A, rmb::sym_force_kernel<false, false, rmb::BodyYukawaLaw>>(0))
                      : f32 ? sym_force32(radii != nullptr)
                          : radii ? (periodic ? sym_kernel_of<A, rmb::sym_force_kernel<true, true>>(0) : sym_kernel_of<A, rmb::sym_force_kernel<false, true>>(0))
                                  : (periodic ? sym_kernel_of<A, rmb::sym_force_kernel<true, false>>(0) : sym_kernel_of<A, rmb::sym_force_kernel<false, false>>(0));
  long blocks;
  plan_cull_sweep(c, k, a.step_end - a.step_begin, &blocks, &a.chunk_steps, 0, dyn_lds);
  return sym_launch(c, k, 1, blocks, dyn_lds, a, rmb::PairConsts{}, rmb::sym_force_finalize_kernel, (n + 255) / 256);
}

}  // namespace rmbi
