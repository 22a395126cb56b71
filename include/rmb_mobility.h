/*
 * rmb_mobility.h -- C ABI of the MI355X blob-mobility engine (librmb_mobility.so).
 *
 * This is the drop-in boundary for the reference's blob-level pairwise operators.  The reference
 * reaches its GPU backend through Python wrappers that allocate, upload, launch and download on
 * every call (mobility/mobility_pycuda.py:2235-2267 and siblings; multi_bodies/forces_pycuda.py:
 * 148-180).  Here the same operators are exported as plain-C entry points (pointers + sizes, no
 * torch / numpy types) that a ctypes / cffi / pybind stub can bind; INTEGRATION.md shows the stub.
 *
 * All matrices are never formed: every entry point computes  out = M(kind) . vec  (or the pair
 * forces) by an O(N^2) sweep in fp64 on the device.
 *
 * Conventions
 *   - positions, vectors, outputs: double, C-contiguous (N,3) row-major == flat 3N, exactly the
 *     layout the reference wrappers pass (mobility/mobility_numba.py:132-134).
 *   - `L` = periodic_length[3]; a component <= 0 means open in that direction; > 0 means
 *     pseudo-periodic (nearest image + the 3^d first neighbour boxes, mobility_numba.py:140-197).
 *   - `wall` != 0 selects the single-wall kernels AND the wrapper-level regularisation of the
 *     reference: z_eff = max(z, a) (mobility.py:52-64) and u = B M(z_eff) B v with
 *     B_ii = z_i/a for z_i < a (mobility.py:67-84, :1150-1163).  wall == 0: unbounded RPY, no clamp
 *     (mobility.py:1119-1129).
 *   - free surface: with context option "free_surface" = 1, `wall` != 0 in rmb_set_positions* means a
 *     stress-free surface at z = 0 instead of a no-slip wall (raw heights, no clamp, no B).  On such a
 *     configuration RMB_TT is the free-surface product (RMB_TT_FREE_SURFACE), the dense per-body blocks
 *     and the rigid-body operator / Arnoldi / Lanczos / GMRES entry points carry the image of
 *     mobility_numba.py:1840-1926; tr / rt / rr / tt_tr, in_plane, the two-vector pass and every
 *     rmb_op but RMB_OP_TT_MULTI (one sweep per vector) return RMB_ERR_STATE: the reference has no
 *     rotational products above a free surface.  (An option, not wall == 2: every non-zero `wall` has
 *     always meant the no-slip wall here.)
 *   - rotational products above a free surface, BEYOND the reference: with context option
 *     "free_surface_rotation" = 1 (default 0: everything above stays as stated) a free-surface
 *     configuration also serves RMB_TR / RMB_RT / RMB_RR / RMB_TT_TR, RMB_OP_VELOCITY_FROM_FORCE_TORQUE,
 *     RMB_OP_GRAND, RMB_OP_FORCE_COLUMN, RMB_OP_{TR,RT,RR}_MULTI (one sweep per vector), their pair shards and
 *     rmb_lanczos_device(product = grand).  The blocks are those of the mirror-image system of the unbounded
 *     RPY tensors B_xx: the image of blob j sits at S r_j, S = diag(1, 1, -1); a force is a polar vector and
 *     mirrors as S f, a torque is an axial one and mirrors as -S tau, so with R = (d_x, d_y, z_i + z_j)
 *       M_tt = B_tt(d) + B_tt(R) S    M_tr = B_tr(d) - B_tr(R) S    M_rt = B_rt(d) + B_rt(R) S    M_rr = B_rr(d) - B_rr(R) S
 *     (overlap patches included; i == j: the unbounded self term plus the blob's own image at R = (0, 0, 2 z_i)).
 *     The 6N matrix is symmetric, and positive definite with open boundaries.  Double precision only
 *     ("precision" = 32 with one of these products returns RMB_ERR_STATE), periodic_length[2] must be 0, no
 *     in_plane variant, no two-vector pass: each refused with RMB_ERR_STATE, nothing else runs in their place.
 *   - every function returns 0 on success, a negative rmb_status otherwise; rmb_last_error()
 *     gives a message for the calling thread.  The reference defines no error codes (failures
 *     surface as Python exceptions from pycuda); the Python shim raises RuntimeError on non-zero.
 *   - host entry points are synchronous (result complete on return), as the reference's are.
 *     *_device entry points enqueue on the context's stream and return immediately.
 */
#ifndef RMB_MOBILITY_H
#define RMB_MOBILITY_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rmb_ctx rmb_ctx;

enum rmb_status {
  RMB_OK = 0,
  RMB_ERR_ARG = -1,      /* null pointer, bad kind, negative size ...            */
  RMB_ERR_STATE = -2,    /* matvec before set_positions, bad target range ...    */
  RMB_ERR_HIP = -3,      /* a HIP runtime call failed (message has the HIP text) */
  RMB_ERR_NO_DEVICE = -4 /* no gfx950 device visible                             */
};

/* Which block of the grand mobility.  Each row names the reference function it replaces
 * (numba CPU twin / pycuda GPU twin, both in mobility/):
 *   TT     mobility_numba.py:124 (wall) :13 (no wall)   / mobility_pycuda.py:150, :371
 *   TR     mobility_numba.py:548        :440            / mobility_pycuda.py:1516, :1733
 *   RT     mobility_numba.py:938        :832            / mobility_pycuda.py:926, :1034
 *   RR     mobility_numba.py:1189       :1077           / mobility_pycuda.py:593, :703
 *   TT_TR  fused u = M_tt f + M_tr tau, pycuda only     / mobility_pycuda.py:1266, :1394
 *   TT_FREE_SURFACE  u = [RPY(d) + RPY(image) P] f above a stress-free surface at z = 0
 *          mobility_numba.py:1770 / mobility_pycuda.py:2081; needs set_positions(wall = 0)   */
enum rmb_kind { RMB_TT = 0, RMB_TR = 1, RMB_RT = 2, RMB_RR = 3, RMB_TT_TR = 4, RMB_TT_FREE_SURFACE = 5 };

/* ---- library / device ------------------------------------------------------------------- */
const char* rmb_version(void);
const char* rmb_last_error(void);
int rmb_device_count(void);

/* ---- persistent context: positions stay resident across the matvecs of one solve ----------
 * (GMRES / Lanczos call M.f many times with fixed r_vectors, multi_bodies.py:445, :599;
 *  the reference re-uploads positions on every call.) */
/* device: index into the visible devices, or -1 = the default device: the environment variable RMB_DEVICE when it
 * is set (an index; anything else -> RMB_ERR_ARG), else 0. */
int rmb_ctx_create(int device, rmb_ctx** ctx);
int rmb_ctx_destroy(rmb_ctx* ctx);
/* hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream); NULL = default stream.
 * A context is SINGLE-STREAM at a time (its accumulators, workspaces and packed positions are re-used from call to
 * call): when the handle changes, the new stream is made to wait (event) for everything already queued on the
 * previous one.  Unchanged handle: no cost.
 * LIFETIME: the stream a context is bound to must be alive while calls are enqueued on it AND at the moment the
 * handle is changed (the switch records an event on it; HIP does not validate stream handles, a destroyed one is a
 * use-after-free).  A host that destroys its streams (one stream per time step, say) calls rmb_ctx_release_stream()
 * before hipStreamDestroy: it waits for the context's work on that stream and forgets the handle (the context is then
 * on the default stream until the next rmb_ctx_set_stream).  If the record on the previous stream fails with an error
 * code, the switch falls back to a device-wide synchronisation and adopts the new handle all the same: a context
 * never stays bound to a stream it could not fence. */
int rmb_ctx_set_stream(rmb_ctx* ctx, void* hip_stream);
int rmb_ctx_release_stream(rmb_ctx* ctx);
/* Options (unknown key -> RMB_ERR_ARG).  Defaults in [].  The keys, what a set value is stored as (as given, clamped,
 * 0 / 1, or refused) and the members behind them are ONE table: kOptions in csrc/rmb_context.hip, defaults in the option
 * block of rmb_ctx (csrc/rmb_internal.h).
 *   "timing"          [0]  n >= 1 = bracket every n-th pair-sweep launch with HIP events (rmb_timing_collect); an
 *                          event pair serialises ~4-8 us around the launch, so throughput runs sample (n = 4)
 *   "symmetric"       [1]  1 = evaluate each unordered pair once and update both blobs (sym_kernels.h /
 *                          symx_kernels.h) whenever the full target range is resident and n >= 128;
 *                          0 = always the one-sided sweep (every ordered pair, atomic-free)
 *   "deterministic"   [0]  bit-reproducible results (for a given N and device).  1 = the one-sided sweep (every
 *                          ordered pair, fixed summation order, no workspace; ~1.5x the default time);
 *                          2 = the symmetric pass with per-unit partials summed in a fixed order instead of
 *                          atomics (1.06-1.18x; workspace min(0.19 N^2 B, "det_workspace_mb")).  Pair shards
 *                          (nshards > 1) honour 2 -- a shard is then a range of WHOLE tile pairs, so a G-rank run
 *                          is bit-reproducible whenever its all-reduce is -- and ignore 1 (a slice of the unordered
 *                          pairs has no one-sided form).  Forces: 1 and 2 both take the one-sided sweep.
 *   "precision"       [64] 32 = single precision on the default symmetric path with open boundaries (the
 *                          reference's `precision = 'single'` build, mobility_pycuda.py:7-19) for tt / tr / rt / rr,
 *                          RMB_TT_TR, RMB_TT_FREE_SURFACE, the in-plane products, the grand / force-column / k-vector operations and the
 *                          blob-blob forces (the reference's GPU force kernel is always single precision,
 *                          forces_pycuda.py:14-21) (sym32_kernels.h, symx32_kernels.h): pair arithmetic in fp32
 *                          (~1e-6 relative, separations from a head / tail split of the fp64 positions), partial sums,
 *                          self terms and scaling in fp64; 1.5-1.6x faster.
 *                          Pseudo-periodic domains, the one-sided sweep, the deterministic modes,
 *                           the per-blob-radii product with sources != targets, pair shards of tr / rt / rr and
 *                          the source->target operators compute in fp64 whatever this says.  Other values:
 *                          RMB_ERR_ARG.  The "wave_clock" / "skip_pairs" diagnostics exist in the fp64 kernels only:
 *                          a product that would run an fp32 kernel with one of them set returns RMB_ERR_STATE.
 *   "free_surface"    [0]  `wall` != 0 in the next rmb_set_positions* loads a configuration above a stress-free surface
 *                          at z = 0 (conventions above)
 *   "free_surface_rotation" [0]  1 = a free-surface configuration also serves the rotational blocks of the mirror-image
 *                          system (a force mirrors as S f, a torque as -S tau; conventions above).  Beyond the reference;
 *                          fp64 per-wave symmetric kernel from 128 blobs on, the one-sided sweep below / for target
 *                          sub-ranges / "deterministic" = 1.  0 = those products return RMB_ERR_STATE
 *   "force_cull"      [1]  blob-blob forces (uniform radius, symmetric path; open or pseudo-periodic): skip tile pairs whose
 *                          bounding boxes are further apart than 2a + 750 b, where exp(-(r - 2a)/b) underflows to
 *                          exactly 0 in double precision (110 b for the float kernel): no bit of the result changes
 *   "force_sort"      [1]  with "force_cull", from 2048 blobs on: sort the blobs along a Morton curve once per configuration
 *                          (on the device) and run the force kernel on the sorted copy, results written back to the caller's
 *                          indices -- the culling then skips the same tile pairs whatever order the caller lists the blobs in
 *                          (262 144 rollers listed at random: 48 -> 4 ms).  Same pair terms in another summation order:
 *                          equal to rounding; 0 = keep the caller's order
 *   "potential_resort" [16] rmb_blob_potential: rebuild the Morton permutation on every K-th evaluation and reuse it in
 *                          between (see there)
 *   "force_precision" [0]  blob-blob forces: 0 = follow "precision", 32 / 64 = pinned whatever "precision" says
 *                          (products in single precision with double-precision forces, or the reverse)
 *   "det_workspace_mb" [8192]  workspace of mode 2; the unit list is processed in chunks that fit
 *   "fused_symmetric" [1]  RMB_TT_TR: 1 = one symmetric pass sharing the pair geometry between both blocks,
 *                          2 = two symmetric passes (tt, then tr accumulated), 0 = the one-sided fused sweep
 *   "symx_single"     [0]  1 = run tt / tr / rt / rr (and the two-vector product) through the generic multi-block
 *                          skeleton instead of the dedicated kernels (A/B measurements)
 *   "chunks"          [0]  one-sided sweep: number of source chunks (blockIdx.y); 0 = chosen from the occupancy
 *   "sym_oversub"     [8]  symmetric kernels: launch up to this many times the resident workgroup count
 *   "sym_min_steps"   [64] symmetric kernels: floor on rotation steps per wave (one tile pair = 64 steps)
 *   "sym_fine_steps"  [0]  symmetric kernels: floor on rotation steps per wave when the launch is smaller than one
 *                          resident round (small suspensions, one rank's pair shard); 0 = 16 while 16-step waves do
 *                          not fill the chip, 32 beyond
 *   "sym_coop"        [1]  tt / tr / rt / rr on the dedicated symmetric kernel: the workgroup-cooperative variant
 *                          (the four waves of a workgroup share one staged tile and one flush per tile instead of each
 *                          staging and flushing its own): 0 = never, 1 = launches of at most four resident rounds of
 *                          workgroups (small suspensions, one rank's pair shard, products up to ~1e4 blobs: faster below
 *                          one round, same time with half the atomic flush traffic up to four), 2 = always
 *   "sym_two_targets" [1]  tt / tr / rt / rr with open boundaries: two target blobs per lane (sym2t_kernels.h: a lane keeps
 *                          blob `lane` of two tile rows, so one record read and one set of LDS adds serve two pairs; +3-4.5 %
 *                          from 1e4 to 1e6 blobs, half the atomic flush traffic): 0 = never, 1 = launches of at least half a
 *                          resident round of workgroups (~6000 blobs; smaller ones stay with the cooperative kernel), 2 = always
 *   "sym_order"       [1]  symmetric kernels: order in which the tile pairs are visited: 1 = blocked (super-blocks of 32 x 32
 *                          tiles, so that neighbouring step ranges re-use the same 64 tiles), 0 = row-major over the tile
 *                          triangle.  The deterministic symmetric mode always runs row-major
 *   "sym_xcd"         [1]  symmetric kernels: XCD-aware workgroup numbering -- every XCD (own L2) gets one contiguous eighth
 *                          of the step range; with "sym_order" = 1 the tile loads of a launch mostly hit L2 (HBM fetch
 *                          traffic / 10 at >= 1e5 blobs; the kernels are VALU-bound, so time moves little)
 *   "sym_chunk_steps" [1024]  symmetric kernels: a wave's share of the rotation steps is cut into equal strided chunks of about
 *                          this many steps (wave w takes chunks w, w + W, w + 2 W, ...), so that the waves running at the same
 *                          time work on neighbouring tile pairs at any problem size; 0 = one contiguous range per wave
 *   "gmres_fuse_pc"   [1]  rmb_rigid_gmres_device: the last launch of an Arnoldi step (normalisation, workgroup = body) also applies
 *                          the block-diagonal preconditioner to the vector it has just normalised, so every step but the first
 *                          of a restart cycle is six launches instead of seven; 0 = separate launches (same arithmetic)
 *                          Also governs rmb_rigid_lanczos_device (its normalisation launch applies L_b^-T for the next step)
 *   "gmres_fuse_dots" [1]  rmb_rigid_gmres_device, decks of up to 256 bodies: the operator's finishing launch (workgroup = body) also
 *                          takes the first Gram-Schmidt pass's dots of its slices with every basis row (one partial per body, summed
 *                          by the first update launch): five launches per iteration; 0 = a separate dots launch.  The Lanczos
 *                          step's finishing launch ("lanczos_fuse_finish") does the same
 *   "krylov_low_sync" [1]  steps of the native GMRES / Lanczos entries: the launch that subtracts the second Gram-Schmidt projection
 *                          also normalises, with |w2|^2 = |w1|^2 - |h2|^2 from partials of the first update launch (orthonormal
 *                          basis; h2 is rounding-sized): one launch less per iteration; 0 = separate norm / normalisation launch
 *   "lanczos_fuse_finish" [1]  rmb_rigid_lanczos_device: the sweep leaves its raw sums and ONE
 *                          launch (workgroup = body) finishes them and multiplies by L_b^-1; 0 = finalize and block product as
 *                          two launches (same arithmetic)
 *   "sym_wps"         [0]  symmetric kernels: cap on resident workgroups per CU (0 = occupancy limit)
 *   "sym_pin"         [1]  symmetric kernels: pad dynamic LDS so that residency is exactly that number
 *   "wave_clock"      [0]  1 = stamp every wave's start / end (rmb_wave_clock_collect); schedule diagnostics
 *   "skip_pairs"      [0]  diagnostics, results are WRONG: bit 0 = no pair arithmetic, bit 1 = no flush of the
 *                          per-wave LDS accumulators (tools/experiments/exp_prewarm.py prices the atomics with it)          */
int rmb_ctx_set_option(rmb_ctx* ctx, const char* key, long value);
/* Current value of an option (same keys, same table); lets a caller switch one temporarily and restore what was there.  Read-only
 * key "last_path": the kernel family of the last product (0 one-sided sweep, 1 symmetric per wave, 2 deterministic
 * symmetric, 3 symmetric workgroup-cooperative, 4 symmetric with two target blobs per lane).  Read-only key
 * "last_krylov_partials": the first-pass partials per basis row that a finishing launch left for the last Gram-Schmidt step
 * (the body count, or the count of 64-blob tiles for the plain Lanczos step); 0 = the step ran its own dots launch. */
int rmb_ctx_get_option(rmb_ctx* ctx, const char* key, long* value);

/* Upload / pack positions: fuses shift_heights + damping_matrix_B (mobility.py:52-84).
 * r: (n,3).  The *_device variant reads a device pointer and is asynchronous. */
int rmb_set_positions(rmb_ctx* ctx, const double* r_host, long n, double a, const double* L, int wall);
int rmb_set_positions_device(rmb_ctx* ctx, const double* r_dev, long n, double a, const double* L, int wall);

/* Multi-GPU: this context only produces targets [begin, end) of the n blobs (all n are sources).
 * Default after set_positions is [0, n).  Output arrays then hold 3*(end-begin) doubles. */
int rmb_set_target_range(rmb_ctx* ctx, long begin, long end);

/* out = M(kind) . vec.  vec2 = torque for RMB_TT_TR, NULL otherwise.  in_plane != 0 gives the
 * in_plane_* variants (mobility_numba.py:291, :690; only meaningful for TT / TR with a wall).
 * vec/vec2: 3n doubles (all sources); out: 3*(end-begin) doubles. */
int rmb_matvec(rmb_ctx* ctx, int kind, int in_plane, const double* vec_host, const double* vec2_host,
               double eta, double* out_host);
int rmb_matvec_device(rmb_ctx* ctx, int kind, int in_plane, const double* vec_dev, const double* vec2_dev,
                      double eta, double* out_dev);

/* Multi-GPU, symmetric pair sharding (RMB_TT / TR / RT / RR / TT_FREE_SURFACE): the unordered blob pairs are cut into
 * `nshards` equal parts; this call evaluates part `shard` (each pair once, applied to both blobs) and
 * writes its contribution to ALL n targets (3n doubles).  The sum over shards is the full product; the
 * self term of target i is added by the shard that owns i in the contiguous block partition.  The
 * caller all-reduces (or reduce-scatters) the outputs.  No reference counterpart (single device). */
int rmb_matvec_pairshard_device(rmb_ctx* ctx, int kind, const double* vec_dev, double eta, double* out_dev,
                                long shard, long nshards);
/* Two source vectors in ONE pass over the pairs (tt only): out_a = M vec_a, out_b = M vec_b.  The vector-independent
 * part of every pair (geometry, both inverse square roots, RPY and wall coefficients) is evaluated once, so the call
 * costs ~0.66 of two rmb_matvec_device calls.  Serves solvers that advance two right-hand sides in lockstep with the
 * same mobility (the Brownian-slip and RFD solves of quaternion_integrator_multi_bodies.py:985-996).  Falls back to two
 * single products where the symmetric kernel does not apply (n < 128, "deterministic", target sub-ranges); a pair
 * shard (nshards > 1) always runs the symmetric kernel, for any n. */
int rmb_matvec2_device(rmb_ctx* ctx, int kind, const double* vec_a_dev, const double* vec_b_dev, double eta,
                       double* out_a_dev, double* out_b_dev);
int rmb_matvec2_pairshard_device(rmb_ctx* ctx, int kind, const double* vec_a_dev, const double* vec_b_dev, double eta,
                                 double* out_a_dev, double* out_b_dev, long shard, long nshards);

/* Several blocks of the grand mobility from ONE pass over the unordered pairs: differences, both inverse square
 * roots, the wall polynomials and the heights are evaluated once per pair and shared by all blocks.
 *   RMB_OP_VELOCITY_FROM_FORCE_TORQUE  in: f, tau   out: u = M_tt f + M_tr tau          (= RMB_TT_TR;
 *       mobility_pycuda.py:1266-1391 / :1394-1512)
 *   RMB_OP_GRAND                       in: f, tau   out: u, w = [[M_tt, M_tr], [M_rt, M_rr]] [f; tau]
 *       (quaternion_integrator/quaternion_integrator_rollers.py:1114-1121 applies the four blocks separately)
 *   RMB_OP_FORCE_COLUMN                in: f        out: u = M_tt f, w = M_rt f   (the two random-finite-difference
 *       products of one draw, quaternion_integrator_rollers.py:1138-1160)
 *   RMB_OP_TT_MULTI (TR_ / RT_ / RR_)  in: k vectors (1..4)   out: the block applied to each (solves and Lanczos
 *       recursions advanced in lockstep on the same configuration: geometry and coefficients once per pair)
 * in_dev / out_dev: arrays of n_in / n_out device pointers to 3n doubles (3*(end-begin) for outputs under a target
 * range).  in_plane != 0 zeroes the z component of every input and output (mobility_numba.py:291, :690).
 * Wall / no-wall / pseudo-periodic follow rmb_set_positions.  The *_pairshard variant evaluates pair shard `shard`
 * of `nshards` into full-length partial outputs (sum over shards = product), as rmb_matvec_pairshard_device. */
enum rmb_op { RMB_OP_VELOCITY_FROM_FORCE_TORQUE = 0, RMB_OP_GRAND = 1, RMB_OP_FORCE_COLUMN = 2, RMB_OP_TT_MULTI = 3,
              RMB_OP_TR_MULTI = 4, RMB_OP_RT_MULTI = 5, RMB_OP_RR_MULTI = 6 };
int rmb_matvec_op_device(rmb_ctx* ctx, int op, int in_plane, int n_in, const double* const* in_dev, int n_out,
                         double* const* out_dev, double eta);
int rmb_matvec_op_pairshard_device(rmb_ctx* ctx, int op, int in_plane, int n_in, const double* const* in_dev, int n_out,
                                   double* const* out_dev, double eta, long shard, long nshards);

/* Dense translation-translation mobility of each rigid body's own blobs (building block of the
 * block-diagonal preconditioner, multi_bodies/multi_bodies.py:516-531; replaces body/body.py:186-191 ->
 * mobility/mobility.py:1018-1116 / :967-1013 called once per body in Python).  All listed bodies have
 * n_b contiguous blobs starting at first_blob[k]; out[k] is the (3 n_b x 3 n_b) row-major block
 * B M(z_eff) B of body k.  Device pointers, asynchronous.  Non-periodic. */
int rmb_body_mobility_dense_device(rmb_ctx* ctx, const long* first_blob_dev, long n_bodies, int n_b, double eta,
                                   double* out_dev);

/* The O(N) pieces of the rigid-body saddle-point solve that sit between two sweeps (csrc/rmb_krylov.hip).  Device
 * pointers, asynchronous on the context's stream, no positions needed, every reduction in a fixed order.
 *
 * rmb_block_apply_device: for every batch entry b (a rigid body)
 *     y1_b = beta1 y1_b + alpha (A11_b x1_b + A12_b x2_b)       y1_b: r1 values at y1 + b r1,  x1_b: c1 values at x1 + b c1
 *     y2_b = beta2 y2_b + alpha (A21_b x1_b + A22_b x2_b)       y2_b: r2 values at y2 + b r2,  x2_b: c2 values at x2 + b c2
 * in ONE launch.  A block is addressed as p[b batch_stride + row row_stride + col col_stride] (a transposed block is
 * the same memory with the two strides exchanged); a NULL rmb_block* or p == NULL is a zero block; beta == 0 does not
 * read y.  x and y must not overlap.  c1 + c2 + r1 + r2 <= 8192.  Replaces the four batched products of the block-diagonal
 * preconditioner (multi_bodies/multi_bodies.py:548-560: A = the blocks of [[M, -K], [-K^T, 0]]^-1 per body) and the
 * K U / K^T lambda products of the operator (multi_bodies/multi_bodies.py:327-375 called from :424-471).
 *
 * rmb_krylov_orthogonalize_device: one Arnoldi step's orthogonalisation against the `rows` basis vectors V[0..rows)
 * (row r at V + r ldv, n values), two passes of classical Gram-Schmidt:
 *     h = V w;  w -= V^T h;  h2 = V w;  w -= V^T h2;   col[0..rows) = h + h2,  col[rows] = |w|,  v_next = w / |w|
 * (w is overwritten with the orthogonalised, un-normalised vector; |w| == 0 leaves inf / nan in v_next, as the division
 * would: test col[rows]).  rows <= 256.  Four launches; what scipy.sparse.linalg.gmres does internally for the
 * reference (general_application_utils.py:608-627). */
/* Per-body geometry and the per-body factors of the block-diagonal preconditioner, one launch each (csrc/rmb_rigid.hip).
 * Bodies of one call have n_b blobs each, stored body after body.
 *
 * rmb_rigid_configuration_device: r = R(q) ref + x for every blob (body/body.py:64-78; rotation matrix of the unit
 * quaternion (s, p) as quaternion_integrator/quaternion.py:41-51), the body-frame offsets rel = R(q) ref and
 * K = [I, -(rel x)] per blob (body/body.py:81-115).  ref (n_bodies, n_b, 3), loc (n_bodies, 3), quat (n_bodies, 4),
 * r (n_bodies n_b, 3), rel (n_bodies, n_b, 3) or NULL, K (n_bodies, 3 n_b, 6) row-major or NULL.
 *
 * rmb_rigid_preconditioner_device: from each body's dense blob mobility Mb (n_bodies, 3 n_b, 3 n_b; symmetrised on
 * load; rmb_body_mobility_dense_device builds it) and K: Lchol (Mb = L L^T, lower, zeros above), Linv = L^-1,
 * Minv = Mb^-1, Nbody = (K^T Mb^-1 K)^-1 (6 x 6), and the blocks of [[Mb, -K], [-K^T, 0]]^-1:
 *   A12 = -Mb^-1 K N (3 n_b x 6), A11 = Mb^-1 + A12 (Mb^-1 K)^T, A21 = A12^T (6 x 3 n_b), A22 = -N
 * (multi_bodies/multi_bodies.py:516-531 builds L and N, :548-560 applies them).  *info_dev (one int, device) is set to
 * 0 and then to 1 by any body whose Mb is not positive definite or whose 6 x 6 resistance K^T Mb^-1 K has no accurate
 * inverse (single blobs, collinear rods: the reference takes the pseudo-inverse there, the caller must too).
 * n_b <= 42, i.e. the reference's 12- and 42-blob shells (one workgroup per body, the factors of a body live in LDS: two
 * n x n matrices up to 16 blobs, ONE matrix worked on in place -- Cholesky, triangular inverse, M^-1 formed on the way out --
 * from 17 to 42 blobs: 126 x 126 doubles = 127 KB of the 160 KB).
 *
 * rmb_rigid_advance_device: loc_out = loc + U[:, 0:3] dt, quat_out = quaternion(U[:, 3:6] dt) * quat for every body
 * (quaternion_integrator/quaternion_integrator_multi_bodies.py:86-91; quaternion.py:17-39: the rotation quaternion is
 * (cos |phi|/2, sin(|phi|/2) phi / |phi|), multiplied from the LEFT).  U (n_bodies, 6); dt_body_dev: NULL, or one step
 * per body that replaces dt (the random finite difference scales the displacement by the body length).  Outputs may
 * alias the inputs. */
/* The rigid-body saddle-point operator in one call (multi_bodies/multi_bodies.py:424-471, all bodies free, one body shape):
 *   out[0 .. 3N)        = M_tt lambda - K U          (N = n_bodies n_b blobs, lambda = x[0 .. 3N), U = x[3N .. 3N + 6 n_bodies))
 *   out[3N .. 3N + 6nb) = -K^T lambda
 * on the context's resident configuration (n = n_bodies n_b).  K (n_bodies, 3 n_b, 6) row-major as
 * rmb_rigid_configuration_device writes it.  With the symmetric kernels (open boundaries, double precision, default
 * modes) this is the pair sweep + ONE finishing launch (workgroup = body: self term, scaling, - K U, and -K^T lambda by
 * a reduction over the body's blobs); otherwise the product and the two K products as separate launches, same result. */
int rmb_rigid_operator_device(rmb_ctx* ctx, long n_bodies, long n_b, const double* K_dev, const double* x_dev, double eta,
                              double* out_dev);
/* One Arnoldi step of the right-preconditioned GMRES of the rigid-body problem (quaternion_integrator_multi_bodies.py:
 * 1441-1547 -> general_application_utils.py:608-627; all bodies free, one body shape), enqueued by ONE call:
 *   z = P^-1 v_j   (the four blocks of rmb_rigid_preconditioner_device, one launch),
 *   w = [M z_lambda - K z_U; -K^T z_lambda]   (rmb_rigid_operator_device: pair sweep + one finishing launch),
 *   two classical Gram-Schmidt passes of w against v_0 .. v_j, column j of the Hessenberg matrix to col_dev[0 .. j + 1]
 *   (and to col_mapped_dev when not NULL), |w| to col_dev[j + 1], v_{j+1} = w / |w|   (rmb_krylov_orthogonalize2_device).
 * V_dev: (restart + 1) rows of ldv doubles, n = 3 n_bodies n_b + 6 n_bodies unknowns each; z_dev, w_dev: n doubles of
 * scratch.  Seven launches from one host call, no copy command -- what a small deck's iteration costs is the number of
 * launches (~4.5 us each however little they do) and of host calls, not their work (profiles/r5_gmres_step.txt). */
int rmb_rigid_arnoldi_step_device(rmb_ctx* ctx, long n_bodies, long n_b, const double* A11_dev, const double* A12_dev,
                                  const double* A21_dev, const double* A22_dev, const double* K_dev, double* V_dev, long ldv, long j,
                                  double eta, double* z_dev, double* w_dev, double* col_dev, double* col_mapped_dev);
/* Single steps in the forms the native loops below run, for the step-level tests (tests/test_gpu_krylov.py): each entry
 * enqueues the launches of ONE iteration and returns -- no loop, no wait.
 * rmb_rigid_arnoldi_step2_device: the step above with the loop's two flags.  z_ready != 0: z_dev already holds P^-1 v_j (the
 *   previous step's last launch left it there), the block launch is skipped; fuse_pc != 0: the Gram-Schmidt ending also writes
 *   z_dev = P^-1 v_{j+1}, and -- with the symmetric sweep, option gmres_fuse_dots and up to 256 bodies -- the operator's
 *   finishing launch takes the first pass's dots as one partial per body.  The ending is the low-synchronisation one (option
 *   krylov_low_sync, on by default).
 * rmb_rigid_lanczos_step_device: one iteration of rmb_rigid_lanczos_device: pv = P v_i (skipped when pv_ready != 0), mw = the
 *   sweep's result, d = P^T M pv orthogonalised in place against v_0 .. v_i, h_ii and h_{i+1,i} in col[i], col[i + 1],
 *   v_{i+1} = row i + 1 of V; fuse_next != 0: the ending also leaves P v_{i+1} in pv_dev (d_dev must then differ from pv_dev).
 * rmb_lanczos_step_device: one iteration of rmb_lanczos_device: x1 = M v_i (product, in_plane as there; 3 N doubles, 6 N for
 *   the grand mobility), orthogonalised in place, column and v_{i+1} as above.  V_dev: rows of ldv >= 3 N (6 N) doubles. */
int rmb_rigid_arnoldi_step2_device(rmb_ctx* ctx, long n_bodies, long n_b, const double* A11_dev, const double* A12_dev,
                                   const double* A21_dev, const double* A22_dev, const double* K_dev, double* V_dev, long ldv, long j,
                                   double eta, double* z_dev, double* w_dev, double* col_dev, double* col_mapped_dev, int z_ready,
                                   int fuse_pc);
int rmb_rigid_lanczos_step_device(rmb_ctx* ctx, long n_bodies, long n_b, const double* Linv_dev, double* V_dev, long ldv, long i,
                                  double eta, double* pv_dev, double* mw_dev, double* d_dev, double* col_dev, double* col_mapped_dev,
                                  int pv_ready, int fuse_next);
int rmb_lanczos_step_device(rmb_ctx* ctx, int product, int in_plane, double* V_dev, long ldv, long i, double eta, double* x1_dev,
                            double* col_dev, double* col_mapped_dev);
/* The whole right-preconditioned GMRES(restart) of [[M, -K], [-K^T, 0]] x = b (quaternion_integrator_multi_bodies.py:1441-1547
 * -> general_application_utils.py:608-627 -> scipy; all bodies free, one body shape) as ONE call: per iteration one
 * rmb_rigid_arnoldi_step_device and an event; the Givens rotations and the convergence test run on the host INSIDE the
 * library, one iteration behind the device, on the Hessenberg column the Gram-Schmidt kernel stored into mapped host
 * memory.  Stops when |b - A x| <= tol |b| by the rotated residual (scipy's tol, atol = 0), on an exact breakdown, or
 * after maxiter INNER iterations; the true residual is formed at every restart.  b_dev: n = 3 n_bodies n_b + 6 n_bodies
 * doubles (the caller normalises it as the reference does, :1518-1521); x_dev: the solution P^-1 y.  *iterations, *residual
 * (relative), *discarded (steps enqueued for nothing: at most one per restart cycle), *products (operator applications),
 * history[0 .. min(iterations, history_cap)) = the relative residual after every iteration (NULL: not wanted).
 * rhs_norm: NULL = b_dev is used as given; otherwise b_dev is the RAW right-hand side: it is scaled to unit norm inside,
 * the solution scaled back, and *rhs_norm = |b| (0: x = 0, no iteration).
 * Synchronous: returns when x_dev is enqueued on the context's stream and every scalar is final. */
int rmb_rigid_gmres_device(rmb_ctx* ctx, long n_bodies, long n_b, const double* A11_dev, const double* A12_dev, const double* A21_dev,
                           const double* A22_dev, const double* K_dev, const double* b_dev, double tol, long restart, long maxiter,
                           double eta, double* x_dev, long* iterations, double* residual, long* discarded, long* products,
                           double* history, long history_cap, double* rhs_norm);
/* The whole preconditioned Lanczos forcing  noise = factor * blockdiag(L_b) (P^T M P)^{1/2} z,  P = blockdiag(L_b^-T), of the
 * Brownian rigid-body schemes (quaternion_integrator_multi_bodies.py:966-973 -> stochastic_forcing/stochastic_forcing.py:112-264
 * with the preconditioner of multi_bodies.py:590-614; covariance factor^2 M) as ONE call.  Per iteration i one step and an
 * event:
 *   y = P v_i,  w = M_tt y,  w <- P^T w   (two block launches around the pair sweep),
 *   two classical Gram-Schmidt passes of w against v_0 .. v_i, which also store h_ii and h_{i+1,i} into mapped host
 *   memory, v_{i+1} = w / |w|;
 * the small tridiagonal eigenproblem (QL sweeps inside the library) and the reference's stopping rule (:239-255: relative
 * change of the noise estimate below tol) run on the host one iteration behind the device.
 * Linv_dev / Lchol_dev: (n_bodies, 3 n_b, 3 n_b) contiguous factors of the body mobilities
 * (rmb_rigid_preconditioner_device); z_dev: 3 N standard normals; noise_dev: 3 N doubles out; max_rows: basis vectors the
 * workspace may hold (2 .. 254).  *status: 0 = noise_dev written, *iterations as the reference counts them; 1 = exact
 * breakdown / eigen-solve failure, 2 = more than max_rows basis vectors needed -- then nothing is written, the stream is
 * drained and the caller runs its general loop.  *products = pair sweeps enqueued (iterations + 1, + 1 discarded).
 * Returns when noise_dev is enqueued on the context's stream and every scalar is final. */
int rmb_rigid_lanczos_device(rmb_ctx* ctx, long n_bodies, long n_b, const double* Linv_dev, const double* Lchol_dev,
                             const double* z_dev, double factor, double tol, long max_iter, long max_rows, double eta,
                             double* noise_dev, long* iterations, long* products, int* status);
/* The unpreconditioned forcing of the single-blob (roller) schemes as one call, same loop:  noise = factor * M^{1/2} z  with
 * product 0: M = M_tt over 3 N unknowns (in_plane != 0: its in-plane variant), product 1: the 6 N x 6 N grand mobility
 * [[M_tt, M_tr], [M_rt, M_rr]], z = [z_f; z_tau] (quaternion_integrator_rollers.py:1082-1121, :1203-1260, :1315-1353 ->
 * stochastic_forcing_lanczos without preconditioner: 40-50 iterations at tol 1e-6).  Arguments and status as above. */
int rmb_lanczos_device(rmb_ctx* ctx, int product, int in_plane, const double* z_dev, double factor, double tol, long max_iter,
                       long max_rows, double eta, double* noise_dev, long* iterations, long* products, int* status);
/* HOST function, no GPU work: coef = scale * Q sqrt(max(lambda, 0)) Q^T e_1 of the k x k symmetric tridiagonal matrix with
 * diagonal h_diag[0 .. k) and off-diagonal h_sup[0 .. k-1) -- the coordinates of the Lanczos noise estimate in the Krylov
 * basis after k iterations (stochastic_forcing.py:215-229), as rmb_rigid_lanczos_device computes them. */
int rmb_lanczos_noise_coefficients(long k, const double* h_diag, const double* h_sup, double scale, double* coef_out);
int rmb_rigid_configuration_device(rmb_ctx* ctx, long n_bodies, long n_b, const double* ref_dev, const double* loc_dev,
                                   const double* quat_dev, double* r_dev, double* rel_dev, double* K_dev);
int rmb_rigid_advance_device(rmb_ctx* ctx, long n_bodies, const double* loc_dev, const double* quat_dev, const double* U_dev,
                             double dt, const double* dt_body_dev, double* loc_out_dev, double* quat_out_dev);
int rmb_rigid_preconditioner_device(rmb_ctx* ctx, long n_bodies, long n_b, const double* Mb_dev, const double* K_dev,
                                    double* Lchol_dev, double* Linv_dev, double* Minv_dev, double* Nbody_dev, double* A11_dev,
                                    double* A12_dev, double* A21_dev, double* A22_dev, int* info_dev);

typedef struct rmb_block { const double* p; long batch_stride, row_stride, col_stride; } rmb_block;
int rmb_block_apply_device(rmb_ctx* ctx, long n_batch, long r1, long c1, long r2, long c2, const rmb_block* a11,
                           const rmb_block* a12, const rmb_block* a21, const rmb_block* a22, const double* x1_dev,
                           const double* x2_dev, double alpha, double beta1, double* y1_dev, double beta2, double* y2_dev);
int rmb_krylov_orthogonalize_device(rmb_ctx* ctx, long n, long rows, const double* V_dev, long ldv, double* w_dev,
                                    double* col_dev, double* v_next_dev);
/* The same step with the new column written once more to col_mapped_dev (rows + 1 doubles of page-locked, device-mapped
 * host memory from rmb_host_mapped_alloc; NULL = rmb_krylov_orthogonalize_device): the host reads it after one event wait,
 * no copy command. */
int rmb_krylov_orthogonalize2_device(rmb_ctx* ctx, long n, long rows, const double* V_dev, long ldv, double* w_dev,
                                     double* col_dev, double* v_next_dev, double* col_mapped_dev);
/* Any form of the Gram-Schmidt ending on caller-chosen V and w.  low_sync != 0 (and option krylov_low_sync): three launches,
 * the last one subtracts the second projection, takes |w| = sqrt(|w1|^2 - |h2|^2) and normalises; otherwise the four launches
 * above.  z_dev != NULL: the vector is laid out as [n_bodies x r1; n_bodies x r2], n_bodies (r1 + r2) = n, and the last launch
 * (workgroup = body) also writes z = blocks * v_next: z1_b = A11_b v1_b + A12_b v2_b, z2_b = A21_b v1_b + A22_b v2_b with the
 * square blocks addressed as in rmb_block_apply_device (NULL = zero block).  z_dev == NULL: the body arguments are ignored. */
int rmb_krylov_orthogonalize3_device(rmb_ctx* ctx, long n, long rows, const double* V_dev, long ldv, double* w_dev,
                                     double* col_dev, double* v_next_dev, double* col_mapped_dev, int low_sync, long n_bodies,
                                     long r1, long r2, const rmb_block* a11, const rmb_block* a12, const rmb_block* a21,
                                     const rmb_block* a22, double* z_dev);
/* The two vector launches of the native loops: y[e] += sum_{i < k} coef[i] V[i][e] for e < n (k <= 256; coef_dev: k doubles the
 * device can read, mapped host memory in the loops), and *out_dev = |v| over n doubles (one workgroup, fixed order). */
int rmb_krylov_lincomb_device(rmb_ctx* ctx, double* y_dev, const double* V_dev, long ldv, const double* coef_dev, long k, long n);
int rmb_krylov_norm_device(rmb_ctx* ctx, const double* v_dev, long n, double* out_dev);
/* Page-locked host memory mapped into the device's address space (hipHostMallocMapped), zero-filled: *host = the address
 * the host reads / writes, *dev = the address kernels use.  Freed with rmb_host_mapped_free(host). */
int rmb_host_mapped_alloc(size_t bytes, void** host, void** dev);
int rmb_host_mapped_free(void* host);

/* Blob-blob soft repulsion on the resident positions (multi_bodies/forces_numba.py:12-55,
 * forces_pycuda.py:66-118): out (n_targets,3).  Uses the UNCLAMPED positions: call
 * rmb_set_positions with wall = 0 first (the reference passes raw r_vectors). */
int rmb_blob_blob_force(rmb_ctx* ctx, double repulsion_strength, double debye_length, double blob_radius,
                        double* out_host);
int rmb_blob_blob_force_device(rmb_ctx* ctx, double repulsion_strength, double debye_length,
                               double blob_radius, double* out_dev);
/* Body-body forces (multi_bodies/multi_bodies_functions.py:359-408, `body_body_force_torque_implementation python`): a
 * Yukawa repulsion U = eps exp(-r/b) / r between the resident points, which the caller sets to the body LOCATIONS
 * (rmb_set_positions with wall = 0; wall = 1 or a target sub-range: RMB_ERR_STATE).  out (n,3):
 *   F_i = sum_j -(eps/b + eps/r) exp(-r/b) (x_j - x_i) / r^2,  r = |x_j - x_i| in the minimal image of every direction
 * with a positive period (all three, as project_to_periodic_image).  The torque of the reference's law is zero and is not
 * returned.  Each unordered pair once on the symmetric force sweep, always fp64 ("force_precision" / "precision" do not
 * apply; atomic flushes whatever "deterministic" says); "force_cull" (tile pairs beyond 750 b: exact zeros) and
 * "force_sort" apply.  Coincident points divide by zero as in the reference: those points get non-finite forces, the
 * others are not affected.  debye_length <= 0 or a null pointer: RMB_ERR_ARG. */
int rmb_body_body_force(rmb_ctx* ctx, double repulsion_strength, double debye_length, double* out_host);
int rmb_body_body_force_device(rmb_ctx* ctx, double repulsion_strength, double debye_length, double* out_dev);
/* The energy whose gradient rmb_body_body_force is: out = U_body = sum_{i<j} eps exp(-r_ij/b) / r_ij over the resident points,
 * which the caller sets to the body LOCATIONS exactly as for rmb_body_body_force (rmb_set_positions with wall = 0; wall = 1 or
 * a target sub-range: RMB_ERR_STATE), r_ij in the minimal image of every direction with a positive period, z included.  One
 * more instance of rmb_blob_potential's sweep: the "yukawa" pair expression, but imaged in all three directions, with no wall
 * gate and no one-blob term (a centre with z <= 0 counts in full, no 1e5 (1 - z)), always fp64.  Each unordered pair once, one
 * partial per wave, the same finishing launch: no atomics, bit-reproducible for a given configuration, permutation and option
 * set.  "force_sort", "force_cull" (tile pairs beyond 750 b: exact zeros) and "potential_resort" apply as to
 * rmb_blob_potential.  One point gives 0; coincident points give +inf.  debye_length <= 0 or a null pointer: RMB_ERR_ARG.
 * The *_device variant writes the one double to device memory, asynchronously on the context's stream. */
int rmb_body_body_potential(rmb_ctx* ctx, double repulsion_strength, double debye_length, double* out_host);
int rmb_body_body_potential_device(rmb_ctx* ctx, double repulsion_strength, double debye_length, double* out_dev);
/* A blob-blob pair law given as a table: a radial law U(r) of K uniform intervals of width h from r0, one cubic per
 * interval, coeff_host[K][4] = (c0, c1, c2, c3) in fp64; r_cut = r0 + K h.
 *   r0 <= r < r_cut:  x = (r - r0)/h, k = min(floor(x), K - 1), t = x - k,
 *                     U = c0 + t (c1 + t (c2 + t c3)),  U' = (c1 + t (2 c2 + 3 t c3)) / h
 *   r < r0:           U = c[0][0] + (c[0][1]/h)(r - r0),  U' = c[0][1]/h      (a linear core, constant force magnitude)
 *   r >= r_cut:       U = U' = +0.0 exactly
 * The force on blob i is (U'(r)/r)(r_j - r_i), evaluated as U'(r) min(1/r, 1e25) (r_j - r_i): coincident blobs get a zero
 * force and the energy c[0][0] - c[0][1] r0 / h.  Force and energy are consistent by construction: the force is the exact
 * derivative of the interpolant whose value is the energy.  rmb_ctx_set_pair_table copies the table into the context
 * (synchronous; coeff_host is the caller's again on return) and replaces the one that was there; n_intervals = 0 clears it.
 * Refused with RMB_ERR_ARG before anything touches a device: n_intervals < 0 or > 1024, h not finite or <= 0, r0 negative
 * or not finite, a coefficient that is not finite, a null coeff_host with n_intervals > 0.  Uniform radius-free law, fp64
 * only; per-blob radii, "precision" = 32, pair shards and the multi-device engine do not serve it.
 *
 * rmb_pair_table_force: out (n,3), the forces of that law on the resident points (rmb_set_positions with wall = 0; wall = 1
 * or a target sub-range: RMB_ERR_STATE, as is a context without a table), minimal image in every direction with a positive
 * period.  Each unordered pair once on the symmetric force sweep whatever n, "symmetric", "deterministic" and "precision"
 * say (atomic flushes; last_path = 1); the K records are staged in K * 32 bytes of LDS per workgroup.  "force_cull" (tile
 * pairs beyond r_cut: exact zeros) and "force_sort" apply.
 *
 * rmb_blob_potential_table: rmb_blob_potential with the pair term taken from the table -- out = {U_one_blob, U_pair}; the
 * one-blob arguments, `form` (which now chooses the one-blob expression only), the wall gate (a blob with z <= 0 contributes
 * 1e5 (1 - z) and no pair term as the lower of the caller's two indices) and the minimal image in x and y only are
 * rmb_blob_potential's.  No atomics; tile culling by r_cut. */
int rmb_ctx_set_pair_table(rmb_ctx* ctx, double r0, double h, long n_intervals, const double* coeff_host);
int rmb_pair_table_force(rmb_ctx* ctx, double* out_host);
int rmb_pair_table_force_device(rmb_ctx* ctx, double* out_dev);
int rmb_blob_potential_table(rmb_ctx* ctx, double repulsion_strength_wall, double debye_length_wall, double weight,
                             double blob_radius, int form, double* out_host);
int rmb_blob_potential_table_device(rmb_ctx* ctx, double repulsion_strength_wall, double debye_length_wall, double weight,
                                    double blob_radius, int form, double* out_dev);
/* Histogram of the pair distances of the resident points: the counts behind the radial distribution function g(r)
 * (multi_bodies/examples/Radial_Dist_Test/gr_pseudo2D_single_blob.cpp).  Uses the raw positions as rmb_blob_potential
 * (rmb_set_positions with wall = 0; wall = 1 or a target sub-range: RMB_ERR_STATE).  For every unordered pair i < j:
 * r = |x_i - x_j| in the minimal image of every direction with a positive period (z included; the reference program's
 * formula, valid for separations of any number of periods), in fp64; if r < r_max, hist[(int)(r / dr)] += 1 with
 * dr = r_max / n_bins.  Coincident points count in bin 0.  One count per UNORDERED pair (the reference program counts 2).
 * The potential's sweep (each pair once, "force_sort" from 2048 points on, "force_cull": tile pairs further apart than r_max
 * are skipped, which drops no pair with r < r_max) with uint32 counters in LDS and integer atomics to the uint64 bins:
 * the counts are the same bits for every launch plan and option set.  Always fp64, single device.
 *   rmb_pair_histogram_device  ADDS into hist_dev[n_bins] (the caller zeroes it and may accumulate frames), asynchronous
 *                              on the context's stream;
 *   rmb_pair_histogram         zeroes hist_host[n_bins] first; synchronous.
 * rmb_pair_histogram_frames_device: the same counts for n_frames frames of n points each, frames_dev = (n_frames, n, 3)
 * packed doubles on the device, L = 3 periods on the host (<= 0: open), in ONE launch over (frame, tile pair), no sort, no
 * culling; adds into hist_dev.  It neither reads nor writes the resident configuration or any other state of the
 * context (only its device and stream), so a sampler may call it between energy evaluations.
 * RMB_ERR_ARG: a null pointer, r_max <= 0, n_bins < 1 or n_bins > 8192.  n = 0, n = 1 and n_frames = 0 leave the histogram
 * unchanged. */
int rmb_pair_histogram_device(rmb_ctx* ctx, double r_max, long n_bins, unsigned long long* hist_dev);
int rmb_pair_histogram(rmb_ctx* ctx, double r_max, long n_bins, unsigned long long* hist_host);
int rmb_pair_histogram_frames_device(rmb_ctx* ctx, const double* frames_dev, long n_frames, long n, const double* L, double r_max,
                                     long n_bins, unsigned long long* hist_dev);
/* Sums behind the 6 x 6 translational-rotational mean-square displacement of rigid-body trajectories (the reference's
 * general_application_utils.py: calc_total_msd_from_matrix_and_center / calc_msd_data_from_trajectory).  frames = (n_frames,
 * n_bodies, 7) packed doubles, one row x y z s p1 p2 p3 per body (quaternion scalar part first, used as it is, never
 * renormalised); offsets = (n_bodies, 3) body-frame tracking offsets p_b or NULL: the tracked point is c_b(f) = x_b(f) +
 * R(q_b(f)) p_b with the reference's rotation matrix.  For every origin o in [o_begin, o_end), lag l in [0, n_lags) with
 * o + l < n_frames, and body b:
 *   Delta = [ c_b(o + l) - c_b(o) ;  u ],   u = 2 s_rel v_rel,   (s_rel, v_rel) = q_b(o + l) (x) conj(q_b(o)),
 * which for unit quaternions is the reference's 1/2 sum_i (R(q(o)) e_i) x (R(q(o + l)) e_i); sums[l] += Delta Delta^T, sums =
 * (n_lags, 6, 6) doubles, both triangles.  Origins whose lag does not exist add nothing; the number of terms per lag follows from
 * the shapes and is the caller's to compute.  A record pass (tracked point and quaternion once per frame and body, body-major),
 * a sweep in which a lane owns a lag and keeps its 21 sums in registers, and a finishing launch that adds the workgroups'
 * partials in a fixed order: no atomics, the same bits for the same call.  origin_chunk: origins staged per window, 0 = planned
 * (values above 1024 are cut to 1024).  Always fp64, single device.  It reads and writes nothing of the resident configuration
 * (only the context's device, stream and a workspace of its own).
 *   rmb_msd_frames_device  ADDS into sums_dev (the caller zeroes it and may accumulate calls), asynchronous on the context's stream;
 *   rmb_msd_frames         host pointers; zeroes sums_host first; synchronous.
 * RMB_ERR_ARG, before the device is touched: a null context / sums / frames pointer, negative sizes, n_lags < 1, origin_chunk < 0,
 * or not 0 <= o_begin <= o_end <= n_frames.  n_frames = 0, n_bodies = 0 and o_begin = o_end leave the sums unchanged. */
int rmb_msd_frames_device(rmb_ctx* ctx, const double* frames_dev, long n_frames, long n_bodies, const double* offsets_dev_or_null,
                          long n_lags, long o_begin, long o_end, long origin_chunk, double* sums_dev);
int rmb_msd_frames(rmb_ctx* ctx, const double* frames_host, long n_frames, long n_bodies, const double* offsets_host_or_null,
                   long n_lags, long o_begin, long o_end, long origin_chunk, double* sums_host);
/* Density modes and the lag sums behind the structure factor S(k), the intermediate scattering function F(k, t) and its
 * self part F_s(k, t) of point trajectories, by direct Fourier sums (no grid; what the reference delegated to HydroGrid,
 * multi_bodies/multi_bodies.py: call_HydroGrid).  frames = (n_frames, n, 3) packed doubles on the device; L = 3 lengths on the
 * host; kint = (K, 3) integers n on the host: k = 2 pi (n_x / L_x, n_y / L_y, n_z / L_z).  L_d is the period of a periodic
 * direction (everything below is then invariant under wrapping) or any reference length of an open one; it may be <= 0
 * only where every n_d = 0.  Phase of point j in turns: t_j = sum_d x_jd (n_d / L_d), with one division per axis and
 * fused steps; theta_j = 2 pi (t_j - rint(t_j)), evaluated as sincospi(2 (t_j - rint(t_j))): the reduction is done in
 * turns, so a cloud many periods from the origin keeps its accuracy.
 *   rmb_density_modes_frames_device    modes[f, k] = (sum_j cos theta_j, -sum_j sin theta_j) = rho_k(f) = sum_j exp(-i theta_j);
 *                                      modes_dev = (n_frames, K, 2), OVERWRITTEN.  A lane owns a wavevector, the points of a
 *                                      frame are staged in LDS; few frames of many points are cut into point ranges whose
 *                                      partials a finishing launch adds in a fixed order.
 *   rmb_scattering_lags_device         C[l, k] = sum_o Re( rho_k(o + l) conj rho_k(o) ) over the modes (n_frames, K, 2);
 *   rmb_self_scattering_frames_device  Sf[l, k] = sum_o sum_j cos( theta_j(o + l) - theta_j(o) ), computed as
 *                                      Re( z_j(o + l) conj z_j(o) ), z = exp(-i theta), from per-point phase records of three
 *                                      wavevectors per pass;
 *                                      both for origins o in [o_begin, o_end), lags l in [0, n_lags) with o + l < n_frames,
 *                                      ADDED to sums_dev = (n_lags, K) (the caller zeroes it and may accumulate calls).  A
 *                                      lane owns a lag (the sweep of rmb_msd_frames_device), partials per workgroup, a
 *                                      finishing launch.
 * Normalisation is the caller's: S(k) = C[0, k] / (n n_origins), F(k, l) = C[l, k] / (n count[l]), F_s(k, l) = Sf[l, k] /
 * (n count[l]).  No floating-point atomics: the same call gives the same bits.  Always fp64, single device, asynchronous
 * on the context's stream.  Nothing of the resident configuration is read or written (only the context's device, stream
 * and a workspace of these entries).
 * RMB_ERR_ARG, before the device is touched: a null pointer (one whose array is empty may be null), negative sizes,
 * n_lags < 1, not 0 <= o_begin <= o_end <= n_frames, K > 16384, |n_d| > 32768, n_d != 0 where L_d <= 0.  n_frames = 0, K = 0
 * and o_begin = o_end leave the lag sums unchanged; n = 0 writes zero modes and adds nothing to the self sums. */
int rmb_density_modes_frames_device(rmb_ctx* ctx, const double* frames_dev, long n_frames, long n, const double* L, const int* kint,
                                    long K, double* modes_dev);
int rmb_scattering_lags_device(rmb_ctx* ctx, const double* modes_dev, long n_frames, long K, long n_lags, long o_begin, long o_end,
                               double* sums_dev);
int rmb_self_scattering_frames_device(rmb_ctx* ctx, const double* frames_dev, long n_frames, long n, const double* L, const int* kint,
                                      long K, long n_lags, long o_begin, long o_end, double* sums_dev);
/* Lag histograms behind the van Hove correlation functions of point trajectories: the self part G_s(r, t), the distribution
 * of single-point displacements, and the distinct part G_d(r, t), the time-dependent pair distribution (g(r) at t = 0).
 * frames = (n_frames, n, 3) packed doubles on the device, possibly unwrapped; origins o in [o_begin, o_end), lags l in
 * [0, n_lags), a pair (o, l) only where o + l < n_frames (the convention of rmb_msd_frames_device).  plane = 0: distances in
 * three dimensions; 1: the z component of every separation and displacement is ignored.
 *   rmb_van_hove_self_frames_device      hist[l, b] += #{(o, j) : bin(|x_j(o + l) - x_j(o)|) = b}, the displacement as it is
 *                                        (no minimal image, as the MSD); moments[l] += (sum |D|^2, sum |D|^4) over ALL terms,
 *                                        those at and beyond r_max included (NULL: not wanted).  A lane owns a point and keeps
 *                                        x_j(o) over a tile of lags; per-workgroup partial moments, a finishing launch.
 *   rmb_van_hove_distinct_frames_device  hist[l, b] += #{(o, i, j), i != j : bin(|image(x_i(o + l) - x_j(o))|) = b}: ORDERED
 *                                        pairs, minimal image in every direction with L_d > 0 (L = 3 lengths on the host; valid
 *                                        for separations of any number of periods).  A workgroup owns a lag; units (origin, tile,
 *                                        tile) over the full tile grid, the 64-step rotation of the pair sweeps.  hist[0] summed
 *                                        over origins is exactly twice rmb_pair_histogram_frames_device's counts.
 * Binning is rmb_pair_histogram's: a term with r < r_max (compared as r^2 < r_max^2) lands in bin (int)(r n_bins / r_max), capped
 * at n_bins - 1; r = 0 counts in bin 0; r >= r_max is dropped from the counts.  hist = (n_lags, n_bins) unsigned 64-bit, ADDED
 * to: uint32 counters in LDS, integer atomics to the caller's bins, the same bits for every launch plan (a workgroup meets
 * fewer than 2^31 terms, or the call is refused).  No floating-point atomics: the moments of the same call are the same bits.
 * Normalisation is the caller's (vanhove.py).  Always fp64, single device, asynchronous on the context's stream.  Nothing of
 * the resident configuration is read or written (only the context's device, stream and a workspace of the self entry).
 * RMB_ERR_ARG, before the context or the device is touched: a null hist / frames / L pointer, negative sizes, n_lags < 1, not
 * 0 <= o_begin <= o_end <= n_frames, plane not 0 or 1, r_max not positive and finite, n_bins outside 1 ... 8192, more pairs than
 * one launch can step through.  n_frames = 0, o_begin = o_end, n = 0 and, for the distinct entry, n = 1 leave the outputs unchanged. */
int rmb_van_hove_self_frames_device(rmb_ctx* ctx, const double* frames_dev, long n_frames, long n, long n_lags, long o_begin, long o_end,
                                    int plane, double r_max, long n_bins, unsigned long long* hist_dev, double* moments_dev_or_null);
int rmb_van_hove_distinct_frames_device(rmb_ctx* ctx, const double* frames_dev, long n_frames, long n, const double* L, long n_lags,
                                        long o_begin, long o_end, int plane, double r_max, long n_bins, unsigned long long* hist_dev);
/* Bond-orientational order of point frames (bond_order_kernels.h; bondorder.py): the sums behind psi_m(i), g_m(r), C_m(t).
 * frames = (n_frames, n, 3) packed doubles on the device, possibly unwrapped; L = 3 periods on the host (<= 0: open); every
 * separation in the minimal image of every direction with a positive period (rmb_pair_histogram's formula).  plane = 1 (xy):
 * distances are in-plane, sqrt(dx^2 + dy^2); plane = 0 (xyz): three-dimensional.  The bond angle is always the in-plane one.
 *   rmb_bond_order_frames_device   out[f, i] = {N_i, Re sum_j z_ij^m1, Im sum_j z_ij^m1, ...} over the neighbours j of point i
 *                                  in frame f: d_ij^2 < r_cut^2 and rho_ij^2 = dx^2 + dy^2 > 0 (the point itself and points
 *                                  stacked on it have no angle: out of the sums and of the count), z = (dx + i dy) / rho.
 *                                  out = (n_frames, n, 1 + 2 n_orders) doubles, OVERWRITTEN; N_i is exact.  orders: n_orders
 *                                  (1 ... 4) values 1 ... 16 on the host.  No trigonometric function: one reciprocal square
 *                                  root and binary powering.  Atomic-free, fixed-order sums: the same call gives the same
 *                                  bits.  source_chunk = 0: the sources of a frame are chunked as planned; > 0: that many
 *                                  sources per chunk (rounded up to a multiple of 4; the chunk count may change the last bits).
 *                                  psi_m(i) = sum / N_i is the caller's division.  r_cut should not exceed half the smallest
 *                                  positive period (beyond it a neighbour is met through one image only).
 *   rmb_pair_field_frames_device   field = (n_frames, n, 2) int32 on the device, (a, b) = rint(psi 2^30) with |a|, |b| <= 2^30.
 *                                  For every unordered pair of a frame with r < r_max, binned as rmb_pair_histogram:
 *                                  counts[bin] += 1 and sums[bin] += (a_i a_j + b_i b_j + 2^29) >> 30 (int64, arithmetic
 *                                  shift).  counts = [n_bins] unsigned 64-bit, sums = [n_bins] signed 64-bit, both ADDED to:
 *                                  integer accumulators in LDS, integer atomics, the same bits for every launch plan and
 *                                  point order.  g_m(r_b) = sums_b / (2^30 counts_b), within (sqrt(2) + 1/2) 2^-30 of the
 *                                  unquantised mean.
 * Always fp64 positions, single device, asynchronous on the context's stream.  Nothing of the resident configuration is read or
 * written (only the context's device, stream, and the one-sided sweeps' workspace of chunk partials for the first entry).
 * RMB_ERR_ARG, before the context or the device is touched: a null pointer, negative sizes, plane not 0 or 1, r_cut / r_max not
 * positive and finite, n_orders outside 1 ... 4, an order outside 1 ... 16, source_chunk < 0, n_bins outside 1 ... 4096, more
 * pairs than one launch can step through.  n_frames = 0 and n = 0 (for the second entry also n = 1) leave the outputs unchanged. */
int rmb_bond_order_frames_device(rmb_ctx* ctx, const double* frames_dev, long n_frames, long n, const double* L, double r_cut, int plane,
                                 const int* orders, int n_orders, long source_chunk, double* out_dev);
int rmb_pair_field_frames_device(rmb_ctx* ctx, const double* frames_dev, const int* field_dev, long n_frames, long n, const double* L,
                                 int plane, double r_max, long n_bins, unsigned long long* counts_dev, long long* sums_dev);
/* Cluster analysis (cluster_kernels.h; clusters.py): the connected components of the bond graph of a point configuration.
 * Points i and j of one frame are bonded when d_ij < r_cut, strictly (compared as d^2 < r_cut^2 in fp64): the separation in the
 * minimal image of every direction with a positive period (rmb_pair_histogram's formula, any number of periods away); plane = 0
 * (xyz): the three-dimensional distance; plane = 1 (xy): the in-plane distance, z and L_z ignored.  Coincident points, and
 * stacked points under xy, have d = 0 and ARE bonded (unlike the neighbours of rmb_bond_order_frames_device).  A cluster is a
 * connected component; the label of a point is the smallest caller index in its cluster.  select = one byte per point on the
 * device (non-zero: selected) or NULL (all): only bonds between two selected points exist; an unselected point gets label -1
 * and belongs to no cluster.
 *   labels[f, i]  int32: the label of point i of frame f (an index within the frame), -1 when unselected;
 *   sizes[f, l]   int32: the number of points of the cluster labelled l, 0 where l is nobody's label.
 * Both are (n_frames, n) (resident entry: n) on the device and OVERWRITTEN.  Three launches: parent = identity; the pair-once
 * sweep, whose pair term is a lock-free union-find in global memory (the larger root is hooked under the smaller with an
 * integer compare-and-swap; no lock, no spin-wait, no floating-point atomic); a finishing launch of one thread per point.  A
 * root is always the minimum of its set, so labels and sizes are the same bits for every launch plan, point order, culling
 * choice and cut of the trajectory.  The parent array lives in a workspace of the context.
 *   rmb_cluster_labels_frames_device  n_frames frames of n points, frames_dev = (n_frames, n, 3) packed doubles, L = 3 periods on
 *                                     the host (<= 0: open), one sweep over (frame, tile pair); n_frames * n <= 2^31 - 1 per
 *                                     call.  Nothing of the resident configuration is read or written.
 *   rmb_cluster_labels_device         the resident raw positions (rmb_set_positions with wall = 0; wall = 1 or a target
 *                                     sub-range: RMB_ERR_STATE), Morton-sorted from 2048 points on ("force_sort"), tile pairs
 *                                     further apart than r_cut skipped ("force_cull"; under plane xy the gap between two tiles
 *                                     is taken without its z term) -- which drops no bond.
 * Always fp64, single device, asynchronous on the context's stream.
 * RMB_ERR_ARG, before the context or the device is touched: a null frames / L / labels / sizes pointer (one whose array is
 * empty may be null), negative sizes, r_cut not positive and finite, plane not 0 or 1, n_frames * n above 2^31 - 1.
 * n_frames = 0 and n = 0 touch nothing; n = 1 gives label 0 and size 1. */
int rmb_cluster_labels_frames_device(rmb_ctx* ctx, const double* frames_dev, const unsigned char* select_dev_or_null, long n_frames, long n,
                                     const double* L, double r_cut, int plane, int* labels_dev, int* sizes_dev);
int rmb_cluster_labels_device(rmb_ctx* ctx, const unsigned char* select_dev_or_null, double r_cut, int plane, int* labels_dev,
                              int* sizes_dev);
/* Hydrodynamic function: the quadratic form of the translational pair mobility with plane waves,
 *   H(k; e) = (1 / (N mu0)) sum_i sum_j e^T M_ij e cos(k . (x_i - x_j)),   mu0 = 1 / (6 pi eta a)
 * (hydro_function_kernels.h).  M is the matrix of the tt product: RPY with the overlap patch; wall = 1: the single-wall block
 * on heights clamped to a, every block damped by b_i b_j, b = z / a for z < a, exactly as rmb_set_positions(wall = 1) packs a
 * configuration; mob_L: the three pseudo-periodic lengths of the mobility (<= 0: open; the 3^d images around the nearest one).
 * Wavevectors as the scattering entries take them: kint = (K, 3) integers n and L = three lengths on the host,
 * k = 2 pi n_d / L_d, the phase reduced in turns on the RAW coordinates.  pol = (K, 3) doubles on the host, the polarisation e
 * of every wavevector (used as given; a unit vector for H).  Per frame f and wavevector m the two raw sums
 *   out[f, m, 0] = S_self = sum_i b_i^2 e^T M_ii e            out[f, m, 1] = S_dist = 2 sum_{i<j} b_i b_j e^T M_ij e cos(theta_i - theta_j)
 * are OVERWRITTEN, out_dev = (n_frames, K, 2) doubles: H = (S_self + S_dist) / (N mu0).  The pair block is built once per
 * pair and contracted with eight wavevectors; no floating-point atomic: per-wave partial sums, added in a fixed order by a
 * finishing launch -- the same call gives the same bits.  fp64, one radius, one device, asynchronous on the context's stream.
 *   rmb_hydro_function_frames_device  n_frames frames of n points, frames_dev = (n_frames, n, 3) packed doubles on the device.
 *                                     Nothing of the resident configuration is read or written.
 *   rmb_hydro_function_device         the resident configuration with its own radius, boundary and periods (wall = 0 or 1; a
 *                                     free-surface configuration or a target sub-range: RMB_ERR_STATE), one frame.
 * RMB_ERR_ARG, before the device is touched: a null pointer (one whose array is empty may be null), negative sizes, K above
 * 16384, |n_d| above 32768, a nonzero n_d along a direction with L_d <= 0, a radius or eta that is not positive and finite,
 * wall not 0 or 1, a polarisation that is not finite, a mobility period that differs from the wavevector length of its
 * direction (the phase factor of a pair would depend on the image).  RMB_ERR_STATE: option "precision" = 32.
 * n_frames = 0 and K = 0 touch nothing; n = 0 gives zeros. */
int rmb_hydro_function_frames_device(rmb_ctx* ctx, const double* frames_dev, long n_frames, long n, double a, double eta, int wall,
                                     const double* mob_L, const double* L, const int* kint, const double* pol, long K, double* out_dev);
int rmb_hydro_function_device(rmb_ctx* ctx, double eta, const double* L, const int* kint, const double* pol, long K, double* out_dev);
/* Total potential energy of the resident configuration: the reference's equilibrium sampler's energy
 * (many_bodyMCMC/many_body_potential_pycuda.py:15-119), out = {U_one_blob, U_pair}; their sum is the reference's np.sum(U).
 * Uses the UNCLAMPED positions as rmb_blob_blob_force (rmb_set_positions with wall = 0; wall = 1 or a target sub-range:
 * RMB_ERR_STATE); minimal image in x and y (periodic_length[2] is ignored, as in the reference); uniform radius, fp64.
 *   form 0 "soft"    one blob, z > 0: weight z + (z < a ? e_w + e_w (a - z)/b_w : e_w exp(-(z - a)/b_w));
 *                    pair: r < 2a ? e + e (2a - r)/b : e exp(-(r - 2a)/b)
 *   form 1 "yukawa"  one blob: weight z + e_w a exp(-(z - a)/b_w)/|z - a| (+ 1e12 e_w when z < a); pair: e exp(-r/b)/r
 *                    (many_bodyMCMC/examples/boomerang_suspension/potential_pycuda_user_defined.py:26-71; r = 0 gives inf)
 * A blob with z <= 0 contributes 1e5 (1 - z) and no pair term as the lower of the caller's two indices.  repulsion_strength_wall
 * = 0 drops the wall term (debye_length_wall is then not read).  Each unordered pair once, every lane its own fp64 sum, one
 * partial per wave, a finishing launch that adds them in a fixed order: no atomics, bit-reproducible for a given
 * configuration, permutation and option set.  Options "force_cull" (skip tile pairs beyond 2a + 750 b, yukawa 750 b: exact
 * zeros) and "force_sort" (Morton order from 2048 blobs on) apply; "potential_resort" [K] = rebuild the Morton permutation on
 * every K-th evaluation and reuse it in between (the tile bounds are recomputed every time, so any permutation is correct).
 * The *_device variant writes the two doubles to device memory, asynchronously on the context's stream. */
int rmb_blob_potential(rmb_ctx* ctx, double repulsion_strength, double debye_length, double repulsion_strength_wall,
                       double debye_length_wall, double weight, double blob_radius, int form, double* out_host);
int rmb_blob_potential_device(rmb_ctx* ctx, double repulsion_strength, double debye_length, double repulsion_strength_wall,
                              double debye_length_wall, double weight, double blob_radius, int form, double* out_dev);
/* One Metropolis proposal of the rigid-body sampler in one launch (many_bodyMCMC/many_body_MCMC.py:160-169): for body
 * k < n_free  loc_new = loc + draws[k, 0:3],  quat_new = quaternion(draws[k, 3:6] max_angle_shift) * quat  (quaternion.py:17-39);
 * bodies from n_free on (prescribed kinematics) keep theirs; then r_new = R(quat_new) ref + loc_new for every blob.
 * blob_body_dev[n_blobs]: body of every blob (non-decreasing); blob_ref_dev[n_blobs]: row of ref_dev (rows x 3, the
 * structures' reference configurations) of every blob; draws_dev (n_bodies, 6).  Outputs must not alias the inputs. */
int rmb_mcmc_propose_device(rmb_ctx* ctx, long n_bodies, long n_free, long n_blobs, const int* blob_body_dev, const int* blob_ref_dev,
                            const double* ref_dev, const double* loc_dev, const double* quat_dev, const double* draws_dev,
                            double max_angle_shift, double* loc_new_dev, double* quat_new_dev, double* r_new_dev);
/* Single-body Metropolis moves.  E(r) = sum_i u1(z_i) + sum_{i<j, z_i>0} u2(r_ij) is rmb_blob_potential's energy (same forms,
 * same rule behind the wall, minimal image in x and y only, same r = 0 behaviour, fp64).  A body owns the contiguous blob
 * range [first, first + count) of r_dev (n_blobs x 3 raw coordinates, the caller's -- NOT the resident configuration, which
 * is neither read nor changed; periodic_length: 3 doubles on the host, [2] ignored).  With r' = r except for that range,
 * where it is r_body_new_dev (count x 3):
 *   out_dev = {U_one(r') - U_one(r), U_pair(r') - U_pair(r)}
 * as a sum over the touched terms, each subtracted (new - old) before it is accumulated: a pair with j < first is gated by
 * z_j > 0 (unchanged by the move), a pair with j >= first + count or with both blobs in the body (once, i < j) by z'_i > 0
 * for the new term and z_i > 0 for the old one.  One lane per blob of the configuration, the body staged in LDS 256 blobs at
 * a time (any count), one pair of partials per wave, a finishing launch that adds them in a fixed order: O(count n_blobs),
 * no atomics, bit-reproducible.  Asynchronous on the context's stream.  RMB_ERR_ARG: a null pointer, an empty or
 * out-of-range blob range, debye_length <= 0 (debye_length_wall <= 0 with a wall term), an unknown form. */
int rmb_mcmc_body_delta_device(rmb_ctx* ctx, long n_blobs, const double* r_dev, long first, long count, const double* r_body_new_dev,
                               const double* periodic_length, double repulsion_strength, double debye_length,
                               double repulsion_strength_wall, double debye_length_wall, double weight, double blob_radius, int form,
                               double* out_dev);
/* The same with the body-body energy of rmb_body_body_potential (strength body_repulsion_strength, range body_debye_length
 * > 0) between the n_bodies locations loc_dev (n_bodies x 3): body `body` moves from loc_dev[body] to loc_new_dev[0..2], and
 *   out_dev = {dU_one, dU_pair, U_body(loc') - U_body(loc)}
 * where the third entry is the sum over the other bodies j of u(|loc_j - loc'_body|) - u(|loc_j - loc_body|), each subtracted
 * before it is accumulated, in the minimal image of all three directions (periodic_length[2] is read by this term alone).  The
 * lane with global index j < n_bodies carries that term; the launch covers max(n_blobs, n_bodies) lanes and every wave stores
 * a third partial.  One body gives exactly 0.  RMB_ERR_ARG also for a body index outside [0, n_bodies). */
int rmb_mcmc_body_delta_bb_device(rmb_ctx* ctx, long n_blobs, const double* r_dev, long first, long count, const double* r_body_new_dev,
                                  long n_bodies, const double* loc_dev, long body, const double* loc_new_dev,
                                  const double* periodic_length, double repulsion_strength, double debye_length,
                                  double repulsion_strength_wall, double debye_length_wall, double weight, double blob_radius, int form,
                                  double body_repulsion_strength, double body_debye_length, double* out_dev);
/* One sweep of single-body moves over bodies 0 ... n_free - 1 in index order, inside the library.  Body k owns the blobs
 * [body_first[k], body_first[k + 1]) (host table of n_bodies + 1 entries from 0 to n_blobs, non-decreasing: anything else is
 * RMB_ERR_ARG).  Per body two launches: the first composes the proposal from draws_dev[k, 0:3] (displacement) and
 * draws_dev[k, 3:6] (rotation vector / max_angle_shift) with the arithmetic of rmb_mcmc_propose_device and computes the
 * difference above on r_dev; the finishing launch (one workgroup) adds the partials and decides
 *   draws_dev[k, 6] < exp(-(dU_one + dU_pair) / kT)      (numpy's comparison: a NaN rejects, -inf accepts).
 * On acceptance it commits in place the body's rows of r_dev, loc_dev[k], quat_dev[k] and energy_dev = {U_one, U_pair} (the
 * running energy: the caller initialises it, e.g. with rmb_blob_potential_device) and sets accepted_dev[k] = 1; on rejection it
 * writes accepted_dev[k] = 0 and nothing else.  draws_dev is (n_free, 7); bodies from n_free on are never moved.  No host
 * synchronisation and no copy command between moves: the caller reads accepted_dev and energy_dev after the call
 * (asynchronous on the context's stream).  With option "timing" the events bracket the whole sweep.  n_free = 0 is a no-op;
 * RMB_ERR_ARG also for a null pointer, kT <= 0, debye_length <= 0 (debye_length_wall <= 0 with a wall term). */
int rmb_mcmc_sweep_device(rmb_ctx* ctx, long n_bodies, long n_free, long n_blobs, const long* body_first, const int* blob_ref_dev,
                          const double* ref_dev, double* loc_dev, double* quat_dev, double* r_dev, const double* draws_dev,
                          double max_angle_shift, const double* periodic_length, double repulsion_strength, double debye_length,
                          double repulsion_strength_wall, double debye_length_wall, double weight, double blob_radius, int form,
                          double kT, double* energy_dev, int* accepted_dev);
/* The same sweep with the body-body energy between the locations loc_dev: the difference launch adds the centre term of
 * rmb_mcmc_body_delta_bb_device from loc_dev as the earlier moves of the sweep left it (the moved body's new centre is the
 * proposal it composes), the finishing launch decides on dU_one + dU_pair + dU_body and commits energy_dev = {U_one, U_pair,
 * U_body} (three doubles; the caller initialises the third e.g. with rmb_body_body_potential_device).  Bodies from n_free on
 * are never moved but take part in the centre pairs.  A deck without blobs (n_blobs = 0) may pass null blob arrays. */
int rmb_mcmc_sweep_bb_device(rmb_ctx* ctx, long n_bodies, long n_free, long n_blobs, const long* body_first, const int* blob_ref_dev,
                             const double* ref_dev, double* loc_dev, double* quat_dev, double* r_dev, const double* draws_dev,
                             double max_angle_shift, const double* periodic_length, double repulsion_strength, double debye_length,
                             double repulsion_strength_wall, double debye_length_wall, double weight, double blob_radius, int form,
                             double body_repulsion_strength, double body_debye_length, double kT, double* energy_dev,
                             int* accepted_dev);
/* One-blob forces of the rigid-multiblob driver (multi_bodies/multi_bodies_functions.py:153-188, `blob_external_force`):
 * f = (0, 0, -weight + wall repulsion), wall repulsion = (eps_wall / debye_wall) exp(-(h - a) / debye_wall) above contact
 * (h > a), eps_wall / debye_wall below; r_dev: n x 3 raw coordinates (the caller's, not the resident ones); accumulate != 0
 * adds to out_dev's z entries (e.g. on top of rmb_blob_blob_force_device's result), 0 overwrites all 3 n entries. */
int rmb_one_blob_force_device(rmb_ctx* ctx, long n, const double* r_dev, double blob_radius, double weight, double eps_wall,
                              double debye_wall, int accumulate, double* out_dev);
/* Pair shard `shard` of `nshards` of the forces (each unordered pair once, F_ji = -F_ij) into a full-length partial
 * (n,3): the sum over shards is rmb_blob_blob_force_device's result (all-reduce on several GPUs).  Atomic flushes
 * whatever "deterministic" says. */
int rmb_blob_blob_force_pairshard_device(rmb_ctx* ctx, double repulsion_strength, double debye_length,
                                         double blob_radius, double* out_dev, long shard, long nshards);
/* Same with one radius per blob: contact distance a_i + a_j instead of 2a (multi_bodies/forces_numba.py:73-137,
 * `blob_blob_force_implementation radii_numba`).  radii: double[n], host / device. */
int rmb_blob_blob_force_radii(rmb_ctx* ctx, const double* radii, double repulsion_strength, double debye_length,
                              double* out);
int rmb_blob_blob_force_radii_device(rmb_ctx* ctx, const double* radii_dev, double repulsion_strength,
                                     double debye_length, double* out_dev);

/* Timing of the dominant (sweep) kernel, measured with HIP events on the context's stream when the
 * "timing" option is on.  Copies up to max_n most recent durations (ms) into ms[], returns count. */
int rmb_timing_collect(rmb_ctx* ctx, double* ms, int max_n);
int rmb_timing_reset(rmb_ctx* ctx);
/* Measurement aid: chip-wide issue rate of independent v_fma_f64 (G wave-instructions per second, 4 waves per SIMD on
 * every CU, no memory traffic) over `launches` back-to-back launches on the context's stream -- the ceiling bench.py
 * prices the VALU-bound pair sweeps against, measured in the same process and clock state.  Synchronous. */
int rmb_ubench_fp64_issue(rmb_ctx* ctx, int launches, double* g_wave_instr_per_s);
/* Schedule diagnostics: with option "wave_clock" = 1 the symmetric kernel stamps every wave's start and end
 * (100 MHz wall clock); copies (start, end) pairs of the last launch into stamps[2*max_waves], returns count. */
int rmb_wave_clock_collect(rmb_ctx* ctx, long long* stamps, long max_waves);
/* Host wall clock of the last rmb_matvec call on this context, microseconds: us4 = {upload of the vector(s) (pageable
 * host memory: the copy is staged, the call returns when it is done), enqueue of the kernels, wait for them + download
 * of the result, the whole call}.  What the reference's synchronous call shape costs beyond the kernel. */
int rmb_last_host_timing(rmb_ctx* ctx, double* us4);
/* launch geometry of the last sweep: target tiles, source chunks, workgroups */
int rmb_last_launch(rmb_ctx* ctx, long* tiles, long* chunks, long* workgroups);
int rmb_ctx_synchronize(rmb_ctx* ctx);

/* Options of the library's default context, the one the stateless entry points below run on (rmb_mobility_oneshot,
 * rmb_forces_oneshot, rmb_mobility_source_target, rmb_pressure_stokeslet, rmb_double_layer): same keys as
 * rmb_ctx_set_option -- e.g. "precision" = 32 selects the single-precision twins for one-shot callers too. */
int rmb_default_ctx_set_option(const char* key, long value);
/* Device of the default context: an index, or -1 = RMB_DEVICE / 0 (the initial state).  An existing default context
 * on another device is destroyed (its resident positions go with it) and re-created on the next stateless call. */
int rmb_default_ctx_set_device(int device);

/* ---- single-process multi-device engine ------------------------------------------------------------------------
 * The reference's callers are ONE Python process that calls a module-level function (multi_bodies/multi_bodies.py:
 * 233-287 selects it, :445 / :599 call it; mobility/mobility.py:222-252 is the call shape): to give that call the
 * whole node the sharding has to sit behind it.  An engine owns one context per listed device, each with its own
 * stream.  Per product: inputs go to every device (host entry: one pinned staging copy + G uploads; device entry: every
 * shard pulls from devices[0] over xGMI with hipMemcpyPeerAsync), device g evaluates pair shard g of G (each unordered
 * pair once, both blobs updated) into a full-length partial, then device g sums slice g of the G partials in FIXED order
 * through peer-mapped reads of the other devices' partials and hands the slice over (peer copy to devices[0] / download).
 * Caller-owned memory is only ever touched by runtime copies; peer-mapped loads are confined to buffers the engine
 * allocated after it enabled peer access.  With option
 * "deterministic" = 2 the mobility products are bit-reproducible for a given device list (the forces' pair shards
 * flush with atomics whatever the option says).  No reference counterpart (single
 * device); the contract is "equal to the one-context result to rounding" (<= 1e-13).
 *   - devices: 1..16 indices; the same device may be listed several times (rehearsal of the G-device path on one GPU).
 *   - without peer access between two listed devices (or with RMB_MULTI_NO_PEER=1) slices travel by hipMemcpyPeerAsync.
 *   - rmb_multi_set_option: "reduce" 0 [default] = the fixed-order slice reduction, 1 = RCCL all-reduce in place
 *     (ncclCommInitAll; librccl.so is dlopen()ed on first use; distinct devices only; not bit-reproducible); every other
 *     key is forwarded to all shard contexts (rmb_ctx_set_option).  rmb_multi_get_option also answers "peer" (1 / 0)
 *     and "threads".
 *   - with several shards every shard has a worker thread that issues its HIP calls (~25 us per shard and product from
 *     one thread otherwise); RMB_MULTI_THREADS=0 keeps everything on the calling thread.  An engine is used from one
 *     thread at a time and does not survive fork() (its worker threads do not exist in the child: create it there).
 *   - host entry points are synchronous.  *_device entry points take pointers on devices[0], are ordered after the work
 *     already queued on the engine's primary stream (rmb_multi_set_stream; NULL = default stream of devices[0]) and
 *     order that stream after their own completion; the primary stream must be alive when a call is made, and may be
 *     destroyed between calls (a switch never touches the previous handle).
 *   - products: kinds as rmb_matvec (in_plane for TT / TR / RT / RR / TT_TR), operations as rmb_matvec_op_device,
 *     uniform-radius blob-blob forces.  Target ranges do not apply (every call produces all n targets). */
typedef struct rmb_multi rmb_multi;
int rmb_multi_create(const int* devices, int n_devices, rmb_multi** engine);
int rmb_multi_destroy(rmb_multi* engine);
int rmb_multi_n_shards(rmb_multi* engine);
/* the context of shard g (options, rmb_timing_collect, rmb_last_launch of one device); owned by the engine */
int rmb_multi_shard_ctx(rmb_multi* engine, int shard, rmb_ctx** ctx);
int rmb_multi_set_stream(rmb_multi* engine, void* hip_stream);
int rmb_multi_set_option(rmb_multi* engine, const char* key, long value);
int rmb_multi_get_option(rmb_multi* engine, const char* key, long* value);
int rmb_multi_set_positions(rmb_multi* engine, const double* r_host, long n, double a, const double* L, int wall);
int rmb_multi_set_positions_device(rmb_multi* engine, const double* r_dev, long n, double a, const double* L, int wall);
int rmb_multi_matvec(rmb_multi* engine, int kind, int in_plane, const double* vec_host, const double* vec2_host, double eta,
                     double* out_host);
int rmb_multi_matvec_device(rmb_multi* engine, int kind, int in_plane, const double* vec_dev, const double* vec2_dev,
                            double eta, double* out_dev);
int rmb_multi_matvec_op_device(rmb_multi* engine, int op, int in_plane, int n_in, const double* const* in_dev, int n_out,
                               double* const* out_dev, double eta);
int rmb_multi_blob_blob_force(rmb_multi* engine, double repulsion_strength, double debye_length, double blob_radius,
                              double* out_host);
int rmb_multi_blob_blob_force_device(rmb_multi* engine, double repulsion_strength, double debye_length, double blob_radius,
                                     double* out_dev);
int rmb_multi_synchronize(rmb_multi* engine);

/* ---- stateless one-shot calls: exactly the reference wrapper signature ----------------------
 * r, vec (, vec2) host (n,3); out host (n,3).  Uses a process-wide context on the default device (RMB_DEVICE, or 0;
 * rmb_default_ctx_set_device). */
int rmb_mobility_oneshot(int kind, int wall, int in_plane, long n, const double* r, const double* vec,
                         const double* vec2, double eta, double a, const double* L, double* out);
int rmb_forces_oneshot(long n, const double* r, const double* L, double repulsion_strength,
                       double debye_length, double blob_radius, double* out);
/* many_body_potential_pycuda.blobs_potential's arguments (r host (n,3), L = periodic_length or NULL): out = {U_one_blob, U_pair} */
int rmb_potential_oneshot(long n, const double* r, const double* L, double repulsion_strength, double debye_length,
                          double repulsion_strength_wall, double debye_length_wall, double weight, double blob_radius, int form,
                          double* out);

/* ---- source -> target products with per-blob radii (K13) --------------------------------------
 * u_t = sum_s M(x_t, a_t; y_s, a_s) f_s for nt targets and ns sources, each blob with its own radius
 * (mobility/mobility_numba.py:1480-1658; CUDA twin mobility_pycuda.py:1974-2078; wrappers
 * mobility.py:494-615: per-blob height clamp + B on both sides when wall == 1).  wall == 2 selects the
 * stress-free surface at z = 0 instead (mobility_numba.py:1941-2091, wrapper mobility.py:1409-1429: mirror image
 * with the z column negated, raw heights, no clamp).  Stateless; the host variant is synchronous, the device
 * variant enqueues on the context's stream. */
int rmb_mobility_source_target(long ns, const double* src, const double* radius_src, long nt, const double* tgt,
                               const double* radius_tgt, const double* force, double eta, const double* L, int wall,
                               double* out);
int rmb_mobility_source_target_device(rmb_ctx* ctx, long ns, const double* src_dev, const double* radius_src_dev,
                                      long nt, const double* tgt_dev, const double* radius_tgt_dev,
                                      const double* force_dev, double eta, const double* L, int wall, double* out_dev);

/* ---- Stokeslet pressure and Stokes double layer, source -> target ---------------------------------------------
 * The remaining O(N_s N_t) operators of mobility/mobility_numba.py (wrappers mobility/mobility.py:1345-1366,
 * :1376-1387, :1432-1442).  Plain positions (no height clamp, no radii), stateless like the K13 entry points; the
 * host variants are synchronous, the device variants enqueue on the context's stream.  Atomic-free, bit-reproducible.
 *
 * rmb_pressure_stokeslet: out[nt], p_t = 1/(4 pi) sum_s f_s . r/|r|^3, wall = 1 adds Blake's image system
 *   (mobility_numba.py:1332-1396, :1399-1476).  The reference's wall routine rescales its running sum inside the
 *   source loop (:1474); the factor is applied once here (= the reference for one source, = superposition of its
 *   single-source results).  L must be NULL or zero: the reference's pseudo-periodic branch divides by the unwrapped
 *   distance (:1374-1375), which is not reproduced -- RMB_ERR_ARG otherwise.
 * rmb_double_layer: out[3 nt], u_t = -3/(4 pi) sum_s w_s r (r.n_s)(r.v_s)/|r|^5, pairs with r <= 1e-14 skipped;
 *   wall = 1 adds the image terms of mobility_numba.py:1725-1759 (evaluated for r = 0 too); blob_radius >= 0 selects
 *   the RPY-regularised unbounded operator (:2095-2168; wall must be 0), blob_radius < 0 the plain one. */
int rmb_pressure_stokeslet(long ns, const double* src, long nt, const double* tgt, const double* force, const double* L,
                           int wall, double* out);
int rmb_pressure_stokeslet_device(rmb_ctx* ctx, long ns, const double* src_dev, long nt, const double* tgt_dev,
                                  const double* force_dev, const double* L, int wall, double* out_dev);
int rmb_double_layer(long ns, const double* src, long nt, const double* tgt, const double* normals, const double* vector,
                     const double* weights, int wall, double blob_radius, double* out);
int rmb_double_layer_device(rmb_ctx* ctx, long ns, const double* src_dev, long nt, const double* tgt_dev,
                            const double* normals_dev, const double* vector_dev, const double* weights_dev, int wall,
                            double blob_radius, double* out_dev);

/* ---- Laplace layer operators of phoretic bodies -------------------------------------------------------------------
 * Laplace_kernels/Laplace_kernels_numba.py.  Nodes x (n x 3), quadrature weights w, unit normals n, a field f per
 * node; every operator is 1/(4 pi) sum_j w_j f_j K(x_i - x_j).  wall = 1 adds the image of a no-slip wall at z = 0:
 * source (x, y, -z), normal (n_x, n_y, -n_z), kept for j == i.  The self operators skip the free-space term of
 * j == i by index, the source -> target ones every pair with |r| < 1e-12.  Plain positions (no height clamp), no
 * periodic images.  Atomic-free, bit-reproducible; the host variants run synchronously on the default context.
 *
 * rmb_laplace_single_layer:          out[n]    S[f]_i = 1/(4 pi) sum_j w_j f_j / |r_ij|                 (:12)
 * rmb_laplace_double_layer:          out[n]    D[f]_i = 1/(4 pi) sum_j w_j f_j (r_ij . n_j) / |r_ij|^3   (:68)
 * rmb_laplace_deriv_double_layer:    out[3n]   G[f]_i = 1/(4 pi) sum_j w_j f_j (I - 3 r r^T/r^2) n_j / r^3  (:138)
 * rmb_laplace_dipole:                out[3n]   P[f]_i = 1/(4 pi) sum_j w_j f_j r_ij / |r_ij|^3          (:254)
 * rmb_laplace_single_layer_source_target, rmb_laplace_double_layer_source_target: out[nt], S / D from ns sources
 *   to nt targets                                                                                        (:329, :398)
 *
 * Device sweeps of the concentration solve (phoretic slip), sources = targets = the n nodes, on the context's stream;
 * out must not alias an input:
 * rmb_laplace_operator_device:  out[n]  = alpha p_i - D[p]_i + S[q]_i   in one pass.  p or q may be NULL (that term is
 *   absent and not computed; alpha applies to p); normals may be NULL when p is.
 * rmb_laplace_gradient_device:  out[3n] = 2 G[p]_i - 2 P[q]_i   in one pass; p or q may be NULL likewise. */
int rmb_laplace_single_layer(long n, const double* r, const double* field, const double* weights, int wall, double* out);
int rmb_laplace_double_layer(long n, const double* r, const double* field, const double* weights, const double* normals,
                             int wall, double* out);
int rmb_laplace_deriv_double_layer(long n, const double* r, const double* field, const double* weights,
                                   const double* normals, int wall, double* out);
int rmb_laplace_dipole(long n, const double* r, const double* field, const double* weights, int wall, double* out);
int rmb_laplace_single_layer_source_target(long ns, const double* src, long nt, const double* tgt, const double* field,
                                           const double* weights, int wall, double* out);
int rmb_laplace_double_layer_source_target(long ns, const double* src, long nt, const double* tgt, const double* field,
                                           const double* weights, const double* normals, int wall, double* out);
int rmb_laplace_operator_device(rmb_ctx* ctx, long n, const double* r_dev, const double* normals_dev,
                                const double* weights_dev, const double* p_dev, const double* q_dev, double alpha, int wall,
                                double* out_dev);
int rmb_laplace_gradient_device(rmb_ctx* ctx, long n, const double* r_dev, const double* normals_dev,
                                const double* weights_dev, const double* p_dev, const double* q_dev, int wall,
                                double* out_dev);

#ifdef __cplusplus
}
#endif
#endif /* RMB_MOBILITY_H */
