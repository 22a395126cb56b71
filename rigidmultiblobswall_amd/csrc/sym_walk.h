// sym_walk.h -- the walk of a wave over its share of the symmetric schedule (sym_schedule.h), written once: the frame
// under sym_kernel, sym2_kernel and sym_force_kernel, the wave-owned symmetric kernels with one target blob per lane whose
// device code and speed it leaves as they were.  No kernel is defined here.  symx_kernel, sym32_tt_kernel, symx32_kernel and
// sym_force32_kernel still write the same loop out (each says why: register allocation, or a measured slowdown) and keep
// its always-true `if` before the seek, so that their device code is the parent's byte for byte; the two-target kernels
// (sym2t_kernels.h, symx2t_kernels.h: another unit grid) and the cooperative ones (sym_coop_kernels.h, symx_coop_kernels.h:
// the workgroup owns the walk) have loops of their own kind.
//
// The rotation steps of a launch, 64 per unit, form the range [step_begin, step_end).  A kernel hands the walk a body
// struct that holds the lane registers it carries from unit to unit (set up by a constructor that leaves them alone:
// aggregate initialisation would zero them as one block, and the compiler then packs the pair arithmetic differently)
// and these force-inlined members:
//   begin()                       reset the lane state; once per chunk, before its first unit
//   culled(I, J)                  wave-uniform: unit (I, J) contributes exactly nothing (constant false where nothing culls)
//   load_row(I)                   fetch row tile I into the lane and zero the row accumulator
//   flush_row(unit_before)        add the row accumulator to the result; unit_before = the last unit index the row run
//                                 covers (the deterministic variant stores its row partial in that unit's slot)
//   unit(I, J, k0, k1, unit)      stage tile J, sync, pair loop over the steps [k0, k1) of the unit, transposed flush,
//                                 trailing barrier
// A culled unit consumes its steps and advances the unit order but causes no row load, no flush and no unit() call.
// The unit indices -- flush_row's argument and unit()'s last -- are what the DET slots of symx_kernel take; that kernel is
// not on the walk yet, so NO body reads them today (the three take them unnamed) and only the host test checks them.
//
// The walk itself is plain integer arithmetic above the __HIPCC__ block, as sym_schedule.h arranges things: it uses no
// HIP builtin -- the kernel computes its wave number -- and tests/test_sym_walk_host.py runs it on the host with a
// recording body.
#pragma once
#include "sym_schedule.h"
#ifdef __HIPCC__
#include "pair_ops.h"   // kSymWaves
#endif

namespace rmb {

struct SymWalk {
  int order, n_tiles;             // unit order (unit_seek / unit_next) on the triangle of n_tiles tiles
  long step_begin, step_end;      // rotation steps [begin, end) of the n_units * 64 this launch covers (pair shard)
  long spw;                       // steps per chunk
  long n_waves, w;                // waves of the launch, number of this one (sym_wave)
};

// Strided chunks: wave `w` takes the step ranges w, w + n, w + 2 n, ... of `spw` steps each (one range when the launch is
// planned that way: n spw >= the steps of the launch).  Waves that run at the same time then work on NEIGHBOURING ranges
// whatever the size of the problem -- with the blocked unit order and the XCD-aware numbering that keeps a launch's tile
// loads in one L2 (profiles/r4_unit_order.txt).  A chunk may begin and end inside a unit: [k0, k1) is the part of the
// unit a visit covers; the unit is decoded once at the chunk start, later units follow by increment.
template <class BODY>
__device__ __forceinline__ void sym_walk(const SymWalk& r, BODY& b) {
  for (long chunk = r.w;; chunk += r.n_waves) {
    long s = r.step_begin + chunk * r.spw;
    if (s >= r.step_end) break;
    long s_end = s + r.spw;
    if (s_end > r.step_end) s_end = r.step_end;
    int I = 0, J = 0;
    unit_seek(r.order, s >> 6, r.n_tiles, I, J);
    int I_cur = -1;
    b.begin();
    while (s < s_end) {
      const int k0 = (int)(s & 63);
      const long left = s_end - s;
      const int k1 = (left < 64 - k0) ? (int)(k0 + left) : 64;
      const long unit = s >> 6;
      s += k1 - k0;
      if (!b.culled(I, J)) {
        if (I != I_cur) {
          if (I_cur >= 0) b.flush_row(unit - 1);
          I_cur = I;
          b.load_row(I);
        }
        b.unit(I, J, k0, k1, unit);
      }
      if (k1 == 64) unit_next(r.order, r.n_tiles, I, J);
    }
    if (I_cur >= 0) b.flush_row((s_end - 1) >> 6);
  }
}

#ifdef __HIPCC__
// the number of this wave in the walk (and of its slot in any per-wave output); xcd != 0: XCD-aware workgroup numbering
__device__ __forceinline__ long sym_wave(int xcd) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  return (xcd ? xcd_swizzle(blockIdx.x, gridDim.x) : (long)blockIdx.x) * kSymWaves + wave;
}
__device__ __forceinline__ long sym_n_waves() { return (long)gridDim.x * kSymWaves; }

// what one lane wrote to the wave's LDS slab is visible to the others after this (and the other way round)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif  // __HIPCC__

}  // namespace rmb
