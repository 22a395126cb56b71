// pair_once_kernels.h -- the frame of the pair-once scalar sweeps (gfx950, fp64): potential energy (potential_kernels.h)
// and pair-distance histogram (pair_hist_kernels.h).  Written once here; a sweep is a policy class.  No kernel is defined.
//
// "Every unordered pair once, and the result is not per point": the schedule of sym_force_kernel (sym_force_kernels.h)
// without its transposed half.  A work unit is a tile pair I <= J of 64 x 64 points and takes 64 rotation steps; lane l is
// point l of tile I (kept in registers while I stays), tile J is staged in the wave's LDS slab `rec` and read by rotation
// (step k: lane l meets slot (l + k) & 63).  A diagonal unit stages the tile itself: step 0 is free for a per-point hook,
// steps 1..32 meet every unordered pair of the tile once -- at k = 32 both lanes of a pair would meet, so that step is
// peeled off the loop and taken by the lower half of the wave -- and steps 33..63 are empty.  The steps of all units form
// one range [0, step_end) that the waves of the launch walk in strided chunks of `chunk_steps` (0: one contiguous range
// per wave), unit_seek at the chunk start and unit_next from there (sym_schedule.h), with the optional XCD-aware
// workgroup numbering.  A chunk may begin and end inside a unit: [k0, k1) is the part of the unit this visit covers.
// Off-diagonal units beyond the reach of the pair term are skipped (tile_gap2 against cull2).
//
// Per lane the pairs are met in schedule order: units as the walk meets them, k ascending, the peeled step last.  The
// energy's floating-point sums depend on exactly that order.
//
// The policy OP supplies (all static, every function __device__ __forceinline__):
//   Args               kernel argument struct, derived from PairOnceArgs
//   Lane               what a lane carries through the whole launch (sums, a pointer to counters)
//   FRAMES             the unit index runs over (frame, tile pair), frame slow, a.units_per_frame units each, row-major
//   PAD_W              .w of a padding record
//   fetch(a, frame, i)                  point i (< a.n) as a record: x, y, z and whatever pair() wants in .w
//   culled(a, I, J)                     wave-uniform: every term of the off-diagonal unit (I, J) is exactly nothing
//   diag_start(a, st, self, valid)      step 0 of a diagonal unit, once per point of the tile
//   guarded(a, I, J)                    wave-uniform choice of the pair body of a unit
//   pair<GUARDED>(a, st, self, q, take) one pair; `take` is true in the loop and lane < 32 at the peeled step
// Padding (the lanes past n of a partial last tile) is staged as points 2e100 apart with .w = PAD_W; pair() must make
// nothing of them.
// A policy that declares `static constexpr bool SLOTS = true` keeps per-point data of its own next to the records (the
// hydrodynamic function's phase factors, hydro_function_kernels.h) and per-chunk sums.  It supplies, on top of the above:
//   row(a, st, self, valid)             once per fetch of the lane's own point (tile I changed)
//   stage(a, st, p, lane, diag)         the record p has just gone into slot `lane`: fill the policy's own slab, same slot
//   pair<GUARDED>(a, st, self, q, take, slot)   pair() with the slot q was read from
//   flush(a, st, chunk)                 the steps of chunk `chunk` are done; once per chunk
// and its chunks are cut PER FRAME: a.spw steps each (always given, never the one-range-per-wave default), a.chunks_per_frame
// = ceil(steps of a frame / a.spw) of them in every frame, the last one short; chunk c is piece c % chunks_per_frame of frame
// c / chunks_per_frame.  No chunk reaches into the next frame, and how a frame is cut does not depend on the frames around it.
// Policies without SLOTS compile to what they were: every use below is an `if constexpr`.
// The walk below stays its own loop, not sym_walk (sym_walk.h): FRAMES needs a hook at the unit advance that no other sweep uses.
#pragma once
#include "pair_ops.h"
#include "sym_schedule.h"
#include "sym_walk.h"

#include <type_traits>

namespace rmb {

template <class OP, class = void> struct PairOnceSlots : std::false_type {};
template <class OP> struct PairOnceSlots<OP, std::void_t<decltype(OP::SLOTS)>> : std::bool_constant<OP::SLOTS> {};

// The fields the frame reads; fill_sym_args (rmb_internal.h) fills them by name.
struct PairOnceArgs {
  const double4* pos;   // packed raw positions (caller's order, or the Morton-sorted copy)
  const double* bounds; // [n_tiles][6] tile bounding boxes of `pos`
  double cull2;         // squared reach of the pair term; +inf = no culling
  long n;               // points (per frame)
  int n_tiles;
  int order, xcd;
  long chunk_steps;     // > 0: steps per strided chunk of a wave; 0: one contiguous range per wave
  long step_end;        // n_units * 64
  double Lx, Ly, iLx, iLy, Lz, iLz;
};

// minimal image of one separation component (L <= 0: open direction); the padding sentinels pass through
template <bool PERIODIC>
__device__ __forceinline__ double image(double L, double iL, double d) {
  if constexpr (PERIODIC) {
    if (L > 0) d = wrap_nearest_pad_safe(d, L, iL);
  }
  return d;
}

// the number of this wave in the walk (and of its slot in any per-wave output)
__device__ __forceinline__ long pair_once_wave(const PairOnceArgs& a) { return sym_wave(a.xcd); }

// steps [kb, kl) of a unit, then the peeled step 32
template <class OP, bool GUARDED>
__device__ __forceinline__ void pair_once_steps(const typename OP::Args& a, typename OP::Lane& st, const double4& self, const double4* rec,
                                                int lane, int kb, int kl, bool peel) {
  for (int k = kb; k < kl; ++k) {
    const double4 q = rec[(lane + k) & 63];
    if constexpr (PairOnceSlots<OP>::value) OP::template pair<GUARDED>(a, st, self, q, true, (lane + k) & 63);
    else                                    OP::template pair<GUARDED>(a, st, self, q, true);
  }
  if (peel) {
    const double4 q = rec[(lane + 32) & 63];
    if constexpr (PairOnceSlots<OP>::value) OP::template pair<GUARDED>(a, st, self, q, lane < 32, (lane + 32) & 63);
    else                                    OP::template pair<GUARDED>(a, st, self, q, lane < 32);
  }
}

// `rec`: this wave's slab of 64 records
template <class OP>
__device__ __forceinline__ void pair_once_sweep(const typename OP::Args& a, typename OP::Lane& st, double4* rec) {
  const int lane = threadIdx.x & 63;
  const long n_waves = sym_n_waves();
  const long w = pair_once_wave(a);
  long spw;
  if constexpr (PairOnceSlots<OP>::value) spw = a.spw;
  else spw = a.chunk_steps > 0 ? a.chunk_steps : (a.step_end + n_waves - 1) / n_waves;
  for (long chunk = w;; chunk += n_waves) {
    long s = chunk * spw;
    long s_end = s + spw;
    if constexpr (PairOnceSlots<OP>::value) {      // piece chunk % chunks_per_frame of frame chunk / chunks_per_frame
      const long f = chunk / a.chunks_per_frame, spf = a.units_per_frame * 64;
      s = f * spf + (chunk - f * a.chunks_per_frame) * spw;
      s_end = s + spw;
      if (s_end > (f + 1) * spf) s_end = (f + 1) * spf;
    }
    if (s >= a.step_end) break;
    if (s_end > a.step_end) s_end = a.step_end;
    int I = 0, J = 0;
    long frame = 0;
    if constexpr (OP::FRAMES) {
      frame = (s >> 6) / a.units_per_frame;
      unit_seek(0, (s >> 6) - frame * a.units_per_frame, a.n_tiles, I, J);
    } else {
      unit_seek(a.order, s >> 6, a.n_tiles, I, J);
    }
    int I_cur = -1;
    double4 self = make_double4(0.0, 0.0, 0.0, 0.0);
    bool vi_ok = false;
    while (s < s_end) {
      const int k0 = (int)(s & 63);
      const long left = s_end - s;
      const int k1 = (left < 64 - k0) ? (int)(k0 + left) : 64;
      s += k1 - k0;
      const bool diag = (I == J);
      const bool idle = diag ? (k0 > 32) : OP::culled(a, I, J);
      if (!idle) {
        if (I != I_cur) {
          I_cur = I;
          const long i = 64L * I + lane;
          vi_ok = i < a.n;
          self = make_double4(1e100, 1e100, 1e100, OP::PAD_W);
          if (vi_ok) self = OP::fetch(a, frame, i);
          if constexpr (PairOnceSlots<OP>::value) OP::row(a, st, self, vi_ok);
        }
        if (!diag) {
          const long j = 64L * J + lane;
          double4 p = make_double4(-1e100, -1e100, -1e100, OP::PAD_W);
          if (j < a.n) p = OP::fetch(a, frame, j);
          rec[lane] = p;
          if constexpr (PairOnceSlots<OP>::value) OP::stage(a, st, p, lane, false);
        } else {
          rec[lane] = make_double4(vi_ok ? self.x : -1e100, vi_ok ? self.y : -1e100, vi_ok ? self.z : -1e100, self.w);
          if constexpr (PairOnceSlots<OP>::value) OP::stage(a, st, self, lane, true);
          if (k0 == 0) OP::diag_start(a, st, self, vi_ok);
        }
        wave_lds_sync();
        const int kb = (diag && k0 < 1) ? 1 : k0;
        const int ke = (diag && k1 > 33) ? 33 : k1;
        // step 32 of a diagonal unit is met from both of its lanes: it is peeled off the loop and taken by the lower half
        const bool peel = diag && kb <= 32 && ke > 32;
        const int kl = peel ? 32 : ke;
        if (OP::guarded(a, I, J)) pair_once_steps<OP, true>(a, st, self, rec, lane, kb, kl, peel);
        else                      pair_once_steps<OP, false>(a, st, self, rec, lane, kb, kl, peel);
        __builtin_amdgcn_wave_barrier();   // rec is rewritten by the next unit
      }
      if (k1 == 64) {
        unit_next(OP::FRAMES ? 0 : a.order, a.n_tiles, I, J);
        if constexpr (OP::FRAMES) {
          if (I == a.n_tiles) { I = 0; J = 0; ++frame; I_cur = -1; }      // first unit of the next frame
        }
      }
    }
    if constexpr (PairOnceSlots<OP>::value) OP::flush(a, st, chunk);
  }
}

}  // namespace rmb
