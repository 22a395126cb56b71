// scat_phase.h -- the phase factor of a point for one wavevector, the one route every Fourier sum of the library takes
// (scattering_kernels.h says why; hydro_function_kernels.h shares it).  No kernel is defined.
#pragma once
#include <hip/hip_runtime.h>

namespace rmb {

// (cos theta, sin theta) of a point for the wavevector with c = n / L
__device__ __forceinline__ void scat_phase(double x, double y, double z, double cx, double cy, double cz, double* s, double* c) {
  const double t = __builtin_fma(z, cz, __builtin_fma(y, cy, x * cx));
  const double r = t - __builtin_rint(t);
  sincospi(r + r, s, c);
}

}  // namespace rmb
