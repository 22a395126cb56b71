// rmb_symx2t.hip -- two-targets-per-lane instances of the generic symmetric skeleton, open boundaries (symx2t_kernels.h).
#include "symx2t_instances.h"

namespace rmbi {
SymKernel symx_two_open(int sx, bool wall) { return symx2t_detail::table<false>(sx, wall); }
}  // namespace rmbi
