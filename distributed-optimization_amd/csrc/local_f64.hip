// local_f64.hip -- k_round_local instantiations: float64 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_local.inc"

namespace dopt {

hipError_t launch_local_f64(int problem, int cpl, bool met, const LocalArgs& a, int n_workers, hipStream_t s) {
  return local_dispatch_cpl<double, double>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
