// gt_f64.hip -- k_round_gt instantiations: float64 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_gt.inc"

namespace dopt {

hipError_t launch_gt_f64(int problem, int cpl, bool met, const GtArgs& a, int n_workers, hipStream_t s) {
  return gt_dispatch_cpl<double, double>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
