// gt_f32.hip -- k_round_gt instantiations: float32 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_gt.inc"

namespace dopt {

hipError_t launch_gt_f32(int problem, int cpl, bool met, const GtArgs& a, int n_workers, hipStream_t s) {
  return gt_dispatch_cpl<float, float>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
