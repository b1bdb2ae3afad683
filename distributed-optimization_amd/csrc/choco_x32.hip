// choco_x32.hip -- k_round_choco instantiations: float64 iterates and arithmetic over float32-stored rows (dopt_set_data_dtype).
#include "kcommon.h"
#include "k_round_choco.inc"

namespace dopt {

hipError_t launch_choco_x32(int problem, int cpl, bool met, const ChocoArgs& a, int n_workers, hipStream_t s) {
  return choco_dispatch_cpl<double, float>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
