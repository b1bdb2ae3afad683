// local_f32.hip -- k_round_local instantiations: float32 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_local.inc"

namespace dopt {

hipError_t launch_local_f32(int problem, int cpl, bool met, const LocalArgs& a, int n_workers, hipStream_t s) {
  return local_dispatch_cpl<float, float>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
