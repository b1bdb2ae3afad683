// saga_x32.hip -- k_round_saga instantiations: float64 iterates and arithmetic over float32-stored rows (dopt_set_data_dtype).
#include "kcommon.h"
#include "k_round_saga.inc"

namespace dopt {

hipError_t launch_saga_x32(int problem, int cpl, bool met, const SagaArgs& a, int n_workers, hipStream_t s) {
  return saga_dispatch_cpl<double, float>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
