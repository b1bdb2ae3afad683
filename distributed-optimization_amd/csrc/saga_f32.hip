// saga_f32.hip -- k_round_saga instantiations: float32 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_saga.inc"

namespace dopt {

hipError_t launch_saga_f32(int problem, int cpl, bool met, const SagaArgs& a, int n_workers, hipStream_t s) {
  return saga_dispatch_cpl<float, float>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
