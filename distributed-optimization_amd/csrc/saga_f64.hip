// saga_f64.hip -- k_round_saga instantiations: float64 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_saga.inc"

namespace dopt {

hipError_t launch_saga_f64(int problem, int cpl, bool met, const SagaArgs& a, int n_workers, hipStream_t s) {
  return saga_dispatch_cpl<double, double>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
