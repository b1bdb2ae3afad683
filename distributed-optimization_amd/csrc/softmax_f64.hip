// softmax_f64.hip -- k_round_softmax instantiations: float64 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_softmax.inc"

namespace dopt {

hipError_t launch_softmax_f64(const SoftmaxArgs& a, int n_workers, hipStream_t s) {
  return softmax_dispatch<double, double>(a, n_workers, s);
}

}  // namespace dopt
