// softmax_x32.hip -- k_round_softmax instantiations: float64 iterates and arithmetic over float32-stored rows (dopt_set_data_dtype).
#include "kcommon.h"
#include "k_round_softmax.inc"

namespace dopt {

hipError_t launch_softmax_x32(const SoftmaxArgs& a, int n_workers, hipStream_t s) {
  return softmax_dispatch<double, float>(a, n_workers, s);
}

}  // namespace dopt
