// softmax_f32.hip -- k_round_softmax instantiations: float32 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_softmax.inc"

namespace dopt {

hipError_t launch_softmax_f32(const SoftmaxArgs& a, int n_workers, hipStream_t s) {
  return softmax_dispatch<float, float>(a, n_workers, s);
}

}  // namespace dopt
