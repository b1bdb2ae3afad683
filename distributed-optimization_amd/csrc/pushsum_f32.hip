// pushsum_f32.hip -- k_round_pushsum instantiations: float32 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_pushsum.inc"

namespace dopt {

hipError_t launch_pushsum_f32(int problem, int cpl, bool met, const PushsumArgs& a, int n_workers, hipStream_t s) {
  return pushsum_dispatch_cpl<float, float>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
