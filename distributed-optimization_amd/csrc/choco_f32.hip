// choco_f32.hip -- k_round_choco instantiations: float32 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_choco.inc"

namespace dopt {

hipError_t launch_choco_f32(int problem, int cpl, bool met, const ChocoArgs& a, int n_workers, hipStream_t s) {
  return choco_dispatch_cpl<float, float>(problem, cpl, met, a, n_workers, s);
}

}  // namespace dopt
