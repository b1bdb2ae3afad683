// sparse_x32.hip -- k_round_sparse instantiations: float64 iterates and arithmetic over float32-stored non-zeros.
#include "kcommon.h"
#include "k_round_sparse.inc"

namespace dopt {

hipError_t launch_sparse_x32(int problem, const SparseArgs& a, int n_workers, hipStream_t s) {
  return sparse_dispatch<double, float>(problem, a, n_workers, s);
}

}  // namespace dopt
