// pushsum_f64.hip -- k_round_pushsum instantiations: float64 iterates, arithmetic and rows.
#include "kcommon.h"
#include "k_round_pushsum.inc"

namespace dopt {

hipError_t launch_pushsum_f64(int problem, int cpl, bool met, const PushsumArgs& a, int n_workers, hipStream_t s) {
  return pushsum_dispatch_cpl<double, double>(problem, cpl, met, a, n_workers, s);
}

hipError_t launch_pushsum_debias(int dtype, const void* u, const void* phi, void* zt, int64_t n, int64_t ld,
                                 hipStream_t s) {
  return dtype == 0 ? pushsum_debias_t<float>(u, phi, zt, n, ld, s) : pushsum_debias_t<double>(u, phi, zt, n, ld, s);
}

}  // namespace dopt
