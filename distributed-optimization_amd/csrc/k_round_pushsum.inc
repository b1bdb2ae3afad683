// k_round_pushsum.inc -- the fused push-sum round (subgradient-push, Nedic & Olshevsky; stochastic
// gradient push, Assran et al.) and its launch dispatch, included by one translation unit per
// (state, data) element-type pair (pushsum_f32.hip, pushsum_f64.hip, pushsum_x32.hip).  The mixing
// matrix A is COLUMN-stochastic with a positive diagonal (a directed graph: A_ij = 1 / (1 + outdeg_j)),
// stored in CSR by rows -- row i lists the in-neighbours j of i and i itself.  State per worker: the
// numerator u_i (the context's iterates), the push-sum weight phi_i > 0 (1 at the start of a chain)
// and the de-biased iterate z_i = u_i / phi_i.  Round t, worker i:
//   v_i    = sum_j A_ij u_j                          (CSR order)
//   phi_i' = sum_j A_ij phi_j                        (CSR order)
//   z_i    = v_i / phi_i'                            (element-wise division)
//   g_i    = grad f_i(z_i; B_{t,i}) + lam z_i        (0 for an empty shard)
//   u_i'   = v_i - eta_t g_i
//   zt_i   = u_i' / phi_i'                           (the point the metrics are taken at)
// With a doubly stochastic A and phi = 1 this is u' = W u - eta g(W u): COMBINE-then-adapt, the
// gradient at the mixed point -- not the D-SGD round of k_round (and of the reference), which takes
// the gradient at the worker's own iterate, u' = W u - eta g(u).  sum_i phi_i = N in every round.
//
// One workgroup per worker.  The row stream is k_round_gt's: every wave streams whole shard rows
// (non-temporal 16-byte loads, the next row requested before the current row's arithmetic, peeled
// and pipelined at CPL <= 4), holds the gradient point, zbar and its gradient partial in registers,
// and takes the row's two dots (x . z for the gradient, x . zbar for the objective of the previous
// round) through one paired butterfly.  What is new: the gradient point does not exist in memory.
//   prologue   behind each wave's first row request, every thread forms phi' from the CSR row
//              (wave-uniform loads, the same bits in every thread: no broadcast, no barrier), and
//              thread tid forms v[c] of its state chunks c = tid + q * threads in CSR order
//              (mix_chunk's left-to-right order).  v[c] stays in the owner's registers; z[c] =
//              v[c] / phi' goes to ONE state row of LDS.  Wave 0 meanwhile takes the consensus
//              partial of the worker's zt row (the state BEFORE the round) at zbar.  One barrier,
//              then every wave loads its w[.] registers from that LDS row -- k_round_local's
//              reload, here at step 0.
//   epilogue   the owner of chunk c folds the waves' partials in wave order, forms gc = s / nb +
//              lam z[c] (z[c] from the LDS row it wrote) and u' = v[c] - eta gc, and stores u' to the
//              other iterate buffer and zt = u' / phi' to the zt buffer, whose column sums the host
//              takes next (xbar = zbar).  Thread 0 stores phi' to the other half of the weight
//              buffer.  No global read, no atomics, every sum in a fixed order.
// A launch without F_STEP runs the row arithmetic of the metrics alone (consensus of zt_i and the
// loss of every row at zbar): no mix, no barrier for it, no store.
//
// LDS: [red: waves x nch state chunks] [z: nch] [sred: 2 x waves doubles]
//      [ubuf / ybuf: the deferred objective terms' dots and labels (float64 arithmetic)]
// k_round_local's plan: every shape that kernel fits, this one fits.
namespace dopt {

// Waves per workgroup: k_round_gt's rule (8 while a register-resident state vector takes <= 4
// 16-byte registers per lane, else 4).
template <typename T, typename S, int CPL>
constexpr int pushsum_waves() {
  return (CPL * (int)sizeof(typename KV<T, S>::V) / 16 <= 4) ? 2 * NW : NW;
}

template <typename T, typename S, int CPL, int PROB, bool MET>
__global__ __launch_bounds__((pushsum_waves<T, S, CPL>() * 64)) __attribute__((amdgpu_waves_per_eu(1))) void k_round_pushsum(
    const PushsumArgs pa) {
  const RoundArgs& a = pa.r;
  constexpr int KW = pushsum_waves<T, S, CPL>();
  constexpr int KT = KW * 64;
  using V = typename KV<T, S>::V;    // state chunk (numerator, gradient point, gradient, zbar)
  using VX = typename KV<T, S>::VX;  // data chunk (shard row)
  constexpr int VN = KV<T, S>::VN;
  constexpr bool DBL = std::is_same<T, double>::value;
  constexpr bool FAST = !DBL && PROB == 0;  // hardware exp / log / reciprocal for the float logistic terms
  constexpr bool PIPE = CPL <= 4;           // two row buffers fit the registers only there
  constexpr int CPT = (64 * CPL + KT - 1) / KT;  // state chunks of a row per thread
  extern __shared__ __attribute__((aligned(32))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x;
  const int flags = a.flags;
  const int nch = a.nchunks;
  const int64_t ld = a.ld;
  const int64_t row0 = a.off[i];
  const int64_t m = a.off[i + 1] - row0;
  const int64_t nb = a.idx ? (a.b < m ? a.b : m) : m;
  // without F_STEP the launch only takes the metrics of the current de-biased iterates (the pass
  // after a call's last round): the same row arithmetic, no mix and no store
  const bool step = (flags & F_STEP) != 0;
  const bool want_loss = MET && (flags & F_LOSS);  // full-shard batches only (host-checked)
  const bool want_cons = MET && (flags & F_CONS);
  const bool defer = MET && DBL && want_loss && a.defer_rows > 0;
  const int64_t nrow = (step || want_loss) ? nb : 0;
  const S* __restrict__ X = (const S*)a.X;
  const S* __restrict__ Yp = (const S*)a.y;
  const int32_t* __restrict__ bidx = a.idx ? a.idx + (int64_t)i * a.b : nullptr;

  V* red = (V*)smem;  // [KW][nch]
  V* zrow = red + (size_t)KW * nch;
  double* sred = (double*)(zrow + nch);  // [2][KW]
  T* ubuf = (T*)(sred + 2 * KW);         // deferred objective terms: the row's dot with zbar ...
  S* ybuf = (S*)(ubuf + a.defer_rows);   // ... and its label, as stored

  auto load_row = [&](int64_t rr, VX (&dst)[CPL], T& yd) {
    const int64_t lr = bidx ? bidx[rr] : rr;
    const S* xp = X + (row0 + lr) * ld;
    yd = (T)Yp[row0 + lr];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int c = lane + 64 * j;
      const int cc = c < nch ? c : nch - 1;  // lanes past the row re-read its last chunk (w, xb are 0 there)
      dst[j] = __builtin_nontemporal_load((const VX*)(xp + (int64_t)cc * VN));
    }
  };
  VX cur[CPL], nxt[CPL];
  T ycur = T(0), ynxt = T(0);
  if (PIPE && wave < nrow) load_row(wave, cur, ycur);  // the first row, ahead of everything else

  V w[CPL], xb[CPL], g[CPL];
  const bool need_xb = want_loss || want_cons;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int c = lane + 64 * j;
    xb[j] = (MET && need_xb && c < nch) ? *(const V*)((const T*)a.xbar + (int64_t)c * VN) : V(0);
    w[j] = V(0);
    g[j] = V(0);
  }

  // prologue: phi' (every thread, the same bits) and v of this thread's state chunks, CSR order
  T ph = T(1);
  V v[CPT];
#pragma unroll
  for (int q = 0; q < CPT; ++q) v[q] = V(0);
  if (step) {
    const int64_t pe0 = a.rp[i], pe1 = a.rp[i + 1];
    const T* __restrict__ cw = (const T*)a.cw;
    const T* __restrict__ pho = (const T*)pa.phi_old;
    ph = T(0);
    for (int64_t e = pe0; e < pe1; ++e) ph += cw[e] * pho[a.ci[e]];
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = threadIdx.x + q * KT;
      if (c < nch) {
        V ax = V(0);
        const int64_t co = (int64_t)c * VN;
#pragma unroll 2
        for (int64_t e = pe0; e < pe1; ++e)
          ax += cw[e] * *(const V*)((const T*)a.x_old + (int64_t)a.ci[e] * ld + co);
        v[q] = ax;
        zrow[c] = ax / ph;  // read back by every wave after the barrier, and by this thread in the epilogue
      }
    }
  }

  // the consensus partial of zt_i (the state before the round) at zbar: wave 0, ahead of its rows
  double cons = 0.0;
  if constexpr (MET) {
    if (want_cons && wave == 0) {
      const T* zsrc = (const T*)pa.zt + (int64_t)i * ld;
      V dv = V(0);
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        const V t = (c < nch ? *(const V*)(zsrc + (int64_t)c * VN) : V(0)) - xb[j];
        dv += t * t;
      }
      cons = wave_sum((double)hsumn<T, VN>(dv));
    }
  }

  if (step) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int c = lane + 64 * j;
      if (c < nch) w[j] = zrow[c];
    }
  }

  double loss = 0.0;
  auto process = [&](VX (&rx)[CPL], T yv, int64_t rr) {
    V rv[CPL];  // the row in T (float32 data -> float64: exact)
    V az = V(0), au = V(0);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      rv[j] = __builtin_convertvector(rx[j], V);
      az += rv[j] * w[j];
      if (MET) au += rv[j] * xb[j];
    }
    T z = hsumn<T, VN>(az), u = hsumn<T, VN>(au);
    wave_sum_pair(z, u, z, u);
    if (step) {
      T coef;
      if constexpr (FAST) coef = -yv * sigmoid_neg_fast(yv * z);
      else coef = (PROB == 0) ? -yv * sigmoid_neg(yv * z) : z - yv;
#pragma unroll
      for (int j = 0; j < CPL; ++j) g[j] += coef * rv[j];
    }
    if constexpr (MET) {
      if (defer) {  // loss term after the row stream, lane-parallel
        if (lane == 0) {
          ubuf[rr] = u;
          ybuf[rr] = (S)yv;  // (T)(S) y: exact
        }
      } else if (want_loss) {
        if constexpr (FAST) loss += row_loss_fast(yv, u);
        else loss += row_loss<T, PROB>(yv, u);
      }
    }
  };
  if constexpr (PIPE) {
    // peeled: every iteration requests the next row unconditionally, so the wait before the
    // current row's arithmetic covers that row only
    int64_t r = wave;
    for (; r + KW < nrow; r += KW) {
      load_row(r + KW, nxt, ynxt);
      process(cur, ycur, r);
#pragma unroll
      for (int j = 0; j < CPL; ++j) cur[j] = nxt[j];
      ycur = ynxt;
    }
    if (r < nrow) process(cur, ycur, r);
  } else {
    for (int64_t r = wave; r < nrow; r += KW) {
      load_row(r, cur, ycur);
      process(cur, ycur, r);
    }
  }

  if (step) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int c = lane + 64 * j;
      if (c < nch) red[(size_t)wave * nch + c] = g[j];
    }
  }
  if constexpr (MET) {
    if (lane == 0) {
      sred[wave] = cons;
      sred[KW + wave] = loss;
    }
  }
  __syncthreads();

  if (step) {
    const T eta = (T)a.eta;
    const T lam = (T)a.lam;
    T* un = (T*)a.x_new + (int64_t)i * ld;
    T* zt = (T*)pa.zt + (int64_t)i * ld;
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = threadIdx.x + q * KT;
      if (c < nch) {
        V s = red[c];
#pragma unroll
        for (int p = 1; p < KW; ++p) s += red[(size_t)p * nch + c];  // fixed order
        const V gc = (nb > 0) ? (s / (T)nb + lam * zrow[c]) : V(0);
        const V u = v[q] - eta * gc;
        const int64_t co = (int64_t)c * VN;
        *(V*)(un + co) = u;
        *(V*)(zt + co) = u / ph;
      }
    }
    if (threadIdx.x == 0) ((T*)pa.phi_new)[i] = ph;
  }
  if constexpr (MET) {
    if (defer) {  // the loss terms of the rows, lane-parallel (fixed order: thread-strided, then waves)
      double l = 0.0;
      for (int64_t r = threadIdx.x; r < m; r += KT) l += row_loss<T, PROB>((T)ybuf[r], ubuf[r]);
      l = wave_sum(l);
      if (lane == 0) sred[KW + wave] = l;
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      double cs = 0.0, ls = 0.0;
#pragma unroll
      for (int q = 0; q < KW; ++q) {
        cs += sred[q];
        ls += sred[KW + q];
      }
      if (want_cons) a.slab_cons[i] = cs;
      if (want_loss) a.slab_loss[i] = ls;
    }
  }
}

// zt[i] = u[i] / phi[i] for every worker: the de-biased iterates of a state the round kernel did not
// write (the start of a call, dopt_pushsum_get_state).  The division is the epilogue's, so a call
// that starts where another ended finds the bits that call left.
template <typename T>
__global__ __launch_bounds__(256) void k_pushsum_debias(const T* __restrict__ u, const T* __restrict__ phi,
                                                        T* __restrict__ zt, int64_t ld) {
  const int64_t i = blockIdx.x;
  const T ph = phi[i];
  for (int64_t k = threadIdx.x; k < ld; k += 256) zt[i * ld + k] = u[i * ld + k] / ph;
}

template <typename T>
static hipError_t pushsum_debias_t(const void* u, const void* phi, void* zt, int64_t n, int64_t ld, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_pushsum_debias<T>), dim3((unsigned)n), dim3(256), 0, s, (const T*)u, (const T*)phi, (T*)zt, ld);
  return hipGetLastError();
}

template <typename T, typename S, int CPL, int PROB, bool MET>
static hipError_t launch_pushsum_t(const PushsumArgs& g, int groups, hipStream_t s) {
  constexpr int KW = pushsum_waves<T, S, CPL>();
  constexpr size_t VB = sizeof(typename KV<T, S>::V);
  const RoundArgs& a = g.r;
  if (a.nchunks < 1 || a.nchunks > 64 * CPL || !a.rp || !g.zt) return hipErrorInvalidValue;
  if ((a.flags & F_STEP) && (!g.phi_old || !g.phi_new)) return hipErrorInvalidValue;
  if ((a.flags & F_LOSS) && a.idx) return hipErrorInvalidValue;  // the objective needs every row of the shard
  const bool defer = MET && std::is_same<T, double>::value && (a.flags & F_LOSS) && a.defer_rows > 0;
  const size_t ub = defer ? ((size_t)a.defer_rows * (sizeof(T) + sizeof(S)) + 15) / 16 * 16 : 0;
  const size_t lds = (size_t)(KW + 1) * a.nchunks * VB + 2 * KW * sizeof(double) + ub;
  const size_t max_lds = 160 * 1024;
  if (lds > max_lds) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_round_pushsum<T, S, CPL, PROB, MET>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  static const std::string name = [] {
    char buf[160];
    snprintf(buf, sizeof(buf), "void dopt::k_round_pushsum<%s, %s, %d, %d, %s>(dopt::PushsumArgs)",
             std::is_same<T, float>::value ? "float" : "double", std::is_same<S, float>::value ? "float" : "double",
             CPL, PROB, MET ? "true" : "false");
    return std::string(buf);
  }();
  note_round_kernel(name.c_str());
  hipLaunchKernelGGL((k_round_pushsum<T, S, CPL, PROB, MET>), dim3(groups), dim3(KW * 64), lds, s, g);
  return hipGetLastError();
}

template <typename T, typename S, int CPL>
static hipError_t pushsum_dispatch_mode(int problem, bool met, const PushsumArgs& g, int groups, hipStream_t s) {
  if (problem == 0)
    return met ? launch_pushsum_t<T, S, CPL, 0, true>(g, groups, s) : launch_pushsum_t<T, S, CPL, 0, false>(g, groups, s);
  return met ? launch_pushsum_t<T, S, CPL, 1, true>(g, groups, s) : launch_pushsum_t<T, S, CPL, 1, false>(g, groups, s);
}

template <typename T, typename S>
static hipError_t pushsum_dispatch_cpl(int problem, int cpl, bool met, const PushsumArgs& g, int groups,
                                       hipStream_t s) {
  if (groups <= 0) return hipSuccess;
  switch (cpl) {
    case 1: return pushsum_dispatch_mode<T, S, 1>(problem, met, g, groups, s);
    case 2: return pushsum_dispatch_mode<T, S, 2>(problem, met, g, groups, s);
    case 4: return pushsum_dispatch_mode<T, S, 4>(problem, met, g, groups, s);
    case 8: return pushsum_dispatch_mode<T, S, 8>(problem, met, g, groups, s);
    case 16:
      // float64 state over float32 rows at 16 chunks per lane is beyond the register file, as for
      // k_round_gt (such rows are column-blocked contexts, which the push-sum round rejects)
      if constexpr (std::is_same<T, S>::value) return pushsum_dispatch_mode<T, S, 16>(problem, met, g, groups, s);
      break;
  }
  return hipErrorInvalidValue;
}

}  // namespace dopt
