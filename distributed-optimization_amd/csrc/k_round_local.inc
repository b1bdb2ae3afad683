// k_round_local.inc -- the fused local-steps round (Local SGD / periodic decentralized SGD) and its
// launch dispatch, included by one translation unit per (state, data) element-type pair
// (local_f32.hip, local_f64.hip, local_x32.hip).  Round t of tau gradient steps, worker i, global
// step s = tau t + k, with W the mixing matrix (CSR, diagonal included):
//   k = 0:          g = grad f_i(x_i; B_{t,0}) + lam x_i;   u = sum_j W_ij x_j - eta_{tau t} g
//   k = 1..tau-1:   g = grad f_i(u;   B_{t,k}) + lam u;     u = u - eta_{tau t + k} g
//   x_i <- u
// i.e. x_{s+1} = W_s x_s - eta_s g_s(x_s) with W_s = W when s mod tau == 0 and I otherwise; g is 0
// for an empty shard (k_round_gt's rule) and tau = 1 is the D-SGD round.  The neighbours' rows are
// read in step 0 only, so a round is ONE launch whatever tau is.
//
// One workgroup per worker.  The row stream is k_round_gt's: every wave streams whole shard rows
// (non-temporal 16-byte loads, the next row requested before the current row's arithmetic, peeled
// and pipelined at CPL <= 4), holds the iterate and its gradient partial in registers, and takes the
// row's two dots (x . w for the gradient, x . xbar for the objective of the previous round) through
// one paired butterfly.  The iterate never leaves the workgroup between the tau steps:
//   prologue   behind each wave's first row request, thread tid forms mx[c] = sum_j W_ij x_j[c] of
//              its state chunks c = tid + q * threads in CSR order (mix_chunk's left-to-right order)
//              and parks it in ONE state row of LDS;
//   step k     every wave streams its share of B_{t,k} (minibatches: rows wave, wave + KW, .. of
//              idx[k][i][.]) and writes its gradient partial to red[wave][.]; barrier; the owner of
//              chunk c folds the partials in wave order, forms gc = s / nb + lam wc with wc the copy
//              of the iterate at c it keeps in a register (selecting it from w[.] by the wave's
//              number costs the CPL >= 4 instances a scratch array), and
//              u = (k == 0 ? mx[c] : wc) - eta_k gc.  On the last step u goes to x_new with a
//              vector store; otherwise it replaces mx[c], a second barrier follows and every wave
//              reloads its w[.] registers from that LDS row.
// Two barriers per local step, no global traffic for the state between steps.  The consensus and
// objective partials of x_t at xbar_t are taken in step 0's pass only (the objective needs
// full-shard batches); a launch without F_STEP runs step 0's row arithmetic and nothing else.
//
// LocalArgs.prefetch (A/B, DESIGN.md 6j): a wave requests the first row of step k + 1 before step
// k's reduction barrier -- its address does not depend on u -- instead of after the reload.  The
// bits are the same either way.
//
// LDS: [red: waves x nch state chunks] [mx: nch] [sred: 2 x waves doubles]
//      [ubuf / ybuf: the deferred objective terms' dots and labels (float64 arithmetic)]
// one state row less than k_round_gt: every shape that kernel fits, this one fits.
namespace dopt {

// Waves per workgroup: k_round_gt's rule (8 while a register-resident state vector takes <= 4
// 16-byte registers per lane, else 4).
template <typename T, typename S, int CPL>
constexpr int local_waves() {
  return (CPL * (int)sizeof(typename KV<T, S>::V) / 16 <= 4) ? 2 * NW : NW;
}

template <typename T, typename S, int CPL, int PROB, bool MET>
__global__ __launch_bounds__((local_waves<T, S, CPL>() * 64)) __attribute__((amdgpu_waves_per_eu(1))) void k_round_local(
    const LocalArgs la) {
  const RoundArgs& a = la.r;
  constexpr int KW = local_waves<T, S, CPL>();
  constexpr int KT = KW * 64;
  using V = typename KV<T, S>::V;    // state chunk (iterate, gradient, xbar)
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
  // without F_STEP the launch only takes the metrics of the current iterates (the pass after a
  // call's last round): step 0's row arithmetic, no mix and no store
  const bool step = (flags & F_STEP) != 0;
  const int tau = step ? la.tau : 1;
  const bool want_loss = MET && (flags & F_LOSS);  // full-shard batches only (host-checked)
  const bool want_cons = MET && (flags & F_CONS);
  const bool defer = MET && DBL && want_loss && a.defer_rows > 0;
  const int64_t nrow0 = (step || want_loss) ? nb : 0;  // rows of step 0's pass; the later passes walk nb
  const bool pre = la.prefetch != 0;
  const S* __restrict__ X = (const S*)a.X;
  const S* __restrict__ Yp = (const S*)a.y;
  const T* wsrc = (const T*)a.x_old + (int64_t)i * ld;

  V* red = (V*)smem;  // [KW][nch]
  V* mx = red + (size_t)KW * nch;
  double* sred = (double*)(mx + nch);   // [2][KW]
  T* ubuf = (T*)(sred + 2 * KW);        // deferred objective terms: the row's dot with xbar ...
  S* ybuf = (S*)(ubuf + a.defer_rows);  // ... and its label, as stored

  // row rr of step k's batch: idx[k][i][rr] of this round's [tau][n][b] draws, or the shard's row rr
  auto load_row = [&](int k, int64_t rr, VX (&dst)[CPL], T& yd) {
    const int64_t lr = a.idx ? a.idx[((int64_t)k * gridDim.x + i) * a.b + rr] : rr;
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
  if (PIPE && wave < nrow0) load_row(0, wave, cur, ycur);  // the first row, ahead of everything else

  V w[CPL], xb[CPL], g[CPL];
  const bool need_xb = want_loss || want_cons;
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int c = lane + 64 * j;
    const bool in = c < nch;
    w[j] = in ? *(const V*)(wsrc + (int64_t)c * VN) : V(0);
    xb[j] = (MET && need_xb && in) ? *(const V*)((const T*)a.xbar + (int64_t)c * VN) : V(0);
  }

  // prologue: sum_j W_ij x_j of this thread's state chunks, CSR order; own[q]: the iterate at those
  // chunks (x_i, then the u this thread formed in the previous step), so the fold indexes no w[.]
  V own[CPT];
#pragma unroll
  for (int q = 0; q < CPT; ++q) own[q] = V(0);
  if (step) {
    const int64_t pe0 = a.rp[i], pe1 = a.rp[i + 1];
    const T* __restrict__ cw = (const T*)a.cw;
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = threadIdx.x + q * KT;
      if (c < nch) {
        V ax = V(0);
        const int64_t co = (int64_t)c * VN;
#pragma unroll 2
        for (int64_t e = pe0; e < pe1; ++e)
          ax += cw[e] * *(const V*)((const T*)a.x_old + (int64_t)a.ci[e] * ld + co);
        mx[c] = ax;  // read back by this same thread in step 0's fold
        own[q] = *(const V*)(wsrc + co);
      }
    }
  }

  double loss = 0.0;
  // one row; FIRST: step 0's pass, which also carries the metrics of x_t at xbar_t
  auto process = [&](auto first, VX (&rx)[CPL], T yv, int64_t rr) {
    constexpr bool FIRST = decltype(first)::value;
    V rv[CPL];  // the row in T (float32 data -> float64: exact)
    V az = V(0), au = V(0);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      rv[j] = __builtin_convertvector(rx[j], V);
      az += rv[j] * w[j];
      if (MET && FIRST) au += rv[j] * xb[j];
    }
    T z = hsumn<T, VN>(az), u = T(0);
    if constexpr (FIRST) {  // the paired butterfly with or without metrics: the same z bits either way
      u = hsumn<T, VN>(au);
      wave_sum_pair(z, u, z, u);
    } else {
      z = wave_sum_dpp(z);
    }
    if (step) {
      T coef;
      if constexpr (FAST) coef = -yv * sigmoid_neg_fast(yv * z);
      else coef = (PROB == 0) ? -yv * sigmoid_neg(yv * z) : z - yv;
#pragma unroll
      for (int j = 0; j < CPL; ++j) g[j] += coef * rv[j];
    }
    if constexpr (MET && FIRST) {
      if (defer) {  // loss term after the steps, lane-parallel
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
  // the rows wave, wave + KW, .. < nrow of step k's batch
  auto pass = [&](auto first, int k, int64_t nrow) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) g[j] = V(0);
    if constexpr (PIPE) {
      // peeled: every iteration requests the next row unconditionally, so the wait before the
      // current row's arithmetic covers that row only (cur holds row `wave`, requested earlier)
      int64_t r = wave;
      for (; r + KW < nrow; r += KW) {
        load_row(k, r + KW, nxt, ynxt);
        process(first, cur, ycur, r);
#pragma unroll
        for (int j = 0; j < CPL; ++j) cur[j] = nxt[j];
        ycur = ynxt;
      }
      if (r < nrow) process(first, cur, ycur, r);
    } else {
      for (int64_t r = wave; r < nrow; r += KW) {
        load_row(k, r, cur, ycur);
        process(first, cur, ycur, r);
      }
    }
  };
  // after step k's pass: fold the waves' partials, step, and hand u on (LDS) or out (x_new)
  auto finish = [&](int k) {
    const bool last = k == tau - 1;
    if (PIPE && pre && !last && wave < nb) load_row(k + 1, wave, cur, ycur);  // across the barrier
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int c = lane + 64 * j;
      if (c < nch) red[(size_t)wave * nch + c] = g[j];
    }
    __syncthreads();
    const T eta = (T)la.eta[k];
    const T lam = (T)a.lam;
    T* xn = (T*)a.x_new + (int64_t)i * ld;
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = threadIdx.x + q * KT;
      if (c < nch) {
        V s = red[c];
#pragma unroll
        for (int p = 1; p < KW; ++p) s += red[(size_t)p * nch + c];  // fixed order
        const V wc = own[q];  // the point of this step's gradient at chunk c
        const V gc = (nb > 0) ? (s / (T)nb + lam * wc) : V(0);
        const V u = (k == 0 ? mx[c] : wc) - eta * gc;
        if (last) *(V*)(xn + (int64_t)c * VN) = u;
        else mx[c] = own[q] = u;
      }
    }
    if (!last) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        w[j] = c < nch ? mx[c] : V(0);
      }
      if (PIPE && !pre && wave < nb) load_row(k + 1, wave, cur, ycur);
    }
  };

  pass(std::true_type{}, 0, nrow0);
  if constexpr (MET) {
    double cons = 0.0;
    if (want_cons && wave == 0) {  // every wave holds the whole iterate: count it once
      V dv = V(0);
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const V t = w[j] - xb[j];
        dv += t * t;
      }
      cons = wave_sum((double)hsumn<T, VN>(dv));
    }
    if (lane == 0) {
      sred[wave] = cons;
      sred[KW + wave] = loss;
    }
  }
  if (step) {
    finish(0);
    for (int k = 1; k < tau; ++k) {
      pass(std::false_type{}, k, nb);
      finish(k);
    }
  }
  if constexpr (MET) {
    __syncthreads();  // sred (and the deferred terms) of every wave
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

template <typename T, typename S, int CPL, int PROB, bool MET>
static hipError_t launch_local_t(const LocalArgs& g, int groups, hipStream_t s) {
  constexpr int KW = local_waves<T, S, CPL>();
  constexpr size_t VB = sizeof(typename KV<T, S>::V);
  const RoundArgs& a = g.r;
  if (a.nchunks < 1 || a.nchunks > 64 * CPL || !a.rp) return hipErrorInvalidValue;
  if ((a.flags & F_STEP) && (g.tau < 1 || g.tau > kMaxLocalSteps)) return hipErrorInvalidValue;
  if ((a.flags & F_LOSS) && a.idx) return hipErrorInvalidValue;  // the objective needs every row of the shard
  const bool defer = MET && std::is_same<T, double>::value && (a.flags & F_LOSS) && a.defer_rows > 0;
  const size_t ub = defer ? ((size_t)a.defer_rows * (sizeof(T) + sizeof(S)) + 15) / 16 * 16 : 0;
  const size_t lds = (size_t)(KW + 1) * a.nchunks * VB + 2 * KW * sizeof(double) + ub;
  const size_t max_lds = 160 * 1024;
  if (lds > max_lds) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_round_local<T, S, CPL, PROB, MET>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  static const std::string name = [] {
    char buf[160];
    snprintf(buf, sizeof(buf), "void dopt::k_round_local<%s, %s, %d, %d, %s>(dopt::LocalArgs)",
             std::is_same<T, float>::value ? "float" : "double", std::is_same<S, float>::value ? "float" : "double",
             CPL, PROB, MET ? "true" : "false");
    return std::string(buf);
  }();
  note_round_kernel(name.c_str());
  hipLaunchKernelGGL((k_round_local<T, S, CPL, PROB, MET>), dim3(groups), dim3(KW * 64), lds, s, g);
  return hipGetLastError();
}

template <typename T, typename S, int CPL>
static hipError_t local_dispatch_mode(int problem, bool met, const LocalArgs& g, int groups, hipStream_t s) {
  if (problem == 0)
    return met ? launch_local_t<T, S, CPL, 0, true>(g, groups, s) : launch_local_t<T, S, CPL, 0, false>(g, groups, s);
  return met ? launch_local_t<T, S, CPL, 1, true>(g, groups, s) : launch_local_t<T, S, CPL, 1, false>(g, groups, s);
}

template <typename T, typename S>
static hipError_t local_dispatch_cpl(int problem, int cpl, bool met, const LocalArgs& g, int groups, hipStream_t s) {
  if (groups <= 0) return hipSuccess;
  switch (cpl) {
    case 1: return local_dispatch_mode<T, S, 1>(problem, met, g, groups, s);
    case 2: return local_dispatch_mode<T, S, 2>(problem, met, g, groups, s);
    case 4: return local_dispatch_mode<T, S, 4>(problem, met, g, groups, s);
    case 8: return local_dispatch_mode<T, S, 8>(problem, met, g, groups, s);
    case 16:
      // float64 state over float32 rows at 16 chunks per lane is beyond the register file, as for
      // k_round_gt (such rows are column-blocked contexts, which the local-steps round rejects)
      if constexpr (std::is_same<T, S>::value) return local_dispatch_mode<T, S, 16>(problem, met, g, groups, s);
      break;
  }
  return hipErrorInvalidValue;
}

}  // namespace dopt
