// k_round_gt.inc -- the fused gradient-tracking round (DIGing / DSGT) and its launch dispatch,
// included by one translation unit per (state, data) element-type pair (gt_f32.hip, gt_f64.hip,
// gt_x32.hip).  Per worker i, with W the mixing matrix (CSR, diagonal included):
//   g_new_i = grad f_i(x_i; minibatch)      (worker.py:30-44, regulariser included; 0 for an empty shard)
//   y_new_i = sum_j W_ij y_j + g_new_i - g_i
//   x_new_i = sum_j W_ij x_j - eta y_new_i
//   g_i <- g_new_i
// i.e. x_{t+1} = W x_t - eta_t y_t, y_{t+1} = W y_t + g_{t+1} - g_t, y_0 = g_0, reordered so that
// y_new_i needs only the neighbours' OLD y and x_new_i only the worker's own y_new_i: one launch per
// round, x and y ping-pong, g is updated in place (only workgroup i touches row i of g).
//
// One workgroup per worker.  Every wave streams whole shard rows (non-temporal 16-byte loads, the
// next row requested before the current row's arithmetic, branch-free and peeled as in k_round) and
// holds the iterate, xbar and its gradient partial in registers; the row's two dots (x . w for the
// gradient, x . xbar for the objective of the previous round) go through one paired butterfly.
//
// The two mixes do not depend on the row stream, so they are formed in the PROLOGUE, behind each
// wave's first row request: thread tid owns state chunks c = tid + q * threads, accumulates
//   mx[c] = sum_j W_ij x_j[c],   my[c] = sum_j W_ij y_j[c] - g_i[c]
// over the worker's CSR row in CSR order (the left-to-right order of mix_chunk) and parks them in
// two state rows of LDS -- 2 rows whatever the degree (k_round stages deg + 1 rows per matrix and
// caps the degree at 6).  The epilogue folds the waves' gradient partials in wave order, takes the
// worker's own iterate from the registers that hold it and mx / my from LDS, and stores x_new,
// y_new and g: it reads no global memory.  GtArgs.epi_mix moves the same two sums into the
// epilogue (through L2, as mix_chunk does) for the A/B of DESIGN.md 6f; the bits are the same.
//
// LDS: [red: waves x nch state chunks] [mx: nch] [my: nch] [sred: 2 x waves doubles]
//      [ubuf / ybuf: the deferred objective terms' dots and labels (float64 arithmetic)]
// Largest row-resident case (1024 chunks of 16 bytes, or 512 of 32; 4 waves): 64 + 32 KiB, + 16 KiB
// of deferred terms at 1024 rows per shard = 112 KiB of the 160 KiB requested.
namespace dopt {

// Waves per workgroup: 8 while the three register-resident state vectors take <= 4 16-byte
// registers per lane each, else 4 (float64 state over float32 rows counts its 32-byte state chunks
// twice: k_round measured 8 waves slower there).
template <typename T, typename S, int CPL>
constexpr int gt_waves() {
  return (CPL * (int)sizeof(typename KV<T, S>::V) / 16 <= 4) ? 2 * NW : NW;
}

template <typename T, typename S, int CPL, int PROB, bool MET>
__global__ __launch_bounds__((gt_waves<T, S, CPL>() * 64)) __attribute__((amdgpu_waves_per_eu(1))) void k_round_gt(
    const GtArgs ga) {
  const RoundArgs& a = ga.r;
  constexpr int KW = gt_waves<T, S, CPL>();
  constexpr int KT = KW * 64;
  using V = typename KV<T, S>::V;    // state chunk (iterate, tracker, gradient, xbar)
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
  // run's last round): the same row arithmetic, no mix and no store
  const bool step = (flags & F_STEP) != 0;
  const bool want_loss = MET && (flags & F_LOSS);  // full-shard batches only (host-checked)
  const bool want_cons = MET && (flags & F_CONS);
  const bool defer = MET && DBL && want_loss && a.defer_rows > 0;
  const int64_t nrow = (step || want_loss) ? nb : 0;
  const S* __restrict__ X = (const S*)a.X;
  const S* __restrict__ Yp = (const S*)a.y;
  const int32_t* __restrict__ bidx = a.idx ? a.idx + (int64_t)i * a.b : nullptr;
  const T* wsrc = (const T*)a.x_old + (int64_t)i * ld;

  V* red = (V*)smem;  // [KW][nch]
  V* mx = red + (size_t)KW * nch;
  V* my = mx + nch;
  double* sred = (double*)(my + nch);  // [2][KW]
  T* ubuf = (T*)(sred + 2 * KW);       // deferred objective terms: the row's dot with xbar ...
  S* ybuf = (S*)(ubuf + a.defer_rows);  // ... and its label, as stored

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
    const bool in = c < nch;
    w[j] = in ? *(const V*)(wsrc + (int64_t)c * VN) : V(0);
    xb[j] = (MET && need_xb && in) ? *(const V*)((const T*)a.xbar + (int64_t)c * VN) : V(0);
    g[j] = V(0);
  }

  // sum_j W_ij x_j and sum_j W_ij y_j - g_i of state chunk c, CSR order
  const int64_t pe0 = a.rp[i], pe1 = a.rp[i + 1];
  const T* __restrict__ cw = (const T*)a.cw;
  auto mix2 = [&](int c, V& ax, V& ay) {
    ax = V(0);
    ay = V(0);
    const int64_t co = (int64_t)c * VN;
#pragma unroll 2
    for (int64_t e = pe0; e < pe1; ++e) {
      const T wt = cw[e];
      const int64_t ro = (int64_t)a.ci[e] * ld + co;
      ax += wt * *(const V*)((const T*)a.x_old + ro);
      ay += wt * *(const V*)((const T*)ga.y_old + ro);
    }
    ay -= *(const V*)((const T*)ga.g_prev + (int64_t)i * ld + co);
  };
  if (step && !ga.epi_mix) {
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = threadIdx.x + q * KT;
      if (c < nch) {
        V ax, ay;
        mix2(c, ax, ay);
        mx[c] = ax;  // read back by this same thread in the epilogue
        my[c] = ay;
      }
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
  __syncthreads();

  if (step) {
    const T eta = (T)a.eta;
    const T lam = (T)a.lam;
    T* xn = (T*)a.x_new + (int64_t)i * ld;
    T* yn = (T*)ga.y_new + (int64_t)i * ld;
    T* gp = (T*)ga.g_prev + (int64_t)i * ld;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const int c = threadIdx.x + k * KT;
      if (c < nch) {
        V s = red[c];
#pragma unroll
        for (int q = 1; q < KW; ++q) s += red[(size_t)q * nch + c];  // fixed order
        // chunk c = lane + 64 (wave + k KW) is this lane's w[wave + k KW]
        const int jj = wave + k * KW;
        V wc = w[0];
#pragma unroll
        for (int j = 1; j < CPL; ++j)
          if (j == jj) wc = w[j];
        const V gc = (nb > 0) ? (s / (T)nb + lam * wc) : V(0);
        V ax, ay;
        if (ga.epi_mix) {
          mix2(c, ax, ay);
        } else {
          ax = mx[c];
          ay = my[c];
        }
        const V ynew = ay + gc;
        const int64_t co = (int64_t)c * VN;
        *(V*)(xn + co) = ax - eta * ynew;
        *(V*)(yn + co) = ynew;
        *(V*)(gp + co) = gc;
      }
    }
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

template <typename T, typename S, int CPL, int PROB, bool MET>
static hipError_t launch_gt_t(const GtArgs& g, int groups, hipStream_t s) {
  constexpr int KW = gt_waves<T, S, CPL>();
  constexpr size_t VB = sizeof(typename KV<T, S>::V);
  const RoundArgs& a = g.r;
  if (a.nchunks < 1 || a.nchunks > 64 * CPL || !a.rp) return hipErrorInvalidValue;
  if ((a.flags & F_LOSS) && a.idx) return hipErrorInvalidValue;  // the objective needs every row of the shard
  const bool defer = MET && std::is_same<T, double>::value && (a.flags & F_LOSS) && a.defer_rows > 0;
  const size_t ub = defer ? ((size_t)a.defer_rows * (sizeof(T) + sizeof(S)) + 15) / 16 * 16 : 0;
  const size_t lds = (size_t)(KW + 2) * a.nchunks * VB + 2 * KW * sizeof(double) + ub;
  const size_t max_lds = 160 * 1024;
  if (lds > max_lds) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_round_gt<T, S, CPL, PROB, MET>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  static const std::string name = [] {
    char buf[160];
    snprintf(buf, sizeof(buf), "void dopt::k_round_gt<%s, %s, %d, %d, %s>(dopt::GtArgs)",
             std::is_same<T, float>::value ? "float" : "double", std::is_same<S, float>::value ? "float" : "double",
             CPL, PROB, MET ? "true" : "false");
    return std::string(buf);
  }();
  note_round_kernel(name.c_str());
  hipLaunchKernelGGL((k_round_gt<T, S, CPL, PROB, MET>), dim3(groups), dim3(KW * 64), lds, s, g);
  return hipGetLastError();
}

template <typename T, typename S, int CPL>
static hipError_t gt_dispatch_mode(int problem, bool met, const GtArgs& g, int groups, hipStream_t s) {
  if (problem == 0) return met ? launch_gt_t<T, S, CPL, 0, true>(g, groups, s) : launch_gt_t<T, S, CPL, 0, false>(g, groups, s);
  return met ? launch_gt_t<T, S, CPL, 1, true>(g, groups, s) : launch_gt_t<T, S, CPL, 1, false>(g, groups, s);
}

template <typename T, typename S>
static hipError_t gt_dispatch_cpl(int problem, int cpl, bool met, const GtArgs& g, int groups, hipStream_t s) {
  if (groups <= 0) return hipSuccess;
  switch (cpl) {
    case 1: return gt_dispatch_mode<T, S, 1>(problem, met, g, groups, s);
    case 2: return gt_dispatch_mode<T, S, 2>(problem, met, g, groups, s);
    case 4: return gt_dispatch_mode<T, S, 4>(problem, met, g, groups, s);
    case 8: return gt_dispatch_mode<T, S, 8>(problem, met, g, groups, s);
    case 16:
      // float64 state over float32 rows at 16 chunks per lane is beyond the register file, as for
      // k_round (such rows are column-blocked contexts, which gradient tracking rejects)
      if constexpr (std::is_same<T, S>::value) return gt_dispatch_mode<T, S, 16>(problem, met, g, groups, s);
      break;
  }
  return hipErrorInvalidValue;
}

}  // namespace dopt
