// k_round_saga.inc -- the fused GT-SAGA round (variance-reduced gradient tracking; Xin, Khan, Kar 2020)
// and its launch dispatch, included by one translation unit per (state, data) element-type pair
// (saga_f32.hip, saga_f64.hip, saga_x32.hip).  The losses are generalised linear, so the gradient of
// shard row j is c_j * row_j with a scalar c_j: the SAGA table holds one scalar per shard row (tab,
// [rows] T) and its mean gradient one state row per worker (gbar, [n x ld] T).  Per worker i with m
// rows, batch B of nb = min(b, m) distinct local rows, W the mixing matrix (CSR, diagonal included):
//   c_new_j = coef(x_i . row_j, y_j)                        j in B
//   s       = sum_{j in B} (c_new_j - tab[j]) * row_j       (row order of the batch, per wave)
//   g_new_i = s / nb + gbar_i + lam x_i                     (0, and tab / gbar untouched, for an empty shard)
//   gbar_i <- gbar_i + s / m;   tab[j] <- c_new_j           j in B
//   y_new_i = sum_j W_ij y_j + g_new_i - g_i;   x_new_i = sum_j W_ij x_j - eta y_new_i;   g_i <- g_new_i
// SagaArgs.init selects the second mode of the same kernel, the pass that opens a chain: every row
// of the shard with c_old = 0, the table stored, and gbar_i = s / m the only state written.
//
// One workgroup per worker, a row per wave at a time, as k_round_gt.  The algorithm lives at b << m
// (16 rows of 512), where a wave streams a handful of rows and everything around the stream is the
// cost, so:
//   * rows go to the waves round-robin (row r of the batch to wave r % KW): at b = 16 every one of the
//     4 waves has 4 rows and the first four rows of the batch are in flight before anything else;
//   * a wave's indices, labels and old table entries are not a chain per row: lane l of the wave
//     requests all three for the wave's l-th row up front (a WINDOW of 64 rows per wave; longer
//     streams refill it every 64 rows), the row loop takes them out with v_readlane, and the new
//     coefficients go back into the window's lanes and leave with one store per window -- lane l
//     stores the entry of its own row, a plain vector store.  Indices are distinct within a worker
//     and a round (the caller's contract) and only workgroup i touches tab_i, so the stores of a
//     round never meet its loads;
//   * the prologue, behind the first row request, forms mx[c] = (W x)[c] and my[c] = (W y)[c] - g_i[c]
//     in CSR order per owner thread (state chunk c = tid + q * threads) and parks them in two LDS rows;
//     gbar_i[c] stays in the owner's registers: the thread that loads it is the one that uses and
//     rewrites it, so a third LDS row would only add a store and a load per chunk (at most 4 chunks
//     of registers per thread);
//   * the epilogue folds the waves' partials in wave order and stores x_new, y_new, g and gbar: no
//     global read, no atomics, every sum in a fixed order -- run to run the bits are the same.
// Metrics as k_round_gt: the consensus of x_old at xbar is fused, the objective with full-shard
// batches only; a launch without F_STEP takes the metrics alone and leaves the table alone.
//
// LDS: [red: waves x nch state chunks] [mx: nch] [my: nch] [sred: 2 x waves doubles]
//      [ubuf / ybuf: the deferred objective terms' dots and labels (float64 arithmetic)]  (k_round_gt's plan)
namespace dopt {

template <typename T, typename S, int CPL>
constexpr int saga_waves() {
  return (CPL * (int)sizeof(typename KV<T, S>::V) / 16 <= 4) ? 2 * NW : NW;
}

template <typename T, typename S, int CPL, int PROB, bool MET>
__global__ __launch_bounds__((saga_waves<T, S, CPL>() * 64)) __attribute__((amdgpu_waves_per_eu(1))) void k_round_saga(
    const SagaArgs ga) {
  const RoundArgs& a = ga.r;
  constexpr int KW = saga_waves<T, S, CPL>();
  constexpr int KT = KW * 64;
  using V = typename KV<T, S>::V;    // state chunk (iterate, tracker, gradient, gbar, xbar)
  using VX = typename KV<T, S>::VX;  // data chunk (shard row)
  constexpr int VN = KV<T, S>::VN;
  constexpr bool DBL = std::is_same<T, double>::value;
  constexpr bool FAST = !DBL && PROB == 0;  // hardware exp / log / reciprocal for the float logistic terms
  constexpr bool PIPE = CPL <= 4;           // two row buffers fit the registers only there
  constexpr int CPT = (64 * CPL + KT - 1) / KT;  // state chunks of a row per thread
  constexpr int WIN = 64;                   // rows of a wave whose index, label and table entry sit in its lanes
  extern __shared__ __attribute__((aligned(32))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x;
  const int flags = a.flags;
  const int nch = a.nchunks;
  const int64_t ld = a.ld;
  const int64_t row0 = a.off[i];
  const int64_t m = a.off[i + 1] - row0;
  const bool init = ga.init != 0;  // the chain's opening pass: all rows, c_old = 0, gbar = s / m
  const bool step = (flags & F_STEP) != 0;
  const bool want_loss = MET && (flags & F_LOSS);  // full-shard batches only (host-checked)
  const bool want_cons = MET && (flags & F_CONS);
  const bool defer = MET && DBL && want_loss && a.defer_rows > 0;
  const int32_t* __restrict__ bidx = (a.idx && !init) ? a.idx + (int64_t)i * a.b : nullptr;
  const int64_t nb = bidx ? (a.b < m ? a.b : m) : m;
  const bool grad = step || init;  // the launch forms coefficients and writes the table
  const int64_t nrow = (grad || want_loss) ? nb : 0;
  // this wave's rows are wave, wave + KW, ...: nk of them, the k-th in lane k % WIN of its window
  const int nk = wave < nrow ? (int)((nrow - wave + KW - 1) / KW) : 0;
  const S* __restrict__ X = (const S*)a.X;
  const S* __restrict__ Yp = (const S*)a.y;
  T* __restrict__ tab = (T*)ga.tab + row0;
  const T* wsrc = (const T*)a.x_old + (int64_t)i * ld;

  V* red = (V*)smem;  // [KW][nch]
  V* mx = red + (size_t)KW * nch;
  V* my = mx + nch;
  double* sred = (double*)(my + nch);  // [2][KW]
  T* ubuf = (T*)(sred + 2 * KW);       // deferred objective terms: the row's dot with xbar ...
  S* ybuf = (S*)(ubuf + a.defer_rows);  // ... and its label, as stored

  // the window: lane l holds local row id, label and old table entry of the wave's row k0 + l
  int32_t wl = 0;
  T wy = T(0), wc = T(0), wn = T(0);
  auto fill = [&](int k0) {
    const int k = k0 + lane;
    wl = 0;
    wy = T(0);
    wc = T(0);
    if (k < nk) {
      const int64_t rr = wave + (int64_t)k * KW;
      wl = bidx ? bidx[rr] : (int32_t)rr;
      wy = (T)Yp[row0 + wl];
      if (step && !init) wc = tab[wl];
    }
  };
  auto load_row = [&](int k, VX (&dst)[CPL]) {
    const int32_t lr = __builtin_amdgcn_readlane(wl, k & (WIN - 1));
    const S* xp = X + (row0 + lr) * ld;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const int c = lane + 64 * j;
      const int cc = c < nch ? c : nch - 1;  // lanes past the row re-read its last chunk (w, xb are 0 there)
      dst[j] = __builtin_nontemporal_load((const VX*)(xp + (int64_t)cc * VN));
    }
  };
  VX cur[CPL], nxt[CPL];
  fill(0);  // the first window and the first row, ahead of everything else
  if (PIPE && nk > 0) load_row(0, cur);

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

  // owner thread of state chunk c = tid + q KT: gbar_i[c] into registers, sum_j W_ij x_j and
  // sum_j W_ij y_j - g_i (CSR order) into the two LDS rows
  V gb[CPT];
  T* gbp = (T*)ga.gbar + (int64_t)i * ld;
  if (step && !init) {
    const int64_t pe0 = a.rp[i], pe1 = a.rp[i + 1];
    const T* __restrict__ cw = (const T*)a.cw;
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = threadIdx.x + q * KT;
      gb[q] = V(0);
      if (c < nch) {
        const int64_t co = (int64_t)c * VN;
        gb[q] = *(const V*)(gbp + co);
        V ax = V(0), ay = V(0);
#pragma unroll 2
        for (int64_t e = pe0; e < pe1; ++e) {
          const T wt = cw[e];
          const int64_t ro = (int64_t)a.ci[e] * ld + co;
          ax += wt * *(const V*)((const T*)a.x_old + ro);
          ay += wt * *(const V*)((const T*)ga.y_old + ro);
        }
        ay -= *(const V*)((const T*)ga.g_prev + (int64_t)i * ld + co);
        mx[c] = ax;  // read back by this same thread in the epilogue
        my[c] = ay;
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < CPT; ++q) gb[q] = V(0);
  }

  double loss = 0.0;
  auto process = [&](VX (&rx)[CPL], int k) {
    const int wlane = k & (WIN - 1);
    const T yv = readlane_t(wy, wlane);
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
    if (grad) {
      T coef;
      if constexpr (FAST) coef = -yv * sigmoid_neg_fast(yv * z);
      else coef = (PROB == 0) ? -yv * sigmoid_neg(yv * z) : z - yv;
      const T dc = coef - readlane_t(wc, wlane);  // c_old = 0 in the opening pass
#pragma unroll
      for (int j = 0; j < CPL; ++j) g[j] += dc * rv[j];
      if (lane == wlane) wn = coef;
    }
    if constexpr (MET) {
      const int64_t rr = wave + (int64_t)k * KW;
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
  // the window's new coefficients: lane l stores the entry of its own row
  auto flush = [&](int k0) {
    if (grad && k0 + lane < nk) tab[wl] = wn;
  };
  for (int k0 = 0; k0 < nk; k0 += WIN) {
    const int k1 = k0 + WIN < nk ? k0 + WIN : nk;
    if (k0 > 0) {
      fill(k0);
      if (PIPE) load_row(k0, cur);
    }
    if constexpr (PIPE) {
      // peeled: every iteration requests the next row unconditionally, so the wait before the
      // current row's arithmetic covers that row only
      int k = k0;
      for (; k + 1 < k1; ++k) {
        load_row(k + 1, nxt);
        process(cur, k);
#pragma unroll
        for (int j = 0; j < CPL; ++j) cur[j] = nxt[j];
      }
      process(cur, k);
    } else {
      for (int k = k0; k < k1; ++k) {
        load_row(k, cur);
        process(cur, k);
      }
    }
    flush(k0);
  }

  if (grad) {
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

  if (grad) {
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
        const int64_t co = (int64_t)c * VN;
        if (init) {
          *(V*)(gbp + co) = (m > 0) ? s / (T)m : V(0);
          continue;
        }
        // chunk c = lane + 64 (wave + k KW) is this lane's w[wave + k KW]
        const int jj = wave + k * KW;
        V xc = w[0];
#pragma unroll
        for (int j = 1; j < CPL; ++j)
          if (j == jj) xc = w[j];
        const V gc = (nb > 0) ? (s / (T)nb + gb[k] + lam * xc) : V(0);
        const V ynew = my[c] + gc;
        *(V*)(xn + co) = mx[c] - eta * ynew;
        *(V*)(yn + co) = ynew;
        *(V*)(gp + co) = gc;
        if (nb > 0) *(V*)(gbp + co) = gb[k] + s / (T)m;
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
static hipError_t launch_saga_t(const SagaArgs& g, int groups, hipStream_t s) {
  constexpr int KW = saga_waves<T, S, CPL>();
  constexpr size_t VB = sizeof(typename KV<T, S>::V);
  const RoundArgs& a = g.r;
  if (a.nchunks < 1 || a.nchunks > 64 * CPL || !a.rp || !g.tab || !g.gbar) return hipErrorInvalidValue;
  if ((a.flags & F_LOSS) && a.idx) return hipErrorInvalidValue;  // the objective needs every row of the shard
  if (g.init && (a.flags & (F_LOSS | F_CONS))) return hipErrorInvalidValue;  // the opening pass takes no metrics
  const bool defer = MET && std::is_same<T, double>::value && (a.flags & F_LOSS) && a.defer_rows > 0;
  const size_t ub = defer ? ((size_t)a.defer_rows * (sizeof(T) + sizeof(S)) + 15) / 16 * 16 : 0;
  const size_t lds = (size_t)(KW + 2) * a.nchunks * VB + 2 * KW * sizeof(double) + ub;
  const size_t max_lds = 160 * 1024;
  if (lds > max_lds) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_round_saga<T, S, CPL, PROB, MET>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  static const std::string name = [] {
    char buf[160];
    snprintf(buf, sizeof(buf), "void dopt::k_round_saga<%s, %s, %d, %d, %s>(dopt::SagaArgs)",
             std::is_same<T, float>::value ? "float" : "double", std::is_same<S, float>::value ? "float" : "double",
             CPL, PROB, MET ? "true" : "false");
    return std::string(buf);
  }();
  note_round_kernel(name.c_str());
  hipLaunchKernelGGL((k_round_saga<T, S, CPL, PROB, MET>), dim3(groups), dim3(KW * 64), lds, s, g);
  return hipGetLastError();
}

template <typename T, typename S, int CPL>
static hipError_t saga_dispatch_mode(int problem, bool met, const SagaArgs& g, int groups, hipStream_t s) {
  if (problem == 0)
    return met ? launch_saga_t<T, S, CPL, 0, true>(g, groups, s) : launch_saga_t<T, S, CPL, 0, false>(g, groups, s);
  return met ? launch_saga_t<T, S, CPL, 1, true>(g, groups, s) : launch_saga_t<T, S, CPL, 1, false>(g, groups, s);
}

template <typename T, typename S>
static hipError_t saga_dispatch_cpl(int problem, int cpl, bool met, const SagaArgs& g, int groups, hipStream_t s) {
  if (groups <= 0) return hipSuccess;
  switch (cpl) {
    case 1: return saga_dispatch_mode<T, S, 1>(problem, met, g, groups, s);
    case 2: return saga_dispatch_mode<T, S, 2>(problem, met, g, groups, s);
    case 4: return saga_dispatch_mode<T, S, 4>(problem, met, g, groups, s);
    case 8: return saga_dispatch_mode<T, S, 8>(problem, met, g, groups, s);
    case 16:
      // float64 state over float32 rows at 16 chunks per lane is beyond the register file, as for
      // k_round (such rows are column-blocked contexts, which GT-SAGA rejects)
      if constexpr (std::is_same<T, S>::value) return saga_dispatch_mode<T, S, 16>(problem, met, g, groups, s);
      break;
  }
  return hipErrorInvalidValue;
}

}  // namespace dopt
