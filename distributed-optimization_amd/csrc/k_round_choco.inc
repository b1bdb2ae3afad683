// k_round_choco.inc -- the fused CHOCO-SGD round (top-k compressed gossip with error feedback) and its
// launch dispatch, included by one translation unit per (state, data) element-type pair
// (choco_f32.hip, choco_f64.hip, choco_x32.hip).  Per worker i, with W the mixing matrix (CSR,
// diagonal included), xhat_i the worker's public copy and k, gamma the compression parameters:
//   g_i      = grad f_i(x_i; minibatch)      (worker.py:30-44, regulariser included; 0 for an empty shard)
//   x_new_i  = x_i - eta g_i + gamma (sum_j W_ij xhat_j - xhat_i)        (the OLD public copies)
//   v_i      = x_new_i - xhat_i
//   q_i      = top_k(v_i)    the k entries of largest |v|, equal magnitudes by lower column, rest 0
//   xhat_i  <- xhat_i + q_i,  x_i <- x_new_i
// x_new_i and the new xhat_i need only the neighbours' OLD xhat: one launch per round, x and xhat
// ping-pong.
//
// One workgroup per worker.  The row stream is k_round_gt's: every wave streams whole shard rows
// (non-temporal 16-byte loads, the next row requested before the current row's arithmetic,
// branch-free and peeled) and holds the iterate, xbar and its gradient partial in registers; the
// row's two dots go through one paired butterfly.
//
// PROLOGUE, behind each wave's first row request: thread tid owns state chunks c = tid + q * threads,
// forms mh[c] = gamma (sum_j W_ij xhat_j[c] - xhat_i[c]) over the worker's CSR row in CSR order and
// parks it and the own xhat_i[c] in two state rows of LDS -- 2 rows whatever the degree; the
// epilogue reads no global memory.
//
// EPILOGUE 1: the waves' gradient partials folded in wave order, x_new stored, v kept in registers.
// EPILOGUE 2, the selection: a workgroup-wide radix select on the magnitude bit pattern of v (the
// sign-cleared 32- / 64-bit integer, whose order is the order of |v|), most-significant byte first.
// Every pass adds the still-candidate elements (those that match the threshold's bytes found so
// far) into ONE 256-bin LDS histogram with vector LDS integer adds -- integer sums, so the bins do
// not depend on the arrival order -- and, after one barrier, EVERY wave scans the histogram top
// down for itself (4 bins per lane, a suffix sum by shuffles): the bin that holds the k-th largest
// candidate gives the threshold's next byte and the remainder kk = k - #{elements above the bin}.
// Nobody broadcasts, so a pass costs one barrier; three histograms rotate so that the next pass's
// bins are cleared before that barrier while no wave can still be reading them.  The passes stop as
// soon as the bin's whole population is taken (kk == its count: no remainder to split).  Otherwise
// the elements that match the threshold are taken in ascending column order until kk are taken:
// an exclusive scan of the threads' match counts in the order (q, tid, element of the chunk), which
// is column order -- shuffles inside a wave, the waves' totals through LDS.  Then
// xhat_new = xhat_i + (selected ? v : 0), vector stores.  Padding columns hold v = 0 and xhat = 0:
// whether or not they are taken they stay 0.
//
// No atomics on global memory; every sum has a fixed order or is an integer: two runs give the same bits.
//
// LDS: [red: waves x nch state chunks] [mh: nch] [xh: nch] [sred: 2 x waves doubles]
//      [hist: 3 x 256 ints] [wtot: 16 ints] [ubuf / ybuf: deferred objective terms]
// ChocoArgs.wave_hist gives every wave a sub-histogram of its own, summed by the scan (3 x waves x 256
// ints), for the A/B of DESIGN.md 6g: the same bits, and not faster, so one shared histogram is the default.
// C3 (256 chunks of 32 bytes, 4 waves, 512 rows deferred): 32 + 16 KiB + 3.2 KiB + 6 KiB = 57 KiB.
// Largest row-resident case (16 KiB per state row, 4 waves, 1024 rows deferred):
// 64 + 32 KiB + 3.2 KiB + 16 KiB = 115 KiB of the 160 KiB requested.
namespace dopt {

constexpr int kChocoBins = 256;
// three rotating histograms of nh sub-histograms each + the tie scan's 16 wave totals
constexpr int choco_scratch(int nh) { return (3 * nh * kChocoBins + 16) * (int)sizeof(int); }

template <typename T, typename S, int CPL>
constexpr int choco_waves() {  // the rule of k_round_gt
  return (CPL * (int)sizeof(typename KV<T, S>::V) / 16 <= 4) ? 2 * NW : NW;
}

// The magnitude of x as an integer whose order is the order of |x|: the bit pattern without the sign.
// By value: the argument is a scalar copy of the vector element (a bit cast of the element
// expression itself reads the vector's first element).
__device__ __forceinline__ uint32_t choco_key(float x) { return __builtin_bit_cast(uint32_t, x) & 0x7fffffffu; }
__device__ __forceinline__ uint64_t choco_key(double x) {
  return __builtin_bit_cast(uint64_t, x) & 0x7fffffffffffffffull;
}

template <typename T, typename S, int CPL, int PROB, bool MET>
__global__ __launch_bounds__((choco_waves<T, S, CPL>() * 64)) __attribute__((amdgpu_waves_per_eu(1))) void k_round_choco(
    const ChocoArgs ca) {
  const RoundArgs& a = ca.r;
  constexpr int KW = choco_waves<T, S, CPL>();
  constexpr int KT = KW * 64;
  using V = typename KV<T, S>::V;    // state chunk (iterate, public copy, gradient, xbar)
  using VX = typename KV<T, S>::VX;  // data chunk (shard row)
  constexpr int VN = KV<T, S>::VN;
  constexpr bool DBL = std::is_same<T, double>::value;
  constexpr bool FAST = !DBL && PROB == 0;  // hardware exp / log / reciprocal for the float logistic terms
  constexpr bool PIPE = CPL <= 4;           // two row buffers fit the registers only there
  constexpr int CPT = (64 * CPL + KT - 1) / KT;  // state chunks of a row per thread
  static_assert(CPT * KW <= 16, "wtot holds 16 wave totals");
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
  // run's last round): the same row arithmetic, no mix, no selection and no store
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
  V* mh = red + (size_t)KW * nch;
  V* xh = mh + nch;
  double* sred = (double*)(xh + nch);  // [2][KW]
  // ChocoArgs.wave_hist (A/B of DESIGN.md 6g): a sub-histogram per wave, summed by the scan (same bits)
  const int nh = ca.wave_hist ? KW : 1;
  const int hsz = nh * kChocoBins;
  int* hist = (int*)(sred + 2 * KW);   // [3][nh][256]
  int* wtot = hist + 3 * hsz;          // [16]
  T* ubuf = (T*)(wtot + 16);           // deferred objective terms: the row's dot with xbar ...
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

  if (step) {  // gamma (sum_j W_ij xhat_j - xhat_i) per owned chunk, CSR order; read back by this same thread
    const int64_t pe0 = a.rp[i], pe1 = a.rp[i + 1];
    const T* __restrict__ cw = (const T*)a.cw;
    const T* __restrict__ xho = (const T*)ca.xhat_old;
    const T gamma = (T)ca.gamma;
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = threadIdx.x + q * KT;
      if (c < nch) {
        const int64_t co = (int64_t)c * VN;
        V acc = V(0);
#pragma unroll 2
        for (int64_t e = pe0; e < pe1; ++e) acc += cw[e] * *(const V*)(xho + (int64_t)a.ci[e] * ld + co);
        const V own = *(const V*)(xho + (int64_t)i * ld + co);
        mh[c] = gamma * (acc - own);
        xh[c] = own;
      }
    }
    for (int j = threadIdx.x; j < hsz; j += KT) hist[j] = 0;  // the first pass's bins
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
    using U = typename std::conditional<DBL, uint64_t, uint32_t>::type;
    constexpr int NB = (int)sizeof(T);  // key bytes = passes at most
    const T eta = (T)a.eta;
    const T lam = (T)a.lam;
    T* xn = (T*)a.x_new + (int64_t)i * ld;
    V v[CPT];  // x_new - xhat of the owned chunks (0 past the row)
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = threadIdx.x + q * KT;
      v[q] = V(0);
      if (c < nch) {
        V s = red[c];
#pragma unroll
        for (int p = 1; p < KW; ++p) s += red[(size_t)p * nch + c];  // fixed order
        // chunk c = lane + 64 (wave + q KW) is this lane's w[wave + q KW]
        const int jj = wave + q * KW;
        V wc = w[0];
#pragma unroll
        for (int j = 1; j < CPL; ++j)
          if (j == jj) wc = w[j];
        const V gc = (nb > 0) ? (s / (T)nb + lam * wc) : V(0);
        const V xnew = wc - eta * gc + mh[c];
        v[q] = xnew - xh[c];
        *(V*)(xn + (int64_t)c * VN) = xnew;
      }
    }

    // radix select: thr = the threshold's bytes found so far (those above `shift`), kk = how many
    // of the elements that match them are still to take, grp = how many match them
    U thr = 0;
    int kk = ca.k, grp = 0, shift = 0;
#pragma unroll 1
    for (int p = 0; p < NB; ++p) {
      shift = (NB - 1 - p) * 8;
      int* h = hist + (p % 3) * hsz;
      int* hw = h + (nh > 1 ? wave * kChocoBins : 0);
#pragma unroll
      for (int q = 0; q < CPT; ++q) {
        if (threadIdx.x + q * KT < nch) {
#pragma unroll
          for (int e = 0; e < VN; ++e) {
            const T ve = v[q][e];
            const U key = choco_key(ve);
            const bool cand = p == 0 || (((key ^ thr) >> shift) >> 8) == 0;
            if (cand) atomicAdd(&hw[(int)(key >> shift) & 255], 1);  // ds_add_u32, no return
          }
        }
      }
      // the next pass's bins: last read two passes ago, i.e. before the previous barrier
      for (int j = threadIdx.x; j < hsz; j += KT) hist[((p + 1) % 3) * hsz + j] = 0;
      __syncthreads();
      // top-down scan, every wave for itself: lane l holds bins 4 l .. 4 l + 3
      int4 hv = *(const int4*)(h + 4 * lane);
      for (int s = 1; s < nh; ++s) {
        const int4 t = *(const int4*)(h + s * kChocoBins + 4 * lane);
        hv.x += t.x;
        hv.y += t.y;
        hv.z += t.z;
        hv.w += t.w;
      }
      const int own = hv.x + hv.y + hv.z + hv.w;
      int suf = own;  // candidates in this lane's bins and above
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(suf, o, 64);
        if (lane + o < 64) suf += t;
      }
      int above = suf - own;
      const bool here = above < kk && kk <= suf;  // exactly one lane: the k-th largest is in its bins
      int bin = 4 * lane + 3, cnt = hv.w;
      if (above + cnt < kk) { above += cnt; bin = 4 * lane + 2; cnt = hv.z; }
      if (bin == 4 * lane + 2 && above + cnt < kk) { above += cnt; bin = 4 * lane + 1; cnt = hv.y; }
      if (bin == 4 * lane + 1 && above + cnt < kk) { above += cnt; bin = 4 * lane; cnt = hv.x; }
      const unsigned long long where = __ballot(here);
      const int src = where ? __ffsll((long long)where) - 1 : 0;
      bin = __shfl(bin, src, 64);
      above = __shfl(above, src, 64);
      grp = __shfl(cnt, src, 64);
      thr |= (U)bin << shift;
      kk -= above;
      if (kk == grp) break;  // the whole bin is taken: nothing left to split (uniform: every wave read the same bins)
    }

    // elements above the threshold prefix are taken; those that match it, in column order until kk are taken
    const U tp = thr >> shift;
    int before[CPT];
#pragma unroll
    for (int q = 0; q < CPT; ++q) before[q] = 0;
    if (kk != grp) {  // uniform
#pragma unroll
      for (int q = 0; q < CPT; ++q) {
        int n = 0;
#pragma unroll
        for (int e = 0; e < VN; ++e) {
          const T ve = v[q][e];
          n += (choco_key(ve) >> shift) == tp;
        }
        if (threadIdx.x + q * KT >= nch) n = 0;
        int inc = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(inc, o, 64);
          if (lane >= o) inc += t;
        }
        before[q] = inc - n;
        if (lane == 63) wtot[q * KW + wave] = inc;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < CPT; ++q) {
        const int upto = q * KW + wave;  // (q, wave) pairs before this one: lower columns
        for (int j = 0; j < upto; ++j) before[q] += wtot[j];
      }
    }
    const bool all = kk == grp;
    T* hn = (T*)ca.xhat_new + (int64_t)i * ld;
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      const int c = threadIdx.x + q * KT;
      if (c < nch) {
        V out = xh[c];
        int seen = before[q];
#pragma unroll
        for (int e = 0; e < VN; ++e) {
          const T ve = v[q][e];
          const U hk = choco_key(ve) >> shift;
          bool take = hk > tp;
          if (hk == tp) {
            take = all || seen < kk;
            ++seen;
          }
          out[e] += take ? ve : T(0);
        }
        *(V*)(hn + (int64_t)c * VN) = out;
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
static hipError_t launch_choco_t(const ChocoArgs& g, int groups, hipStream_t s) {
  constexpr int KW = choco_waves<T, S, CPL>();
  constexpr size_t VB = sizeof(typename KV<T, S>::V);
  const RoundArgs& a = g.r;
  if (a.nchunks < 1 || a.nchunks > 64 * CPL || !a.rp) return hipErrorInvalidValue;
  if ((a.flags & F_LOSS) && a.idx) return hipErrorInvalidValue;  // the objective needs every row of the shard
  if ((a.flags & F_STEP) && (g.k < 1 || (int64_t)g.k > (int64_t)a.nchunks * KV<T, S>::VN || !g.xhat_old || !g.xhat_new))
    return hipErrorInvalidValue;
  const bool defer = MET && std::is_same<T, double>::value && (a.flags & F_LOSS) && a.defer_rows > 0;
  const size_t ub = defer ? ((size_t)a.defer_rows * (sizeof(T) + sizeof(S)) + 15) / 16 * 16 : 0;
  // partial rows, two state rows, wave sums, histograms and scan scratch, deferred terms
  const size_t lds = (size_t)(KW + 2) * a.nchunks * VB + 2 * KW * sizeof(double) + choco_scratch(g.wave_hist ? KW : 1) + ub;
  const size_t max_lds = 160 * 1024;
  if (lds > max_lds) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_round_choco<T, S, CPL, PROB, MET>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  static const std::string name = [] {
    char buf[160];
    snprintf(buf, sizeof(buf), "void dopt::k_round_choco<%s, %s, %d, %d, %s>(dopt::ChocoArgs)",
             std::is_same<T, float>::value ? "float" : "double", std::is_same<S, float>::value ? "float" : "double",
             CPL, PROB, MET ? "true" : "false");
    return std::string(buf);
  }();
  note_round_kernel(name.c_str());
  hipLaunchKernelGGL((k_round_choco<T, S, CPL, PROB, MET>), dim3(groups), dim3(KW * 64), lds, s, g);
  return hipGetLastError();
}

template <typename T, typename S, int CPL>
static hipError_t choco_dispatch_mode(int problem, bool met, const ChocoArgs& g, int groups, hipStream_t s) {
  if (problem == 0)
    return met ? launch_choco_t<T, S, CPL, 0, true>(g, groups, s) : launch_choco_t<T, S, CPL, 0, false>(g, groups, s);
  return met ? launch_choco_t<T, S, CPL, 1, true>(g, groups, s) : launch_choco_t<T, S, CPL, 1, false>(g, groups, s);
}

template <typename T, typename S>
static hipError_t choco_dispatch_cpl(int problem, int cpl, bool met, const ChocoArgs& g, int groups, hipStream_t s) {
  if (groups <= 0) return hipSuccess;
  switch (cpl) {
    case 1: return choco_dispatch_mode<T, S, 1>(problem, met, g, groups, s);
    case 2: return choco_dispatch_mode<T, S, 2>(problem, met, g, groups, s);
    case 4: return choco_dispatch_mode<T, S, 4>(problem, met, g, groups, s);
    case 8: return choco_dispatch_mode<T, S, 8>(problem, met, g, groups, s);
    case 16:
      // float64 state over float32 rows at 16 chunks per lane is beyond the register file, as for
      // k_round (such rows are column-blocked contexts, which the CHOCO round rejects)
      if constexpr (std::is_same<T, S>::value) return choco_dispatch_mode<T, S, 16>(problem, met, g, groups, s);
      break;
  }
  return hipErrorInvalidValue;
}

}  // namespace dopt
