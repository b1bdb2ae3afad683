// k_round_sparse.inc -- the fused D-SGD round over shards stored in CSR and its launch dispatch,
// included by one translation unit per (state, value) element-type pair (sparse_f32.hip,
// sparse_f64.hip, sparse_x32.hip).  Per worker i, with W the mixing matrix (CSR, diagonal included):
//   z = X_i x_i (batch rows),  r_k = -y_k sigma(-y_k z_k) | z_k - y_k   (obj_problems.py; 0 off the batch)
//   g_i = X_i^T r / b + lam x_i                                          (0 for an empty shard)
//   x_new_i = sum_j W_ij x_j - eta g_i
// A sparse round is two sparse products around a dense mix over a state row of d elements, d up to
// 2^20: nothing of the dense row stream (row loads, the iterate in registers, a butterfly per row)
// carries over.  One workgroup of 4 waves per worker, four phases:
//   1 rows     a wave per batch row: lanes stride over the row's non-zeros and gather x_i[col] (and
//              xbar[col] for the objective) from global memory; fixed-order wave sum; the residual
//              r_k goes to an LDS array indexed by LOCAL ROW, zeroed first
//   2 dense    every 16-byte chunk of the state row: x_new = mix - eta lam x_i, mix over the CSR row
//              of W in CSR order; kSpU chunks per thread are in flight per CSR entry, so the loads of
//              a chunk group are independent of each other (the k_mix pattern); the chunk's
//              ||x_i - xbar||^2 feeds the consensus
//   barrier
//   3 columns  the shard's COLUMN VIEW (the same non-zeros sorted by column, doubly compressed: only
//              the columns the shard touches): g_c = sum_e sval[e] r[srow[e]] in stored order -- one
//              thread per short column, one wave per long column (lanes stride, fixed-order wave sum)
//              -- then x_new[c] is RECOMPUTED from the round's inputs, mix[c] - eta (g_c / b + lam
//              x_i[c]) with a scalar gather of the neighbours' x_j[c], and stored over phase 2's value
// The scatter g = X^T r therefore needs no atomics: every support column has one owner that sums it
// in a fixed order, and phase 3 only overwrites (it never reads x_new), so no thread reads back a
// value the same launch wrote.  Two runs give the same bits.
//
// LDS: [sred: 2 x waves doubles] [r: max_m T]  (max_m <= 16384: 128 KiB of float64)
namespace dopt {

constexpr int kSpU = 4;  // state chunks per thread per step of the dense pass

template <typename T, typename S, int PROB>
__global__ __launch_bounds__(NT) void k_round_sparse(const SparseArgs sa) {
  const RoundArgs& a = sa.r;
  using V = typename VT<T>::v;  // 16-byte state chunk
  constexpr int VN = VT<T>::n;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* sred = (double*)smem;   // [2][NW]: consensus, loss
  T* rres = (T*)(sred + 2 * NW);  // [max_m] residuals by local row

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = blockIdx.x;
  const int flags = a.flags;
  const int64_t ld = a.ld;
  const int64_t row0 = a.off[i];
  const int64_t m = a.off[i + 1] - row0;
  const int64_t nb = a.idx ? (a.b < m ? a.b : m) : m;
  // without F_STEP the launch only takes the metrics at xbar: the same row and chunk arithmetic, no
  // residuals, no mix and no store
  const bool step = (flags & F_STEP) != 0;
  const bool want_loss = (flags & F_LOSS) != 0;  // every row of the shard (host-checked: no idx)
  const bool want_cons = (flags & F_CONS) != 0;
  const T* __restrict__ xi = (const T*)a.x_old + (int64_t)i * ld;
  const T* __restrict__ xbar = (const T*)a.xbar;
  const S* __restrict__ Yp = (const S*)a.y + row0;
  const int64_t* __restrict__ rp = sa.row_ptr + row0;
  const int32_t* __restrict__ col = sa.col;
  const S* __restrict__ val = (const S*)sa.val;
  const int32_t* __restrict__ bidx = a.idx ? a.idx + (int64_t)i * a.b : nullptr;

  // ---- phase 1: rows
  if (step) {
    for (int64_t r = tid; r < m; r += NT) rres[r] = T(0);
    __syncthreads();
  }
  double loss = 0.0;
  const int64_t nrow = (step || want_loss) ? nb : 0;
  if (wave < nrow) {
    int64_t lr = bidx ? bidx[wave] : wave;
    int64_t p0 = rp[lr], p1 = rp[lr + 1];
    for (int64_t rr = wave; rr < nrow; rr += NW) {
      // the next row's extent, requested before this row's gathers
      const int64_t rn = rr + NW < nrow ? rr + NW : rr;
      const int64_t lrn = bidx ? bidx[rn] : rn;
      const int64_t q0 = rp[lrn], q1 = rp[lrn + 1];
      const T yv = (T)Yp[lr];
      T z = T(0), u = T(0);
      for (int64_t e = p0 + lane; e < p1; e += 128) {  // two non-zeros per lane in flight
        const bool two = e + 64 < p1;
        const int64_t e2 = two ? e + 64 : e;
        const int32_t c1 = col[e], c2 = col[e2];
        const T v1 = (T)val[e], v2 = two ? (T)val[e2] : T(0);
        if (step) {
          const T x1 = xi[c1], x2 = xi[c2];
          z += v1 * x1;
          z += v2 * x2;
        }
        if (want_loss) {
          const T b1 = xbar[c1], b2 = xbar[c2];
          u += v1 * b1;
          u += v2 * b2;
        }
      }
      if (step) {
        z = wave_sum(z);
        const T coef = (PROB == 0) ? -yv * sigmoid_neg(yv * z) : z - yv;
        if (lane == 0) rres[lr] = coef;
      }
      if (want_loss) {
        u = wave_sum(u);
        loss += row_loss<T, PROB>(yv, u);  // per wave in row order
      }
      lr = lrn;
      p0 = q0;
      p1 = q1;
    }
  }

  // ---- phase 2: dense
  const int nch = a.nchunks;
  const T eta = (T)a.eta;
  const T lam = nb > 0 ? (T)a.lam : T(0);  // an empty shard's gradient is 0, regulariser included
  const int64_t pe0 = a.rp[i], pe1 = a.rp[i + 1];
  const T* __restrict__ cw = (const T*)a.cw;
  const int32_t* __restrict__ ci = a.ci;
  const T* __restrict__ xo = (const T*)a.x_old;
  T* xn = (T*)a.x_new + (int64_t)i * ld;
  double cons = 0.0;
  if (step || want_cons) {
    for (int c0 = tid; c0 < nch; c0 += kSpU * NT) {
      int64_t co[kSpU];  // chunks past the row re-read its last chunk and store nothing
      V own[kSpU], xb[kSpU], acc[kSpU];
#pragma unroll
      for (int q = 0; q < kSpU; ++q) {
        const int c = c0 + q * NT;
        co[q] = (int64_t)(c < nch ? c : nch - 1) * VN;
        own[q] = *(const V*)(xi + co[q]);
        xb[q] = want_cons ? *(const V*)(xbar + co[q]) : V(0);
        acc[q] = V(0);
      }
      if (step) {
#pragma unroll 2
        for (int64_t e = pe0; e < pe1; ++e) {  // CSR order, as mix_chunk
          const T wt = cw[e];
          const T* src = xo + (int64_t)ci[e] * ld;
#pragma unroll
          for (int q = 0; q < kSpU; ++q) acc[q] += wt * *(const V*)(src + co[q]);
        }
#pragma unroll
        for (int q = 0; q < kSpU; ++q)
          if (c0 + q * NT < nch) *(V*)(xn + co[q]) = acc[q] - eta * (lam * own[q]);
      }
      if (want_cons) {
#pragma unroll
        for (int q = 0; q < kSpU; ++q)
          if (c0 + q * NT < nch) {
            const V dv = own[q] - xb[q];
            cons += (double)hsum<T>(dv * dv);
          }
      }
    }
  }
  cons = wave_sum(cons);
  if (lane == 0) {
    sred[wave] = cons;
    sred[NW + wave] = loss;
  }
  __syncthreads();  // the residuals are complete, and phase 2's stores precede phase 3's to the same columns

  if (tid == 0) {
    double cs = 0.0, ls = 0.0;
#pragma unroll
    for (int q = 0; q < NW; ++q) {  // wave order
      cs += sred[q];
      ls += sred[NW + q];
    }
    if (want_cons) a.slab_cons[i] = cs;
    if (want_loss) a.slab_loss[i] = ls;
  }

  // ---- phase 3: support columns (a minibatch round still walks all of them: r = 0 off the batch)
  if (!step || nb <= 0) return;
  const int64_t s0 = sa.sup_off[i];
  const int ns = (int)(sa.sup_off[i + 1] - s0);
  const int32_t* __restrict__ scol = sa.scol + s0;
  const int32_t* __restrict__ sptr = sa.sptr + s0 + i;
  const int64_t e0 = rp[0];  // the worker's first entry, in both views
  const int32_t* __restrict__ srow = sa.srow + e0;
  const S* __restrict__ sval = (const S*)sa.sval + e0;
  const int nsh = sa.all_wave ? 0 : sa.n_short[i];
  const T bt = (T)nb;
  auto store_col = [&](int c, T g) {  // x_new[c] again, from the round's inputs
    T mix = T(0);
    for (int64_t e = pe0; e < pe1; ++e) mix += cw[e] * xo[(int64_t)ci[e] * ld + c];
    xn[c] = mix - eta * (g / bt + lam * xi[c]);
  };
  for (int k = tid; k < nsh; k += NT) {  // short columns: a thread each, stored order
    const int p1 = sptr[k + 1];
    T g = T(0);
    for (int e = sptr[k]; e < p1; ++e) g += (T)sval[e] * rres[srow[e]];
    store_col(scol[k], g);
  }
  for (int k = nsh + wave; k < ns; k += NW) {  // long columns: a wave each
    const int p1 = sptr[k + 1];
    T g = T(0);
    for (int e = sptr[k] + lane; e < p1; e += 64) g += (T)sval[e] * rres[srow[e]];
    g = wave_sum(g);
    if (lane == 0) store_col(scol[k], g);
  }
}

template <typename T, typename S, int PROB>
static hipError_t launch_sparse_t(const SparseArgs& g, int groups, hipStream_t s) {
  const RoundArgs& a = g.r;
  if (groups <= 0) return hipSuccess;
  if (a.nchunks < 1 || !a.rp || g.max_m < 0 || g.max_m > kSparseMaxRows) return hipErrorInvalidValue;
  if ((a.flags & F_LOSS) && a.idx) return hipErrorInvalidValue;  // the objective needs every row of the shard
  const size_t lds = 2 * NW * sizeof(double) + ((size_t)g.max_m * sizeof(T) + 15) / 16 * 16;
  const size_t max_lds = 160 * 1024;
  if (lds > max_lds) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_round_sparse<T, S, PROB>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  static const std::string name = [] {
    char buf[160];
    snprintf(buf, sizeof(buf), "void dopt::k_round_sparse<%s, %s, %d>(dopt::SparseArgs)",
             std::is_same<T, float>::value ? "float" : "double", std::is_same<S, float>::value ? "float" : "double",
             PROB);
    return std::string(buf);
  }();
  note_round_kernel(name.c_str());
  hipLaunchKernelGGL((k_round_sparse<T, S, PROB>), dim3(groups), dim3(NT), lds, s, g);
  return hipGetLastError();
}

template <typename T, typename S>
static hipError_t sparse_dispatch(int problem, const SparseArgs& g, int groups, hipStream_t s) {
  if (problem == 0) return launch_sparse_t<T, S, 0>(g, groups, s);
  if (problem == 1) return launch_sparse_t<T, S, 1>(g, groups, s);
  return hipErrorInvalidValue;
}

}  // namespace dopt
