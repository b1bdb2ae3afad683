// k_round_softmax.inc -- the fused D-SGD round of multinomial logistic (softmax) regression on the
// gfx950 matrix cores, and its launch dispatch; included by one translation unit per (state, data)
// element-type pair (softmax_f32.hip, softmax_f64.hip, softmax_x32.hip).  Per worker i with the
// iterate W_i (C x d), rows x_k and labels y_k in {0 .. C-1}:
//   z_k = W_i x_k,  p_k = softmax(z_k),  loss_k = logsumexp(z_k) - z_k[y_k]   (max-subtracted)
//   G_i = (1/b) sum_k (p_k - e_{y_k}) x_k^T + lam W_i                        (0 for an empty shard)
//   W_i' = sum_j Wmix_ij W_j - eta G_i
// A state row is stored class-major, C blocks of ld elements, so the mix, the column sums and the
// consensus are element-wise on a flat vector of C ld elements.
//
// One workgroup of 4 waves per worker.  The shard streams through LDS in tiles of 16 rows
// (non-temporal 16-byte loads into registers, tile t + 1 requested before tile t's arithmetic where
// the registers hold it -- softmax_pipe below; minibatch rows gathered through idx; rows past the
// batch and columns past the row are zeros).
// Wave w owns NFT feature tiles of 16, the features [16 NFT w, 16 NFT (w + 1)), in BOTH products:
//   logits    Z[16 rows x 16 classes]    += X[rows, 4 features] W^T[4 features, classes]   (split-K over
//             the waves; the four 16 x 16 partials meet in LDS and are summed in wave order)
//   gradient  G[16 features x 16 classes] += X^T[features, 4 rows] R[4 rows, classes],  R = P - Y
// with v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 (float32 rows are widened on the fragment
// read).  Lane l = 16 g + n (g = l >> 4, n = l & 15) keeps, per feature tile, the four values
// W[class n][tile + 4 g + q], q = 0..3, as the B operands of the logits product: k-step q gives lane
// group g the feature 4 g + q, which the A fragment (one 16-byte LDS read of row n) follows.  The
// gradient accumulators use the same (lane, register) -> (class, feature) map: the MFMA result
// register r of lane group g is output row Mfma::row(g, r), and the A fragment of the gradient puts
// feature Mfma::feat(i) into operand row i so that this row is feature 4 g + r.  The epilogue is
// therefore element-wise in registers: 16- or 32-byte loads of the neighbours' chunks (CSR order,
// through L2), W' = mix - eta (G / b + lam W) stored with vector stores, and the consensus partial
// of the chunk.  No LDS round trip for state, no global atomics, every reduction in a fixed order.
//
// Without F_STEP the launch takes metrics only and its B operands are xbar (the same for every
// worker): F_LOSS = sum_k loss_k(Wbar) over all rows of the shard, F_CONS = ||W_i - Wbar||^2 with
// W_i read in the epilogue.  The step launch fuses F_CONS (it holds W_i; Wbar is read per chunk)
// through the same accumulation, so either launch gives the same bits.
//
// LDS: [tile: 16 rows x (64 NFT features of S + 80 bytes of padding)] [zp: 4 waves x 16 x 16 T]
//      [R: 16 x 16 T] [sred: 2 x 4 doubles].  The padding makes the row stride 20 mod 64 dwords: the
//      16-rows-by-4-dwords fragment reads of the logits hit 64 distinct banks, the 4-rows-by-16-dwords
//      reads of the gradient overlap in 12 banks only.
namespace dopt {

constexpr int SM_WAVES = 4;
constexpr int SM_THREADS = SM_WAVES * 64;
constexpr int SM_PAD = 80;  // bytes per tile row

template <typename T>
struct Mfma;
template <>
struct Mfma<float> {
  typedef float acc __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc mma(float a, float b, acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // C/D: register r of lane group g holds output row 4 g + r
  static __device__ __forceinline__ int row(int g, int r) { return 4 * g + r; }
  static __device__ __forceinline__ int feat(int i) { return i; }
};
template <>
struct Mfma<double> {
  typedef double acc __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc mma(double a, double b, acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // C/D: register r of lane group g holds output row g + 4 r (as k_rs_gram reads it)
  static __device__ __forceinline__ int row(int g, int r) { return g + 4 * r; }
  // operand row i = g + 4 r carries feature 4 g + r
  static __device__ __forceinline__ int feat(int i) { return 4 * (i & 3) + (i >> 2); }
};

template <typename T>
__device__ __forceinline__ T group16_max(T v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const T u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T group16_sum(T v) {  // both lanes of a pair add the same two values: lane-independent
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T, typename S, int NFT, bool PIPE>
__global__ __launch_bounds__(SM_THREADS) __attribute__((amdgpu_waves_per_eu(1))) void k_round_softmax(
    const SoftmaxArgs sa) {
  const RoundArgs& a = sa.r;
  using M = Mfma<T>;
  using A4 = typename M::acc;
  using VX = typename KV<T, S>::VX;  // one 16-byte chunk of a shard row
  constexpr int VN = KV<T, S>::VN;
  constexpr int XC = 4 / VN;  // 16-byte chunks of a 4-feature fragment (float64 rows: 2)
  // state access: 4 contiguous features of one class, in vectors of HN (rows are padded to VN
  // elements, and a float64 state row over float64 data is 16-byte aligned only)
  constexpr int HN = (sizeof(T) == 8 && sizeof(S) == 8) ? 2 : 4;
  constexpr int NH = 4 / HN;
  using HV = typename VecOf<T, HN>::v;
  constexpr int TW = SM_WAVES * NFT * 16;  // features of a tile row
  constexpr int WCH = TW / VN;             // ... in 16-byte chunks
  constexpr int STRIDE = WCH * 16 + SM_PAD;
  constexpr int NLD = 16 * WCH / SM_THREADS;  // chunks of a tile per thread
  static_assert(NLD >= 1 && 16 * WCH % SM_THREADS == 0, "tile chunks divide over the threads");
  extern __shared__ __attribute__((aligned(32))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, n = lane & 15;
  const int i = blockIdx.x;
  const int flags = a.flags;
  const int C = sa.n_classes;
  const int nch = a.nchunks;
  const int64_t ld = a.ld;
  const int64_t ldw = (int64_t)C * ld;
  const int64_t row0 = a.off[i];
  const int64_t m = a.off[i + 1] - row0;
  const int64_t nb = a.idx ? (a.b < m ? a.b : m) : m;
  const bool step = (flags & F_STEP) != 0;
  const bool want_loss = (flags & F_LOSS) != 0;  // metrics launch, every row of the shard (host-checked)
  const bool want_cons = (flags & F_CONS) != 0;
  const int64_t nrow = (step || want_loss) ? nb : 0;
  const int64_t ntiles = (nrow + 15) / 16;
  const S* __restrict__ X = (const S*)a.X;
  const S* __restrict__ Yp = (const S*)a.y;
  const int32_t* __restrict__ bidx = a.idx ? a.idx + (int64_t)i * a.b : nullptr;
  const T* own_row = (const T*)a.x_old + (int64_t)i * ldw;
  const T* wsrc = step ? own_row : (const T*)a.xbar;  // the B operands of the logits

  char* xs = smem;
  T* zp = (T*)(smem + 16 * STRIDE);  // [SM_WAVES][16][16]
  T* Rs = zp + SM_WAVES * 256;       // [16][16]
  double* sred = (double*)(Rs + 256);

  // tile t -> registers: thread tid takes chunks q = tid + 256 k, row q / WCH, chunk q % WCH
  auto load_tile = [&](int64_t t, VX (&st)[NLD], int& yl) {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int q = tid + SM_THREADS * k;
      const int r = q / WCH, ch = q % WCH;
      const int64_t rg = t * 16 + r;
      st[k] = VX(0);
      if (rg < nrow && ch < nch) {
        const int64_t lr = bidx ? bidx[rg] : rg;
        st[k] = __builtin_nontemporal_load((const VX*)(X + (row0 + lr) * ld + (int64_t)ch * VN));
      }
    }
    const int64_t rg = t * 16 + (tid >> 4);  // the label of the row this thread's softmax term belongs to
    yl = -1;
    if (rg < nrow) yl = (int)Yp[row0 + (bidx ? bidx[rg] : rg)];
  };
  auto store_tile = [&](const VX (&st)[NLD]) {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int q = tid + SM_THREADS * k;
      *(VX*)(xs + (q / WCH) * STRIDE + (q % WCH) * 16) = st[k];
    }
  };
  VX st[NLD];
  int ycur = -1, ynxt = -1;
  if (PIPE && ntiles > 0) load_tile(0, st, ynxt);  // the first tile, ahead of everything else

  // resident operands and accumulators: feature tile j of this wave, class n, features 4 g + q
  T wreg[NFT][4];
  A4 G[NFT];
#pragma unroll
  for (int j = 0; j < NFT; ++j) {
    const int f0 = (wave * NFT + j) * 16 + 4 * g;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int fo = f0 + HN * h;
      HV v = HV(0);
      if (n < C && fo < ld) v = *(const HV*)(wsrc + (int64_t)n * ld + fo);
#pragma unroll
      for (int e = 0; e < HN; ++e) wreg[j][HN * h + e] = v[e];
    }
    G[j] = A4(0);
  }

  double loss = 0.0;
  for (int64_t t = 0; t < ntiles; ++t) {
    if constexpr (PIPE) {
      ycur = ynxt;
    } else {
      load_tile(t, st, ycur);
    }
    store_tile(st);
    __syncthreads();
    if (PIPE && t + 1 < ntiles) load_tile(t + 1, st, ynxt);

    // logits of the tile over this wave's features: two accumulators, two dependency chains
    A4 z0 = A4(0), z1 = A4(0);
#pragma unroll
    for (int j = 0; j < NFT; ++j) {
      const char* p = xs + n * STRIDE + ((wave * NFT + j) * 16 + 4 * g) * (int)sizeof(S);
      S xv[4];
#pragma unroll
      for (int c = 0; c < XC; ++c) {
        const VX v = *(const VX*)(p + 16 * c);
#pragma unroll
        for (int e = 0; e < VN && e < 4; ++e) xv[c * VN + e] = v[e];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (j & 1) z1 = M::mma((T)xv[q], wreg[j][q], z1);
        else z0 = M::mma((T)xv[q], wreg[j][q], z0);
      }
    }
    z0 += z1;
#pragma unroll
    for (int r = 0; r < 4; ++r) zp[(wave * 16 + M::row(g, r)) * 16 + n] = z0[r];
    __syncthreads();

    // softmax of row tid >> 4 across the 16 lanes of its group (class tid & 15)
    {
      const int cls = tid & 15;
      T z = zp[tid];
#pragma unroll
      for (int w = 1; w < SM_WAVES; ++w) z += zp[w * 256 + tid];  // wave order
      const bool cv = cls < C;
      const bool rv = ycur >= 0;
      const T mx = group16_max(cv ? z : -INFINITY);
      const T e = cv ? exp(z - mx) : T(0);
      const T s = group16_sum(e);
      const T hit = (cls == ycur) ? T(1) : T(0);
      Rs[tid] = (rv && cv) ? e / s - hit : T(0);
      if (want_loss) {
        const T zy = group16_sum(cls == ycur ? z : T(0));
        if (rv && cls == 0) loss += (double)(mx + log(s) - zy);
      }
    }
    if (step) {
      __syncthreads();
      T b[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) b[kk] = Rs[(4 * kk + g) * 16 + n];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const char* p = xs + (4 * kk + g) * STRIDE + (wave * NFT * 16 + M::feat(n)) * (int)sizeof(S);
#pragma unroll
        for (int j = 0; j < NFT; ++j) G[j] = M::mma((T)*(const S*)(p + j * 16 * (int)sizeof(S)), b[kk], G[j]);
      }
      __syncthreads();  // the tile is free for the next rows
    }
  }

  // epilogue: element-wise in registers
  double cons = 0.0;
  if (step || want_cons) {
    const T eta = (T)a.eta;
    const T lam = (T)a.lam;
    const int64_t pe0 = a.rp[i], pe1 = a.rp[i + 1];
    const T* __restrict__ cw = (const T*)a.cw;
    T* xn = (T*)a.x_new + (int64_t)i * ldw;
#pragma unroll
    for (int j = 0; j < NFT; ++j) {
      const int f0 = (wave * NFT + j) * 16 + 4 * g;
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const int fo = f0 + HN * h;
        if (n < C && fo < ld) {
          const int64_t co = (int64_t)n * ld + fo;
          HV opnd, gs;
#pragma unroll
          for (int e = 0; e < HN; ++e) {
            opnd[e] = wreg[j][HN * h + e];
            gs[e] = G[j][HN * h + e];
          }
          const HV own = step ? opnd : *(const HV*)(own_row + co);
          if (step) {
            HV mix = HV(0);
            for (int64_t e = pe0; e < pe1; ++e)  // CSR order
              mix += cw[e] * *(const HV*)((const T*)a.x_old + (int64_t)a.ci[e] * ldw + co);
            const HV gc = (nb > 0) ? (gs / (T)nb + lam * own) : HV(0);
            *(HV*)(xn + co) = mix - eta * gc;
          }
          if (want_cons) {
            const HV xb = step ? *(const HV*)((const T*)a.xbar + co) : opnd;
            const HV dv = own - xb;
#pragma unroll
            for (int e = 0; e < HN; ++e) cons += (double)(dv[e] * dv[e]);
          }
        }
      }
    }
  }
  if (want_cons || want_loss) {  // fixed order: lanes, then waves
    cons = wave_sum(cons);
    loss = wave_sum(loss);
    if (lane == 0) {
      sred[wave] = cons;
      sred[SM_WAVES + wave] = loss;
    }
    __syncthreads();
    if (tid == 0) {
      double cs = 0.0, ls = 0.0;
#pragma unroll
      for (int w = 0; w < SM_WAVES; ++w) {
        cs += sred[w];
        ls += sred[SM_WAVES + w];
      }
      if (want_cons) a.slab_cons[i] = cs;
      if (want_loss) a.slab_loss[i] = ls;
    }
  }
}

// The next tile waits in registers while the current one is multiplied, except where the float64
// operands and accumulators of 16 feature tiles per wave (256 + 256 registers with the fragments)
// leave no room for it: there the tile is loaded when it is needed.
template <typename T, int NFT>
constexpr bool softmax_pipe() {
  return !(sizeof(T) == 8 && NFT == 16);
}

template <typename T, typename S, int NFT>
static hipError_t launch_softmax_t(const SoftmaxArgs& g, int groups, hipStream_t s) {
  constexpr int VN = KV<T, S>::VN;
  constexpr int TW = SM_WAVES * NFT * 16;
  constexpr size_t lds = 16 * (size_t)(TW / VN * 16 + SM_PAD) + (SM_WAVES + 1) * 256 * sizeof(T) + 2 * SM_WAVES * sizeof(double);
  static_assert(lds <= 160 * 1024, "the tile and the partial logits fit the LDS");
  constexpr bool PIPE = softmax_pipe<T, NFT>();
  const RoundArgs& a = g.r;
  if (a.ld < 1 || a.ld > TW || a.ld % VN || a.nchunks != a.ld / VN || !a.rp) return hipErrorInvalidValue;
  if (g.n_classes < 2 || g.n_classes > 16) return hipErrorInvalidValue;
  if ((a.flags & F_LOSS) && ((a.flags & F_STEP) || a.idx)) return hipErrorInvalidValue;  // the objective: its own launch, every row
  if (a.flags & ~(F_STEP | F_CONS | F_LOSS)) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_round_softmax<T, S, NFT, PIPE>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  static const std::string name = [] {
    char buf[160];
    snprintf(buf, sizeof(buf), "void dopt::k_round_softmax<%s, %s, %d, %s>(dopt::SoftmaxArgs)",
             std::is_same<T, float>::value ? "float" : "double", std::is_same<S, float>::value ? "float" : "double",
             NFT, PIPE ? "true" : "false");
    return std::string(buf);
  }();
  note_round_kernel(name.c_str());
  hipLaunchKernelGGL((k_round_softmax<T, S, NFT, PIPE>), dim3(groups), dim3(SM_THREADS), lds, s, g);
  return hipGetLastError();
}

// Feature tiles per wave: the smallest power of two whose 64 NFT features hold the row.
template <typename T, typename S>
static hipError_t softmax_dispatch(const SoftmaxArgs& g, int groups, hipStream_t s) {
  if (groups <= 0) return hipSuccess;
  const int64_t ld = g.r.ld;
  if (ld <= 64) return launch_softmax_t<T, S, 1>(g, groups, s);
  if (ld <= 128) return launch_softmax_t<T, S, 2>(g, groups, s);
  if (ld <= 256) return launch_softmax_t<T, S, 4>(g, groups, s);
  if (ld <= 512) return launch_softmax_t<T, S, 8>(g, groups, s);
  if (ld <= 1024) return launch_softmax_t<T, S, 16>(g, groups, s);
  return hipErrorInvalidValue;
}

}  // namespace dopt
