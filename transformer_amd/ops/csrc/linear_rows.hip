// Skinny-M linear for decode: Y[M,N] = X[M,K] . W[N,K]^T (+bias)(+ReLU),
// 1 <= M <= 64, bf16 in/out, fp32 accumulate, ONE launch: no workspace, no
// atomics, no zero-fill, fixed summation order.  linear_rows_ln carries the
// residual add and the LayerNorm that follows three of a decoder layer's
// linears in the same launch.
//
// Why not the training GEMM: with M = batch rows the 128-row tile has 1-16
// live rows, and the split-K path it takes at these shapes is three launches
// (zero-fill, atomics kernel, finalize).  A decode linear is a streaming read
// of W, so the design below reads every byte of W exactly once, straight
// into MFMA operand registers.
//
// Operands (swapped).  mfma_f32_16x16x32_bf16 with 16 rows of W on the
// instruction's M side and 16 rows of X on its N side.  W rows are
// K-contiguous, so the A fragment of lane l (row l%16, k-group l/16) is a
// 16-byte global load that needs no LDS trip.  The contraction index may be
// permuted as long as both operands agree, so a wave takes K in steps of 64:
// k-group g owns the 16 contiguous elements [16g, 16g+16) of the step and
// feeds their halves to two MFMAs.  A wave's load then covers 128 contiguous
// bytes of each of its 16 W rows (whole cache lines).  The X fragments use
// the same k mapping and come straight from global: X is at most 64 rows and
// L2-resident, and lanes whose X row is >= M load nothing and supply zeros.
//
// Row groups.  MG in {1,2,4} 16-row groups of X: one W fragment feeds MG
// MFMAs into MG accumulators, so M = 64 still streams W once.
//
// Work split.  One block owns a 16-column strip of N (grid = cdiv(N,16));
// its NW waves take the 64-element K steps round-robin.  Every wave stores
// its fp32 partials to LDS; wave mg (< MG) then sums group mg's partials in
// wave order 0..NW-1 -- a fixed order, so results are reproducible -- and
// runs the epilogue.
//
// Epilogue.  Accumulator lane l holds 4 consecutive output columns
// n0 + 4*(l/16) + {0..3} of X row 16*mg + l%16: 4 consecutive bias values,
// ReLU, one 8-byte bf16 store.  N % 4 != 0 (or unaligned bias/out) takes
// guarded scalar accesses instead; W rows >= N are never read.
//
// LN variant.  The epilogue stores the fp32 pre-norm strip
// t = acc + bias + res to an (M,N) fp32 workspace with write-through
// (agent-scope) stores and takes a ticket (common.h last_arriver).  The
// last block normalises all M rows, one wave per row, two rows of a wave in
// flight at once; mean and variance are two-pass fp32 over registers.  It
// stores bf16 and re-zeroes the ticket, so a graph replay needs no memset.
// No block reads what another wrote before the gate.  The linear's output is
// never rounded to bf16 on the way to the LayerNorm.
//
// Pre-LN variant (linear_rows_preln).  The LayerNorm of the linear's INPUT:
// XN = LN(P + R), Y = act(XN . W^T + bias).  A LayerNorm row needs only its
// own row and every block reads all of X anyway, so every block normalises
// all M rows itself before its K loop: no ticket, no workspace, no tail, no
// block reading what another block of the launch wrote.  A quarter-wave owns
// a row (4 rows per wave, a 16-row group per pass of the 4 waves): 16-byte
// loads of P and R, the fp32 sum kept in registers, mean then centred
// squares reduced by 4 xor-shuffles, bf16 rows written to a padded LDS tile
// (rows >= M as zeros), one barrier.  The K loop is the plain kernel's, with
// the X fragments read from the tile, so Y is bit-equal to linear_rows(XN).
// A wave's first W loads are issued before the prologue.  Row m of XN goes
// to global from block m % gridDim.x, out of the registers that hold it.
//
// Workspace: [ticket: 1 word, padded to 4][t: M*N floats].  Calls on one
// stream may share it (they are stream-ordered); calls on different streams
// must NOT.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#define LR_MAX_M 64
#define LR_LN_MAX_N 2048     // LN tail keeps a row in registers
#define LR_PRE_MAX_K 1024    // pre-LN prologue keeps a row in 16 lanes
#define LR_PRE_PAD 8         // tile row stride K + 8: 16 rows, 16 banks apart

typedef __bf16 bf16x8l __attribute__((ext_vector_type(8)));

// Built without packed fp32 VALU ops, whatever the build's global flags are.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// Agent-scope relaxed accesses to the pre-norm workspace: the stores write
// through to the coherent point and the loads bypass this CU's and this
// XCD's non-coherent lines, so the strip needs no L2 write-back fence.
DEV_INLINE void lr_ws_store(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DEV_INLINE float lr_ws_load(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LayerNorm of rows wave, wave+NW, .. of t (M,N fp32), one wave per row,
// two rows of a wave in flight so that one row's load and shuffle latency
// hides under the other's.  Column c = lane + 64*i sits in slot i.
template <int NW>
DEV_INLINE void lr_ln_rows(const float* t, const short* __restrict__ gamma,
                           const short* __restrict__ beta,
                           short* __restrict__ y, int M, int N, float eps,
                           int wave, int lane) {
  constexpr int NC = LR_LN_MAX_N / WAVE;
  const float inv_n = 1.0f / (float)N;
  for (int m0 = wave; m0 < M; m0 += 2 * NW) {
    const int m1 = m0 + NW;
    const bool two = m1 < M;                   // wave-uniform
    float ta[NC], tb[NC], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + i * WAVE;
      ta[i] = tb[i] = 0.f;
      if (i * WAVE >= N) continue;             // wave-uniform
      ta[i] = c < N ? lr_ws_load(t + (long)m0 * N + c) : 0.f;
      tb[i] = (two && c < N) ? lr_ws_load(t + (long)m1 * N + c) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) { sa += ta[i]; sb += tb[i]; }
    const float mean_a = wave_sum(sa) * inv_n, mean_b = wave_sum(sb) * inv_n;
    float qa = 0.f, qb = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const bool in = lane + i * WAVE < N;
      const float da = ta[i] - mean_a, db = tb[i] - mean_b;
      qa += in ? da * da : 0.f;
      qb += in ? db * db : 0.f;
    }
    const float rs_a = rsqrtf(wave_sum(qa) * inv_n + eps);
    const float rs_b = rsqrtf(wave_sum(qb) * inv_n + eps);
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = lane + i * WAVE;
      if (i * WAVE >= N) break;                // wave-uniform
      if (c < N) {
        const float ga = bfbits2f(gamma[c]), be = bfbits2f(beta[c]);
        y[(long)m0 * N + c] = f2bfbits((ta[i] - mean_a) * rs_a * ga + be);
        if (two)
          y[(long)m1 * N + c] = f2bfbits((tb[i] - mean_b) * rs_b * ga + be);
      }
    }
  }
}

// K steps a wave has in flight: 8 loads of W/X per lane and step at MG=4
template <int MG> constexpr int lr_unr() { return MG == 4 ? 2 : 4; }

// W fragments of steps s0, s0 + NW, ..: wp already carries row and k-group.
template <int MG, int NW>
DEV_INLINE void lr_load_w(s16x8 (&wv)[lr_unr<MG>()][2], const short* wp,
                          bool wlive, int s0, int g, int K) {
  const s16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < lr_unr<MG>(); ++u)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = (s0 + u * NW) * 64 + h * 8;
      wv[u][h] = (k + g * 16 + 8 <= K && wlive) ? *(const s16x8*)(wp + k)
                                                : zero8;
    }
}

// Pre-LN prologue: tile[16*MG][K + LR_PRE_PAD] = bf16(LN(P + R)), rows >= M
// zero; row m also to XN from block m % gridDim.x.  Lane j of a quarter-wave
// holds the 16-byte chunks j, j + 16, .. of its row.
template <int MG, int NW>
DEV_INLINE void lr_preln_tile(const short* __restrict__ P,
                              const short* __restrict__ R,
                              const short* __restrict__ gamma,
                              const short* __restrict__ beta,
                              short* __restrict__ XN, short* tile, int M,
                              int K, float eps, int wave, int lane) {
  static_assert(NW == 4, "4 waves x 4 rows = one 16-row group per pass");
  constexpr int NCH = LR_PRE_MAX_K / 128;
  const s16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const int j = lane & 15, ld = K + LR_PRE_PAD;
  const float inv_k = 1.0f / (float)K;
#pragma unroll 1
  for (int mg = 0; mg < MG; ++mg) {
    const int m = mg * 16 + wave * 4 + (lane >> 4);
    const bool live = m < M;
    float t[NCH][8], s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int k = (j + 16 * i) * 8;
      const bool in = live && k < K;
      const s16x8 pv = in ? *(const s16x8*)(P + (long)m * K + k) : zero8;
      const s16x8 rv = in ? *(const s16x8*)(R + (long)m * K + k) : zero8;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        t[i][e] = bfbits2f(pv[e]) + bfbits2f(rv[e]);
        s += t[i][e];
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const float mean = s * inv_k;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const bool in = (j + 16 * i) * 8 < K;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = t[i][e] - mean;
        q += in ? d * d : 0.f;
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) q += __shfl_xor(q, off);
    const float rs = rsqrtf(q * inv_k + eps);
    const bool mine = live && m % (int)gridDim.x == (int)blockIdx.x;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int k = (j + 16 * i) * 8;
      if (k >= K) continue;
      s16x8 ov = zero8;
      if (live) {
        const s16x8 gv = *(const s16x8*)(gamma + k);
        const s16x8 bv = *(const s16x8*)(beta + k);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          ov[e] = f2bfbits((t[i][e] - mean) * rs * bfbits2f(gv[e]) +
                           bfbits2f(bv[e]));
      }
      *(s16x8*)(tile + m * ld + k) = ov;
      if (mine) *(s16x8*)(XN + (long)m * K + k) = ov;
    }
  }
  __syncthreads();
}

template <int MG, int NW, bool LN>
__global__ __launch_bounds__(NW * WAVE)
void linear_rows_kernel(const short* __restrict__ X,
                        const short* __restrict__ W,
                        const short* __restrict__ bias, short* __restrict__ Y,
                        int M, int N, int K, int relu, int vec,
                        const short* __restrict__ res,
                        const short* __restrict__ gamma,
                        const short* __restrict__ beta, float* ws, float eps) {
  constexpr bool PRE = false;
  short* const XN = nullptr;
  short* const tile = nullptr;
#include "linear_rows_body.inc"
}

// Dynamic LDS: the 16*MG x (K + LR_PRE_PAD) bf16 tile.
template <int MG, int NW>
__global__ __launch_bounds__(NW * WAVE)
void linear_rows_preln_kernel(const short* __restrict__ X,
                              const short* __restrict__ res,
                              const short* __restrict__ gamma,
                              const short* __restrict__ beta, float eps,
                              const short* __restrict__ W,
                              const short* __restrict__ bias,
                              short* __restrict__ XN, short* __restrict__ Y,
                              int M, int N, int K, int relu, int vec) {
  constexpr bool LN = false, PRE = true;
  float* const ws = nullptr;
  extern __shared__ __attribute__((aligned(16))) short tile[];
#include "linear_rows_body.inc"
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---- host wrappers ---------------------------------------------------------

// Waves per block.  Measured (tools/linear_rows_bench.py, docs/PERF.md).
static int lr_nw(int K) { return K >= 2048 ? 8 : 4; }

static bool lr_al(const void* p, uintptr_t a) { return (uintptr_t)p % a == 0; }

template <bool LN>
static void lr_launch(const torch::Tensor& x, const torch::Tensor& w,
                      const short* bias, torch::Tensor& y, bool relu, bool vec,
                      const short* res, const short* gamma, const short* beta,
                      float* ws, float eps, int64_t nw_arg) {
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(nw_arg == 0 || nw_arg == 4 || nw_arg == 8,
              "linear_rows: nw must be 0 (rule), 4 or 8");
  const int nw = nw_arg ? (int)nw_arg : lr_nw(K);
  const int mg = M <= 16 ? 1 : M <= 32 ? 2 : 4;
  auto stream = at::hip::getCurrentHIPStream();
#define LR_GO(MGC, NWC)                                                      \
  linear_rows_kernel<MGC, NWC, LN><<<cdiv(N, 16), NWC * WAVE, 0, stream>>>(  \
      (const short*)x.data_ptr(), (const short*)w.data_ptr(), bias,          \
      (short*)y.data_ptr(), M, N, K, relu ? 1 : 0, vec ? 1 : 0, res, gamma,  \
      beta, ws, eps)
  if (nw == 4) {
    if (mg == 1) LR_GO(1, 4); else if (mg == 2) LR_GO(2, 4); else LR_GO(4, 4);
  } else {
    if (mg == 1) LR_GO(1, 8); else if (mg == 2) LR_GO(2, 8); else LR_GO(4, 8);
  }
#undef LR_GO
}

static void lr_check_xw(const torch::Tensor& x, const torch::Tensor& w) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && x.dtype() == torch::kBFloat16 &&
              w.dtype() == torch::kBFloat16 && x.dim() == 2 && w.dim() == 2,
              "linear_rows: x (M,K) and w (N,K) must be 2-D bf16 on GPU");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous(),
              "linear_rows: x and w must be contiguous");
  TORCH_CHECK(x.size(1) == w.size(1), "linear_rows: K mismatch");
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= LR_MAX_M,
              "linear_rows: 1 <= M <= ", LR_MAX_M, " (got ", x.size(0),
              "); larger M is ops.linear's job");
  TORCH_CHECK(x.size(1) >= 8 && x.size(1) % 8 == 0 && w.size(0) >= 1,
              "linear_rows: K must be a positive multiple of 8");
  TORCH_CHECK(lr_al(x.data_ptr(), 16) && lr_al(w.data_ptr(), 16),
              "linear_rows: x and w must be 16-byte aligned");
}

static const short* lr_vecN(const c10::optional<torch::Tensor>& t, int64_t N,
                            const char* name) {
  if (!t.has_value() || !t->defined() || t->numel() == 0) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kBFloat16 &&
              t->is_contiguous() && t->numel() == N,
              "linear_rows: ", name, " must be a contiguous bf16 (N,) tensor");
  return (const short*)t->data_ptr();
}

torch::Tensor linear_rows(torch::Tensor x, torch::Tensor w,
                          c10::optional<torch::Tensor> bias, bool relu,
                          int64_t nw) {
  lr_check_xw(x, w);
  const int64_t M = x.size(0), N = w.size(0);
  const short* bp = lr_vecN(bias, N, "bias");
  auto y = torch::empty({M, N}, x.options());
  const bool vec = N % 4 == 0 && lr_al(bp, 8) && lr_al(y.data_ptr(), 8);
  lr_launch<false>(x, w, bp, y, relu, vec, nullptr, nullptr, nullptr, nullptr,
                   0.f, nw);
  return y;
}

// Zeroed ticket + the fp32 pre-norm rows of any linear_rows_ln call with
// M <= M_max and N <= N_max.  Allocate ONCE, outside graph capture; share
// across the layers of a step, never across streams.
torch::Tensor linear_rows_workspace(int64_t M, int64_t N) {
  TORCH_CHECK(M > 0 && N > 0, "linear_rows_workspace: bad shape");
  return torch::zeros({4 + M * N},
                      torch::TensorOptions().dtype(torch::kFloat32)
                          .device(torch::kCUDA, at::cuda::current_device()));
}

torch::Tensor linear_rows_ln(torch::Tensor x, torch::Tensor w,
                             c10::optional<torch::Tensor> bias,
                             torch::Tensor res, torch::Tensor gamma,
                             torch::Tensor beta, double eps, torch::Tensor ws,
                             int64_t nw) {
  lr_check_xw(x, w);
  const int64_t M = x.size(0), N = w.size(0);
  TORCH_CHECK(N <= LR_LN_MAX_N, "linear_rows_ln: N <= ", LR_LN_MAX_N);
  const short* bp = lr_vecN(bias, N, "bias");
  const short* gp = lr_vecN(gamma, N, "gamma");
  const short* btp = lr_vecN(beta, N, "beta");
  TORCH_CHECK(gp != nullptr && btp != nullptr,
              "linear_rows_ln: gamma and beta are required");
  TORCH_CHECK(res.is_cuda() && res.dtype() == torch::kBFloat16 &&
              res.is_contiguous() && res.dim() == 2 && res.size(0) == M &&
              res.size(1) == N,
              "linear_rows_ln: res must be a contiguous bf16 (M,N) tensor");
  TORCH_CHECK(ws.defined() && ws.is_cuda() && ws.dtype() == torch::kFloat32 &&
              ws.is_contiguous() && lr_al(ws.data_ptr(), 16),
              "linear_rows_ln: ws must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(ws.numel() >= 4 + M * N, "linear_rows_ln: ws too small (",
              ws.numel(), " < ", 4 + M * N,
              "); allocate it with linear_rows_workspace");
  auto y = torch::empty({M, N}, x.options());
  const bool vec = N % 4 == 0 && lr_al(bp, 8) && lr_al(res.data_ptr(), 8);
  lr_launch<true>(x, w, bp, y, false, vec, (const short*)res.data_ptr(), gp,
                  btp, ws.data_ptr<float>(), (float)eps, nw);
  return y;
}

// One pre-LN instantiation: raises its dynamic-LDS limit to the largest
// tile it serves the first time a device sees it, then launches.
template <int MG>
static void lr_preln_go(hipStream_t stream, int dev, const short* p,
                        const short* r, const short* gamma, const short* beta,
                        float eps, const short* w, const short* bias,
                        short* xn, short* y, int M, int N, int K, bool relu,
                        bool vec) {
  auto kern = linear_rows_preln_kernel<MG, 4>;
  static unsigned long long raised = 0;      // bit per device
  if (!(raised >> dev & 1ull)) {
    const int most = 16 * MG * (LR_PRE_MAX_K + LR_PRE_PAD) * 2;
    C10_HIP_CHECK(hipFuncSetAttribute(
        (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, most));
    raised |= 1ull << dev;
  }
  const size_t lds = (size_t)16 * MG * (K + LR_PRE_PAD) * 2;
  kern<<<cdiv(N, 16), 4 * WAVE, lds, stream>>>(p, r, gamma, beta, eps, w, bias,
                                              xn, y, M, N, K, relu ? 1 : 0,
                                              vec ? 1 : 0);
}

std::vector<torch::Tensor> linear_rows_preln(
    torch::Tensor p, torch::Tensor res, torch::Tensor gamma,
    torch::Tensor beta, double eps, torch::Tensor w,
    c10::optional<torch::Tensor> bias, bool relu, int64_t nw) {
  lr_check_xw(p, w);
  const int64_t M = p.size(0), K = p.size(1), N = w.size(0);
  TORCH_CHECK(K <= LR_PRE_MAX_K, "linear_rows_preln: K <= ", LR_PRE_MAX_K);
  TORCH_CHECK(nw == 0 || nw == 4,
              "linear_rows_preln: nw must be 0 (rule) or 4");
  TORCH_CHECK(lr_nw(K) == 4, "linear_rows_preln: 4 waves per block only");
  TORCH_CHECK(res.is_cuda() && res.dtype() == torch::kBFloat16 &&
              res.is_contiguous() && res.dim() == 2 && res.size(0) == M &&
              res.size(1) == K && lr_al(res.data_ptr(), 16),
              "linear_rows_preln: res must be a contiguous, 16-byte aligned "
              "bf16 (M,K) tensor");
  const short* bp = lr_vecN(bias, N, "bias");
  const short* gp = lr_vecN(gamma, K, "gamma");
  const short* btp = lr_vecN(beta, K, "beta");
  TORCH_CHECK(gp != nullptr && btp != nullptr && lr_al(gp, 16) &&
              lr_al(btp, 16),
              "linear_rows_preln: gamma and beta are required, 16-byte "
              "aligned");
  auto xn = torch::empty({M, K}, p.options());
  auto y = torch::empty({M, N}, p.options());
  TORCH_CHECK(lr_al(xn.data_ptr(), 16), "linear_rows_preln: xn alignment");
  const bool vec = N % 4 == 0 && lr_al(bp, 8) && lr_al(y.data_ptr(), 8);
  const int dev = p.get_device();
  TORCH_CHECK(dev >= 0 && dev < 64, "linear_rows_preln: device index");
  auto stream = at::hip::getCurrentHIPStream();
#define LRP_GO(MGC)                                                          \
  lr_preln_go<MGC>(stream, dev, (const short*)p.data_ptr(),                  \
                   (const short*)res.data_ptr(), gp, btp, (float)eps,        \
                   (const short*)w.data_ptr(), bp, (short*)xn.data_ptr(),    \
                   (short*)y.data_ptr(), (int)M, (int)N, (int)K, relu, vec)
  if (M <= 16) LRP_GO(1); else if (M <= 32) LRP_GO(2); else LRP_GO(4);
#undef LRP_GO
  return {xn, y};
}
