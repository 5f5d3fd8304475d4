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
// Workspace: [ticket: 1 word, padded to 4][t: M*N floats].  Calls on one
// stream may share it (they are stream-ordered); calls on different streams
// must NOT.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#define LR_MAX_M 64
#define LR_LN_MAX_N 2048     // LN tail keeps a row in registers

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

// vec: N % 4 == 0 and bias/res/y/ws 8-(16-)byte aligned -> vector epilogue.
template <int MG, int NW, bool LN>
__global__ __launch_bounds__(NW * WAVE)
void linear_rows_kernel(const short* __restrict__ X,
                        const short* __restrict__ W,
                        const short* __restrict__ bias, short* __restrict__ Y,
                        int M, int N, int K, int relu, int vec,
                        const short* __restrict__ res,
                        const short* __restrict__ gamma,
                        const short* __restrict__ beta, float* ws, float eps) {
  // K steps a wave has in flight: 8 loads of W/X per lane and step at MG=4
  constexpr int UNR = MG == 4 ? 2 : 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = lane >> 4, r16 = lane & 15;
  const int n0 = blockIdx.x * 16;
  const int nrow = n0 + r16;                  // this lane's W row
  const bool wlive = nrow < N;
  const short* wp = W + (long)nrow * K + g * 16;
  const short* xp = X + (long)r16 * K + g * 16;

  f32x4 acc[MG];
#pragma unroll
  for (int mg = 0; mg < MG; ++mg) acc[mg] = f32x4{0.f, 0.f, 0.f, 0.f};

  const s16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const int nsteps = cdiv(K, 64);
  for (int s0 = wave; s0 < nsteps; s0 += NW * UNR) {
    s16x8 wv[UNR][2], xv[UNR][MG][2];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // steps past nsteps start at k >= K: the one test covers both
        const int k = (s0 + u * NW) * 64 + h * 8;    // + g*16 in wp/xp
        const bool kin = k + g * 16 + 8 <= K;
        wv[u][h] = (kin && wlive) ? *(const s16x8*)(wp + k) : zero8;
#pragma unroll
        for (int mg = 0; mg < MG; ++mg)
          xv[u][mg][h] = (kin && mg * 16 + r16 < M)
                             ? *(const s16x8*)(xp + (long)mg * 16 * K + k)
                             : zero8;
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg)
          acc[mg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              (bf16x8l)wv[u][h], (bf16x8l)xv[u][mg][h], acc[mg], 0, 0, 0);
  }

  // waves -> block: wave mg sums group mg's partials in wave order
  __shared__ __attribute__((aligned(16))) float s_part[NW][MG][WAVE][4];
#pragma unroll
  for (int mg = 0; mg < MG; ++mg) *(f32x4*)s_part[wave][mg][lane] = acc[mg];
  __syncthreads();

  if (wave < MG) {
    const int mg = wave;
    f32x4 v = *(const f32x4*)s_part[0][mg][lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += *(const f32x4*)s_part[w][mg][lane];
    const int m = mg * 16 + r16, n = n0 + g * 4;
    if (m < M && n < N) {
      const long o = (long)m * N + n;
      if (vec) {                               // n + 4 <= N: N % 4 == 0
        if (bias != nullptr) {
          const s16x4 bv = *(const s16x4*)(bias + n);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bfbits2f(bv[r]);
        }
        if constexpr (LN) {
          const s16x4 rv = *(const s16x4*)(res + o);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += bfbits2f(rv[r]);
#pragma unroll
          for (int r = 0; r < 4; ++r) lr_ws_store(ws + 4 + o + r, v[r]);
        } else {
          s16x4 ov;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            ov[r] = f2bfbits(relu ? fmaxf(v[r], 0.f) : v[r]);
          *(s16x4*)(Y + o) = ov;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (n + r >= N) break;
          float a = v[r];
          if (bias != nullptr) a += bfbits2f(bias[n + r]);
          if constexpr (LN) {
            lr_ws_store(ws + 4 + o + r, a + bfbits2f(res[o + r]));
          } else {
            Y[o + r] = f2bfbits(relu ? fmaxf(a, 0.f) : a);
          }
        }
      }
    }
  }

  if constexpr (LN) {
    // last_arriver drains each wave's write-through stores (vmcnt) before
    // the ticket, and its winner takes an agent acquire before the loads
    unsigned* ticket = (unsigned*)ws;
    if (!last_arriver(ticket, gridDim.x)) return;
    lr_ln_rows<NW>(ws + 4, gamma, beta, Y, M, N, eps, wave, lane);
    if (tid == 0)
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
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
