// Gradient accumulation for micro-batched optimizer steps
// (runtime/optimizer.py NoamAdam.accumulate): acc[i] += float(grad[i]) over
// the whole flat buffer, bf16 gradient in, fp32 accumulator read-modify-write.
//
// There is no "first micro-step" flag.  The accumulator is all-zero between
// optimizer steps — the accumulator-reading Adam kernels (adam.hip) store
// zeros back in the pass that consumes it — so the same launch serves every
// micro-step, eagerly and inside a captured hipGraph.
//
// Pure bandwidth: 10 B/element (2 read + 4 read + 4 write).  One fp32 add of
// a bf16 value per element, so the result has no ordering freedom.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

constexpr int GA_THREADS = 256;     // 4 waves
constexpr int GA_VEC = 8;           // elements per thread per trip
constexpr int GA_MAX_BLOCKS = 2048; // 8 blocks/CU on 256 CUs

static inline int ga_blocks(long n) {
  long b = (n + (long)GA_THREADS * GA_VEC - 1) / ((long)GA_THREADS * GA_VEC);
  if (b < 1) b = 1;
  return (int)(b < GA_MAX_BLOCKS ? b : GA_MAX_BLOCKS);
}

// The buffer is split on the ACCUMULATOR's alignment (it carries 8 of the 10
// bytes per element): a scalar head (< 4 elements, up to acc's first 16-byte
// boundary), a body of 8-element groups whose accumulator accesses are two
// aligned f32x4 loads and two aligned f32x4 stores, and a scalar tail (< 8
// elements).  The gradient of a group is one s16x8 load when grad + head is
// 16-byte aligned too — always, for the optimizer's flat buffers — and eight
// 2-byte loads otherwise (G_ALIGNED is chosen on the host).  Head and tail go
// to fixed threads of block 0.  Every access is inside [0, n).
template <bool G_ALIGNED>
__global__ __launch_bounds__(GA_THREADS)
void grad_accum_kernel(const short* __restrict__ g, float* __restrict__ acc,
                       long n) {
  long head = (long)(((16 - ((size_t)acc & 15)) & 15) >> 2);
  if (head > n) head = n;
  const long nvec = (n - head) / GA_VEC;
  const long tail0 = head + nvec * GA_VEC;
  const short* __restrict__ gb = g + head;
  float* __restrict__ ab = acc + head;

  const long stride = (long)gridDim.x * GA_THREADS;
#pragma unroll 2
  for (long i = (long)blockIdx.x * GA_THREADS + threadIdx.x; i < nvec;
       i += stride) {
    s16x8 x;
    if (G_ALIGNED) {
      x = *(const s16x8*)(gb + i * GA_VEC);
    } else {
#pragma unroll
      for (int j = 0; j < GA_VEC; ++j) x[j] = gb[i * GA_VEC + j];
    }
    f32x4* ap = (f32x4*)(ab + i * GA_VEC);
    f32x4 a0 = ap[0];
    f32x4 a1 = ap[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a0[j] += bfbits2f(x[j]);
      a1[j] += bfbits2f(x[4 + j]);
    }
    ap[0] = a0;
    ap[1] = a1;
  }
  if (blockIdx.x == 0) {
    const long t = threadIdx.x;
    if (t < head) acc[t] += bfbits2f(g[t]);
    if (t < GA_VEC && tail0 + t < n) acc[tail0 + t] += bfbits2f(g[tail0 + t]);
  }
}

int64_t grad_accum_max_blocks() { return GA_MAX_BLOCKS; }

// acc (fp32, 1-D contiguous) += grad (bf16, 1-D contiguous, same length >= 1).
// grad's base need only be 2-byte aligned, acc's 4-byte aligned.
void grad_accum(torch::Tensor grad, torch::Tensor acc) {
  TORCH_CHECK(grad.is_cuda() && grad.dtype() == torch::kBFloat16 &&
              grad.dim() == 1 && grad.is_contiguous() && grad.numel() >= 1);
  TORCH_CHECK(acc.is_cuda() && acc.dtype() == torch::kFloat32 &&
              acc.dim() == 1 && acc.is_contiguous());
  TORCH_CHECK(acc.numel() == grad.numel(), "grad_accum: accumulator holds ",
              acc.numel(), " elements, gradient ", grad.numel());
  TORCH_CHECK(acc.get_device() == grad.get_device());
  const long n = grad.numel();
  const short* g = (const short*)grad.data_ptr();
  float* a = acc.data_ptr<float>();
  const size_t head = ((16 - ((size_t)a & 15)) & 15) >> 2;
  const bool g_aligned = (((size_t)g + 2 * head) & 15) == 0;
  auto stream = at::hip::getCurrentHIPStream();
  if (g_aligned)
    grad_accum_kernel<true><<<ga_blocks(n), GA_THREADS, 0, stream>>>(g, a, n);
  else
    grad_accum_kernel<false><<<ga_blocks(n), GA_THREADS, 0, stream>>>(g, a, n);
}
