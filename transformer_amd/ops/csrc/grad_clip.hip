// Global gradient norm + clip/skip decision for the flat bf16 gradient buffer
// (runtime/optimizer.py FlatParams.flat_g).  Two plain launches, no atomics,
// so the result is bit-reproducible and the pair is hipGraph-capturable:
//
//   stage 1  grad_sumsq_kernel     per-block fp32 partial sums of squares
//   stage 2  grad_norm_finalize_kernel  fixed-order sum of the partials, then
//            stats = {norm, scale, skipped_this_step, skipped_total}
//
// The clipped Adam variants (adam.hip) read `scale` and `skipped_this_step`
// from the stats buffer, so the whole guard lives on the device: a captured
// step is vetoed in-graph with no host sync.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

constexpr int GN_THREADS = 256;     // 4 waves
constexpr int GN_VEC = 8;           // bf16 per 16-byte load
constexpr int GN_MAX_BLOCKS = 2048; // 8 blocks/CU on 256 CUs

// Number of stage-1 blocks: a function of n only (never of the device or the
// launch history), so the summation tree — and the result bits — depend on n
// alone.
static inline int gn_blocks(long n) {
  long b = (n + (long)GN_THREADS * GN_VEC - 1) / ((long)GN_THREADS * GN_VEC);
  if (b < 1) b = 1;
  return (int)(b < GN_MAX_BLOCKS ? b : GN_MAX_BLOCKS);
}

// Stage 1.  The buffer is split into a scalar head (< 8 elements, up to the
// first 16-byte boundary), a 16-byte-aligned body read as s16x8 by a
// grid-stride loop, and a scalar tail (< 8 elements).  Head and tail go to
// fixed threads of block 0.  Each thread keeps one fp32 accumulator per
// vector lane, so its longest add chain is (body iterations + 3), not
// 8 x iterations.
__global__ __launch_bounds__(GN_THREADS)
void grad_sumsq_kernel(const short* __restrict__ g, long n,
                       float* __restrict__ partials) {
  long head = (long)(((16 - ((size_t)g & 15)) & 15) >> 1);
  if (head > n) head = n;
  const long nvec = (n - head) / GN_VEC;
  const long tail0 = head + nvec * GN_VEC;
  const s16x8* __restrict__ body = (const s16x8*)(g + head);

  float acc[GN_VEC];
#pragma unroll
  for (int j = 0; j < GN_VEC; ++j) acc[j] = 0.f;

  const long stride = (long)gridDim.x * GN_THREADS;
#pragma unroll 4
  for (long i = (long)blockIdx.x * GN_THREADS + threadIdx.x; i < nvec;
       i += stride) {
    s16x8 x = body[i];
#pragma unroll
    for (int j = 0; j < GN_VEC; ++j) {
      float f = bfbits2f(x[j]);
      acc[j] += f * f;
    }
  }
  if (blockIdx.x == 0) {
    const long t = threadIdx.x;
    if (t < head) {
      float f = bfbits2f(g[t]);
      acc[0] += f * f;
    }
    if (tail0 + t < n && t < GN_VEC) {
      float f = bfbits2f(g[tail0 + t]);
      acc[1] += f * f;
    }
  }
  float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
            ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  s = wave_sum(s);

  __shared__ float wsum[GN_THREADS / WAVE];
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// Stage 1 for the fp32 gradient accumulator (grad_accum.hip).  Same split,
// same 8 elements per thread per trip (two f32x4 loads), same per-lane
// accumulators and the same combine tree as grad_sumsq_kernel, launched on
// the same gn_blocks(n) grid, so the workspace size, the add-chain length
// and the "result bits depend on n alone" property carry over.  The head is
// < 4 elements (up to the first 16-byte boundary of a 4-byte-aligned base).
__global__ __launch_bounds__(GN_THREADS)
void grad_sumsq_f32_kernel(const float* __restrict__ g, long n,
                           float* __restrict__ partials) {
  long head = (long)(((16 - ((size_t)g & 15)) & 15) >> 2);
  if (head > n) head = n;
  const long nvec = (n - head) / GN_VEC;
  const long tail0 = head + nvec * GN_VEC;
  const f32x4* __restrict__ body = (const f32x4*)(g + head);

  float acc[GN_VEC];
#pragma unroll
  for (int j = 0; j < GN_VEC; ++j) acc[j] = 0.f;

  const long stride = (long)gridDim.x * GN_THREADS;
#pragma unroll 4
  for (long i = (long)blockIdx.x * GN_THREADS + threadIdx.x; i < nvec;
       i += stride) {
    f32x4 x0 = body[2 * i];
    f32x4 x1 = body[2 * i + 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] += x0[j] * x0[j];
      acc[4 + j] += x1[j] * x1[j];
    }
  }
  if (blockIdx.x == 0) {
    const long t = threadIdx.x;
    if (t < head) {
      float f = g[t];
      acc[0] += f * f;
    }
    if (tail0 + t < n && t < GN_VEC) {
      float f = g[tail0 + t];
      acc[1] += f * f;
    }
  }
  float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
            ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  s = wave_sum(s);

  __shared__ float wsum[GN_THREADS / WAVE];
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// Stage 2: one block.  Thread t sums partials t, t+256, ... in double, then a
// fixed LDS tree combines the 256 doubles.  Thread 0 applies the rules:
//   scale = 1.0f exactly          when max_norm <= 0 or norm <= max_norm
//         = max_norm/(norm+1e-6f) otherwise
//   skip  iff skipping is enabled and the fp32 sum of squares is not finite.
// "Not finite" deliberately includes fp32 overflow of a finite but absurd
// gradient (sum of squares > FLT_MAX, i.e. norm > ~1.8e19): such a step is
// skipped too.  skipped_total accumulates on the device (exact in fp32 up to
// 2^24 skips).
__global__ __launch_bounds__(GN_THREADS)
void grad_norm_finalize_kernel(const float* __restrict__ partials, int nparts,
                               float max_norm, int skip_nonfinite,
                               float* __restrict__ stats) {
  __shared__ double red[GN_THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += GN_THREADS)
    s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = GN_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double total = red[0];
    const float ssf = (float)total;  // > FLT_MAX rounds to +inf
    union { float f; unsigned int u; } c;
    c.f = ssf;
    const bool finite = (c.u & 0x7f800000u) != 0x7f800000u;
    const float norm = (float)sqrt(total);
    float scale = 1.0f;
    if (max_norm > 0.f && !(norm <= max_norm))
      scale = max_norm / (norm + 1e-6f);
    const float skipped = (skip_nonfinite && !finite) ? 1.0f : 0.0f;
    stats[0] = norm;
    stats[1] = scale;
    stats[2] = skipped;
    stats[3] = stats[3] + skipped;
  }
}

int64_t grad_norm_blocks(int64_t n) { return gn_blocks((long)n); }
int64_t grad_norm_max_blocks() { return GN_MAX_BLOCKS; }

// stats (fp32[>=4], device) <- {norm, scale, skipped_this_step, skipped_total}
// for the 1-D contiguous bf16 tensor `grad` (any length >= 1; the base need
// only be 2-byte aligned).  `partials` is a caller-owned fp32 workspace of at
// least grad_norm_blocks(n) elements — allocated once, outside any capture.
void grad_norm_clip(torch::Tensor grad, torch::Tensor partials,
                    torch::Tensor stats, double max_norm,
                    bool skip_nonfinite) {
  TORCH_CHECK(grad.is_cuda() && grad.dtype() == torch::kBFloat16 &&
              grad.dim() == 1 && grad.is_contiguous() && grad.numel() >= 1);
  TORCH_CHECK(partials.is_cuda() && partials.dtype() == torch::kFloat32 &&
              partials.is_contiguous());
  TORCH_CHECK(stats.is_cuda() && stats.dtype() == torch::kFloat32 &&
              stats.is_contiguous() && stats.numel() >= 4);
  TORCH_CHECK(partials.get_device() == grad.get_device() &&
              stats.get_device() == grad.get_device());
  const long n = grad.numel();
  const int nb = gn_blocks(n);
  TORCH_CHECK(partials.numel() >= nb, "grad_norm_clip: workspace holds ",
              partials.numel(), " partials, need ", nb);
  auto stream = at::hip::getCurrentHIPStream();
  grad_sumsq_kernel<<<nb, GN_THREADS, 0, stream>>>(
      (const short*)grad.data_ptr(), n, partials.data_ptr<float>());
  grad_norm_finalize_kernel<<<1, GN_THREADS, 0, stream>>>(
      partials.data_ptr<float>(), nb, (float)max_norm,
      skip_nonfinite ? 1 : 0, stats.data_ptr<float>());
}

// grad_norm_clip for the fp32 gradient accumulator: fp32 stage 1, the same
// finalize, hence the same stats layout and rules.  The base of `acc` need
// only be 4-byte aligned.
void grad_norm_clip_f32(torch::Tensor acc, torch::Tensor partials,
                        torch::Tensor stats, double max_norm,
                        bool skip_nonfinite) {
  TORCH_CHECK(acc.is_cuda() && acc.dtype() == torch::kFloat32 &&
              acc.dim() == 1 && acc.is_contiguous() && acc.numel() >= 1);
  TORCH_CHECK(partials.is_cuda() && partials.dtype() == torch::kFloat32 &&
              partials.is_contiguous());
  TORCH_CHECK(stats.is_cuda() && stats.dtype() == torch::kFloat32 &&
              stats.is_contiguous() && stats.numel() >= 4);
  TORCH_CHECK(partials.get_device() == acc.get_device() &&
              stats.get_device() == acc.get_device());
  const long n = acc.numel();
  const int nb = gn_blocks(n);
  TORCH_CHECK(partials.numel() >= nb, "grad_norm_clip_f32: workspace holds ",
              partials.numel(), " partials, need ", nb);
  auto stream = at::hip::getCurrentHIPStream();
  grad_sumsq_f32_kernel<<<nb, GN_THREADS, 0, stream>>>(
      acc.data_ptr<float>(), n, partials.data_ptr<float>());
  grad_norm_finalize_kernel<<<1, GN_THREADS, 0, stream>>>(
      partials.data_ptr<float>(), nb, (float)max_norm,
      skip_nonfinite ? 1 : 0, stats.data_ptr<float>());
}
