// Fused flat-buffer Adam (reference train.py:65-66:
// β1=0.9, β2=0.98, ε=1e-9, Noam LR computed host-side per step).
// One kernel over the whole flat parameter set: fp32 master weights + m/v,
// bf16 gradient in, bf16 parameter copy out (the model's live weights).
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

// Vectorized: 28 B/param of HBM traffic (fp32 master/m/v RW + bf16 g/p),
// f32x4 + s16x4 transactions so the kernel runs at memory speed-of-light.
__global__ void adam_kernel(float* __restrict__ master, float* __restrict__ m,
                            float* __restrict__ v,
                            const short* __restrict__ grad,
                            short* __restrict__ param, long n, float lr,
                            float b1, float b2, float eps, float bc1,
                            float bc2) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 4 <= n) {
    f32x4 mm = *(const f32x4*)(m + i);
    f32x4 vv = *(const f32x4*)(v + i);
    f32x4 ww = *(const f32x4*)(master + i);
    s16x4 g4 = *(const s16x4*)(grad + i);
    s16x4 p4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float g = bfbits2f(g4[j]);
      float mj = b1 * mm[j] + (1.f - b1) * g;
      float vj = b2 * vv[j] + (1.f - b2) * g * g;
      mm[j] = mj;
      vv[j] = vj;
      float w = ww[j] - lr * (mj * bc1) / (sqrtf(vj * bc2) + eps);
      ww[j] = w;
      p4[j] = f2bfbits(w);
    }
    *(f32x4*)(m + i) = mm;
    *(f32x4*)(v + i) = vv;
    *(f32x4*)(master + i) = ww;
    *(s16x4*)(param + i) = p4;
  } else {
    for (long j = i; j < n; ++j) {
      float g = bfbits2f(grad[j]);
      float mj = b1 * m[j] + (1.f - b1) * g;
      float vj = b2 * v[j] + (1.f - b2) * g * g;
      m[j] = mj;
      v[j] = vj;
      float w = master[j] - lr * (mj * bc1) / (sqrtf(vj * bc2) + eps);
      master[j] = w;
      param[j] = f2bfbits(w);
    }
  }
}

// Device-side schedule prelude for HIP-graph capture (Q12): ONE thread
// increments the step tensor and derives {lr, bc1, bc2} so a captured
// graph replays with a advancing Noam schedule instead of baked host
// constants.  lr = d_model^-0.5 * min(step^-0.5, step * warmup^-1.5).
__global__ void adam_coefs_kernel(long long* __restrict__ step,
                                  float* __restrict__ coefs, float dmr,
                                  float warmup_pow, float b1, float b2) {
  long long s = *step + 1;
  *step = s;
  float fs = (float)s;
  float lr = dmr * fminf(rsqrtf(fs), fs * warmup_pow);
  coefs[0] = lr;
  coefs[1] = 1.0f / (1.0f - powf(b1, fs));
  coefs[2] = 1.0f / (1.0f - powf(b2, fs));
}

// Variant of adam_kernel whose lr/bias-corrections come from the coefs
// buffer written by adam_coefs_kernel (graph-capturable).
__global__ void adam_dev_kernel(float* __restrict__ master,
                                float* __restrict__ m, float* __restrict__ v,
                                const short* __restrict__ grad,
                                short* __restrict__ param, long n,
                                const float* __restrict__ coefs, float b1,
                                float b2, float eps) {
  const float lr = coefs[0], bc1 = coefs[1], bc2 = coefs[2];
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 4 <= n) {
    f32x4 mm = *(const f32x4*)(m + i);
    f32x4 vv = *(const f32x4*)(v + i);
    f32x4 ww = *(const f32x4*)(master + i);
    s16x4 g4 = *(const s16x4*)(grad + i);
    s16x4 p4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float g = bfbits2f(g4[j]);
      float mj = b1 * mm[j] + (1.f - b1) * g;
      float vj = b2 * vv[j] + (1.f - b2) * g * g;
      mm[j] = mj;
      vv[j] = vj;
      float w = ww[j] - lr * (mj * bc1) / (sqrtf(vj * bc2) + eps);
      ww[j] = w;
      p4[j] = f2bfbits(w);
    }
    *(f32x4*)(m + i) = mm;
    *(f32x4*)(v + i) = vv;
    *(f32x4*)(master + i) = ww;
    *(s16x4*)(param + i) = p4;
  } else {
    for (long j = i; j < n; ++j) {
      float g = bfbits2f(grad[j]);
      float mj = b1 * m[j] + (1.f - b1) * g;
      float vj = b2 * v[j] + (1.f - b2) * g * g;
      m[j] = mj;
      v[j] = vj;
      float w = master[j] - lr * (mj * bc1) / (sqrtf(vj * bc2) + eps);
      master[j] = w;
      param[j] = f2bfbits(w);
    }
  }
}

// ---- clipped / skippable variants -----------------------------------------
// `stats` = {norm, scale, skipped_this_step, skipped_total}, written by
// grad_norm_clip (grad_clip.hip) earlier on the same stream.  The gradient is
// multiplied by stats[1] in fp32 before the m/v updates; when stats[2] != 0
// the kernel returns before any store (NOT a multiply by zero: 0*inf = NaN).
//
// Both clipped kernels share the one body below.  adam_kernel and
// adam_dev_kernel above keep their own text on purpose: routing them through
// a shared inline function made hipcc pick a different mul+add contraction
// for the m update, i.e. different last bits from what they produced before.
// The shared body therefore spells the fused multiply-adds out, in the form
// the vector path of adam_kernel compiles to, so that with scale == 1 a
// clipped update of a 4-aligned buffer is bit-identical to the unclipped one
// whatever the compiler would have chosen here.
DEV_INLINE float adam_elem(float g, float& mj, float& vj, float w, float lr,
                           float b1, float b2, float eps, float bc1,
                           float bc2) {
  mj = __builtin_fmaf(1.f - b1, g, b1 * mj);
  vj = __builtin_fmaf(b2, vj, (1.f - b2) * g * g);
  return w - lr * (mj * bc1) / (sqrtf(vj * bc2) + eps);
}

DEV_INLINE void adam_clip_update(float* __restrict__ master,
                                 float* __restrict__ m, float* __restrict__ v,
                                 const short* __restrict__ grad,
                                 short* __restrict__ param, long n, float lr,
                                 float b1, float b2, float eps, float bc1,
                                 float bc2, float gscale) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 4 <= n) {
    f32x4 mm = *(const f32x4*)(m + i);
    f32x4 vv = *(const f32x4*)(v + i);
    f32x4 ww = *(const f32x4*)(master + i);
    s16x4 g4 = *(const s16x4*)(grad + i);
    s16x4 p4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = mm[j], vj = vv[j];
      float w = adam_elem(bfbits2f(g4[j]) * gscale, mj, vj, ww[j], lr, b1, b2,
                          eps, bc1, bc2);
      mm[j] = mj;
      vv[j] = vj;
      ww[j] = w;
      p4[j] = f2bfbits(w);
    }
    *(f32x4*)(m + i) = mm;
    *(f32x4*)(v + i) = vv;
    *(f32x4*)(master + i) = ww;
    *(s16x4*)(param + i) = p4;
  } else {
    for (long j = i; j < n; ++j) {
      float mj = m[j], vj = v[j];
      float w = adam_elem(bfbits2f(grad[j]) * gscale, mj, vj, master[j], lr,
                          b1, b2, eps, bc1, bc2);
      m[j] = mj;
      v[j] = vj;
      master[j] = w;
      param[j] = f2bfbits(w);
    }
  }
}

__global__ void adam_clip_kernel(float* __restrict__ master,
                                 float* __restrict__ m, float* __restrict__ v,
                                 const short* __restrict__ grad,
                                 short* __restrict__ param, long n, float lr,
                                 float b1, float b2, float eps, float bc1,
                                 float bc2, const float* __restrict__ stats) {
  if (stats[2] != 0.f) return;
  adam_clip_update(master, m, v, grad, param, n, lr, b1, b2, eps, bc1, bc2,
                   stats[1]);
}

__global__ void adam_dev_clip_kernel(float* __restrict__ master,
                                     float* __restrict__ m,
                                     float* __restrict__ v,
                                     const short* __restrict__ grad,
                                     short* __restrict__ param, long n,
                                     const float* __restrict__ coefs, float b1,
                                     float b2, float eps,
                                     const float* __restrict__ stats) {
  if (stats[2] != 0.f) return;
  adam_clip_update(master, m, v, grad, param, n, coefs[0], b1, b2, eps,
                   coefs[1], coefs[2], stats[1]);
}

// Graph-capturable fused Adam: advances `step` (int64[1], device) and runs
// the update with the device-derived Noam lr.  d_model/warmup fixed.
void adam_fused_dev(torch::Tensor master, torch::Tensor m, torch::Tensor v,
                    torch::Tensor grad, torch::Tensor param,
                    torch::Tensor step, torch::Tensor coefs, double d_model,
                    double warmup, double beta1, double beta2, double eps) {
  TORCH_CHECK(master.dtype() == torch::kFloat32 && master.is_contiguous());
  TORCH_CHECK(step.dtype() == torch::kInt64 && step.numel() == 1 &&
              step.is_cuda());
  TORCH_CHECK(coefs.dtype() == torch::kFloat32 && coefs.numel() >= 3 &&
              coefs.is_cuda());
  long n = master.numel();
  auto stream = at::hip::getCurrentHIPStream();
  adam_coefs_kernel<<<1, 1, 0, stream>>>(
      (long long*)step.data_ptr(), coefs.data_ptr<float>(),
      1.0f / sqrtf((float)d_model),
      powf((float)warmup, -1.5f), (float)beta1, (float)beta2);
  adam_dev_kernel<<<((n + 3) / 4 + 255) / 256, 256, 0, stream>>>(
      master.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
      (const short*)grad.data_ptr(), (short*)param.data_ptr(), n,
      coefs.data_ptr<float>(), (float)beta1, (float)beta2, (float)eps);
}

void adam_fused(torch::Tensor master, torch::Tensor m, torch::Tensor v,
                torch::Tensor grad, torch::Tensor param, double lr,
                double beta1, double beta2, double eps, int64_t step) {
  TORCH_CHECK(master.dtype() == torch::kFloat32 && master.is_contiguous());
  TORCH_CHECK(grad.dtype() == torch::kBFloat16 && param.dtype() == torch::kBFloat16);
  long n = master.numel();
  TORCH_CHECK(m.numel() == n && v.numel() == n && grad.numel() == n &&
              param.numel() == n);
  float bc1 = 1.0f / (1.0f - powf((float)beta1, (float)step));
  float bc2 = 1.0f / (1.0f - powf((float)beta2, (float)step));
  auto stream = at::hip::getCurrentHIPStream();
  adam_kernel<<<((n + 3) / 4 + 255) / 256, 256, 0, stream>>>(
      master.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
      (const short*)grad.data_ptr(), (short*)param.data_ptr(), n, (float)lr,
      (float)beta1, (float)beta2, (float)eps, bc1, bc2);
}

static void check_clip_args(const torch::Tensor& master,
                            const torch::Tensor& m, const torch::Tensor& v,
                            const torch::Tensor& grad,
                            const torch::Tensor& param,
                            const torch::Tensor& stats) {
  TORCH_CHECK(master.is_cuda() && master.dtype() == torch::kFloat32 &&
              master.is_contiguous());
  TORCH_CHECK(m.is_cuda() && m.dtype() == torch::kFloat32 &&
              m.is_contiguous() && v.is_cuda() &&
              v.dtype() == torch::kFloat32 && v.is_contiguous());
  TORCH_CHECK(grad.is_cuda() && grad.dtype() == torch::kBFloat16 &&
              grad.is_contiguous() && param.is_cuda() &&
              param.dtype() == torch::kBFloat16 && param.is_contiguous());
  const long n = master.numel();
  TORCH_CHECK(m.numel() == n && v.numel() == n && grad.numel() == n &&
              param.numel() == n);
  TORCH_CHECK(stats.is_cuda() && stats.dtype() == torch::kFloat32 &&
              stats.is_contiguous() && stats.numel() >= 4);
  TORCH_CHECK(stats.get_device() == master.get_device() &&
              grad.get_device() == master.get_device());
}

// adam_fused with the gradient scaled by stats[1] (fp32, before the m/v
// updates) and the whole update vetoed when stats[2] != 0.  `stats` is the
// buffer written by grad_norm_clip on the same stream.
void adam_fused_clip(torch::Tensor master, torch::Tensor m, torch::Tensor v,
                     torch::Tensor grad, torch::Tensor param, double lr,
                     double beta1, double beta2, double eps, int64_t step,
                     torch::Tensor stats) {
  check_clip_args(master, m, v, grad, param, stats);
  long n = master.numel();
  float bc1 = 1.0f / (1.0f - powf((float)beta1, (float)step));
  float bc2 = 1.0f / (1.0f - powf((float)beta2, (float)step));
  auto stream = at::hip::getCurrentHIPStream();
  adam_clip_kernel<<<((n + 3) / 4 + 255) / 256, 256, 0, stream>>>(
      master.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
      (const short*)grad.data_ptr(), (short*)param.data_ptr(), n, (float)lr,
      (float)beta1, (float)beta2, (float)eps, bc1, bc2,
      stats.data_ptr<float>());
}

// Graph-capturable clipped Adam.  The device step tensor advances even on a
// skipped step, so the Noam schedule and the host step counter stay in
// lock-step with no sync.
void adam_fused_dev_clip(torch::Tensor master, torch::Tensor m,
                         torch::Tensor v, torch::Tensor grad,
                         torch::Tensor param, torch::Tensor step,
                         torch::Tensor coefs, double d_model, double warmup,
                         double beta1, double beta2, double eps,
                         torch::Tensor stats) {
  check_clip_args(master, m, v, grad, param, stats);
  TORCH_CHECK(step.dtype() == torch::kInt64 && step.numel() == 1 &&
              step.is_cuda());
  TORCH_CHECK(coefs.dtype() == torch::kFloat32 && coefs.numel() >= 3 &&
              coefs.is_cuda());
  long n = master.numel();
  auto stream = at::hip::getCurrentHIPStream();
  adam_coefs_kernel<<<1, 1, 0, stream>>>(
      (long long*)step.data_ptr(), coefs.data_ptr<float>(),
      1.0f / sqrtf((float)d_model),
      powf((float)warmup, -1.5f), (float)beta1, (float)beta2);
  adam_dev_clip_kernel<<<((n + 3) / 4 + 255) / 256, 256, 0, stream>>>(
      master.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
      (const short*)grad.data_ptr(), (short*)param.data_ptr(), n,
      coefs.data_ptr<float>(), (float)beta1, (float)beta2, (float)eps,
      stats.data_ptr<float>());
}

// ---- accumulator-reading variants (gradient accumulation) -----------------
// The gradient is the fp32 accumulator filled by grad_accum (grad_accum.hip)
// instead of the bf16 flat gradient.  Same adam_elem body, so with the
// accumulator holding bf16-representable values and a 4-aligned length the
// update is bit-identical to the bf16-gradient kernels above.  Every thread
// also stores ZEROS back over the accumulator elements it read: that restores
// the "all-zero between optimizer steps" invariant grad_accum relies on, for
// +4 B/param in a pass that already reads the buffer.  `stats` may be null
// (scale 1, never vetoed).  On a vetoed step (stats[2] != 0) master/m/v/param
// are not touched but the accumulator is still zeroed — a poisoned sum must
// not leak into the next step.
DEV_INLINE void adam_acc_update(float* __restrict__ master,
                                float* __restrict__ m, float* __restrict__ v,
                                float* __restrict__ acc,
                                short* __restrict__ param, long n, float lr,
                                float b1, float b2, float eps, float bc1,
                                float bc2, const float* __restrict__ stats) {
  const bool veto = stats != nullptr && stats[2] != 0.f;
  const float gscale = (stats != nullptr && !veto) ? stats[1] : 1.0f;
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 4 <= n) {
    if (!veto) {
      f32x4 mm = *(const f32x4*)(m + i);
      f32x4 vv = *(const f32x4*)(v + i);
      f32x4 ww = *(const f32x4*)(master + i);
      f32x4 g4 = *(const f32x4*)(acc + i);
      s16x4 p4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float mj = mm[j], vj = vv[j];
        float w = adam_elem(g4[j] * gscale, mj, vj, ww[j], lr, b1, b2, eps,
                            bc1, bc2);
        mm[j] = mj;
        vv[j] = vj;
        ww[j] = w;
        p4[j] = f2bfbits(w);
      }
      *(f32x4*)(m + i) = mm;
      *(f32x4*)(v + i) = vv;
      *(f32x4*)(master + i) = ww;
      *(s16x4*)(param + i) = p4;
    }
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    *(f32x4*)(acc + i) = z;
  } else {
    for (long j = i; j < n; ++j) {
      if (!veto) {
        float mj = m[j], vj = v[j];
        float w = adam_elem(acc[j] * gscale, mj, vj, master[j], lr, b1, b2,
                            eps, bc1, bc2);
        m[j] = mj;
        v[j] = vj;
        master[j] = w;
        param[j] = f2bfbits(w);
      }
      acc[j] = 0.f;
    }
  }
}

__global__ void adam_acc_kernel(float* __restrict__ master,
                                float* __restrict__ m, float* __restrict__ v,
                                float* __restrict__ acc,
                                short* __restrict__ param, long n, float lr,
                                float b1, float b2, float eps, float bc1,
                                float bc2, const float* __restrict__ stats) {
  adam_acc_update(master, m, v, acc, param, n, lr, b1, b2, eps, bc1, bc2,
                  stats);
}

__global__ void adam_dev_acc_kernel(float* __restrict__ master,
                                    float* __restrict__ m,
                                    float* __restrict__ v,
                                    float* __restrict__ acc,
                                    short* __restrict__ param, long n,
                                    const float* __restrict__ coefs, float b1,
                                    float b2, float eps,
                                    const float* __restrict__ stats) {
  adam_acc_update(master, m, v, acc, param, n, coefs[0], b1, b2, eps,
                  coefs[1], coefs[2], stats);
}

static const float* check_acc_args(const torch::Tensor& master,
                                   const torch::Tensor& m,
                                   const torch::Tensor& v,
                                   const torch::Tensor& acc,
                                   const torch::Tensor& param,
                                   const c10::optional<torch::Tensor>& stats) {
  TORCH_CHECK(master.is_cuda() && master.dtype() == torch::kFloat32 &&
              master.is_contiguous());
  TORCH_CHECK(m.is_cuda() && m.dtype() == torch::kFloat32 &&
              m.is_contiguous() && v.is_cuda() &&
              v.dtype() == torch::kFloat32 && v.is_contiguous());
  TORCH_CHECK(acc.is_cuda() && acc.dtype() == torch::kFloat32 &&
              acc.is_contiguous());
  TORCH_CHECK(param.is_cuda() && param.dtype() == torch::kBFloat16 &&
              param.is_contiguous());
  const long n = master.numel();
  TORCH_CHECK(m.numel() == n && v.numel() == n && acc.numel() == n &&
              param.numel() == n);
  // the vector path reads f32x4 / s16x4 at the bases
  TORCH_CHECK(((size_t)master.data_ptr() & 15) == 0 &&
              ((size_t)m.data_ptr() & 15) == 0 &&
              ((size_t)v.data_ptr() & 15) == 0 &&
              ((size_t)acc.data_ptr() & 15) == 0 &&
              ((size_t)param.data_ptr() & 7) == 0,
              "adam_fused_acc: buffers must be 16-byte aligned");
  TORCH_CHECK(acc.get_device() == master.get_device() &&
              param.get_device() == master.get_device());
  if (!stats.has_value()) return nullptr;
  const torch::Tensor& st = *stats;
  TORCH_CHECK(st.is_cuda() && st.dtype() == torch::kFloat32 &&
              st.is_contiguous() && st.numel() >= 4 &&
              st.get_device() == master.get_device());
  return st.data_ptr<float>();
}

// adam_fused with the fp32 accumulator as the gradient; the accumulator is
// all-zero afterwards.  `stats` (optional) as in adam_fused_clip.
void adam_fused_acc(torch::Tensor master, torch::Tensor m, torch::Tensor v,
                    torch::Tensor acc, torch::Tensor param, double lr,
                    double beta1, double beta2, double eps, int64_t step,
                    c10::optional<torch::Tensor> stats) {
  const float* st = check_acc_args(master, m, v, acc, param, stats);
  long n = master.numel();
  float bc1 = 1.0f / (1.0f - powf((float)beta1, (float)step));
  float bc2 = 1.0f / (1.0f - powf((float)beta2, (float)step));
  auto stream = at::hip::getCurrentHIPStream();
  adam_acc_kernel<<<((n + 3) / 4 + 255) / 256, 256, 0, stream>>>(
      master.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
      acc.data_ptr<float>(), (short*)param.data_ptr(), n, (float)lr,
      (float)beta1, (float)beta2, (float)eps, bc1, bc2, st);
}

// Graph-capturable form: device step tensor + in-kernel Noam lr, as
// adam_fused_dev(_clip).  The step tensor advances on a vetoed step too.
void adam_fused_dev_acc(torch::Tensor master, torch::Tensor m,
                        torch::Tensor v, torch::Tensor acc,
                        torch::Tensor param, torch::Tensor step,
                        torch::Tensor coefs, double d_model, double warmup,
                        double beta1, double beta2, double eps,
                        c10::optional<torch::Tensor> stats) {
  const float* st = check_acc_args(master, m, v, acc, param, stats);
  TORCH_CHECK(step.dtype() == torch::kInt64 && step.numel() == 1 &&
              step.is_cuda());
  TORCH_CHECK(coefs.dtype() == torch::kFloat32 && coefs.numel() >= 3 &&
              coefs.is_cuda());
  long n = master.numel();
  auto stream = at::hip::getCurrentHIPStream();
  adam_coefs_kernel<<<1, 1, 0, stream>>>(
      (long long*)step.data_ptr(), coefs.data_ptr<float>(),
      1.0f / sqrtf((float)d_model),
      powf((float)warmup, -1.5f), (float)beta1, (float)beta2);
  adam_dev_acc_kernel<<<((n + 3) / 4 + 255) / 256, 256, 0, stream>>>(
      master.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
      acc.data_ptr<float>(), (short*)param.data_ptr(), n,
      coefs.data_ptr<float>(), (float)beta1, (float)beta2, (float)eps, st);
}
