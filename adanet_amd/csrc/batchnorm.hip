// BatchNorm2d fwd/bwd (K8 remainder): per-channel statistics over N*H*W,
// bf16 NCHW activations with fp32 stats/affine — replaces the round-1
// torch nn.BatchNorm2d fallback in the NASNet cells (reference arg scopes
// research/improve_nas/trainer/nasnet.py:127-233).
//
// Structure: one 256-thread block per (channel, image chunk) for the
// reductions (bn_sweep: vectorized short8 row loads when HW%8==0; block sum
// into the chunk's slot, then one wave per channel over the slots) and a
// grid-stride elementwise kernel for normalize / dx. dgamma == sum
// dy*xhat and dbeta == sum dy fall out of the backward reduction for free.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

namespace {

struct bn8 {
  bf16_t v[8];
};

// One channel's elements of images [n0, n1) over the 256-thread block:
// short8 loads when HW % 8 == 0, scalar loads otherwise. f gets one element
// of each of the NP tensors at a time.
template <int NP, typename F>
__device__ __forceinline__ void bn_sweep(const bf16_t* const (&p)[NP], int n0,
                                         int n1, int C, int c, int64_t HW,
                                         F f) {
  const int tid = threadIdx.x;
  for (int n = n0; n < n1; ++n) {
    const int64_t off = ((int64_t)n * C + c) * HW;
    if ((HW & 7) == 0) {
      for (int64_t i = (int64_t)tid * 8; i < HW; i += 256 * 8) {
        bn8 v[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) v[j] = *(const bn8*)(p[j] + off + i);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float e[NP];
#pragma unroll
          for (int j = 0; j < NP; ++j) e[j] = bf2f(v[j].v[k]);
          f(e);
        }
      }
    } else {
      for (int64_t i = tid; i < HW; i += 256) {
        float e[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) e[j] = bf2f(p[j][off + i]);
        f(e);
      }
    }
  }
}

// mean, clamped variance and rstd of channel c from its sum and sum of
// squares, plus the running-stat update (unbiased variance).
__device__ __forceinline__ void bn_finish_stats(
    float s, float s2, int c, int N, int64_t HW, float eps, float momentum,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    float* __restrict__ running_mean, float* __restrict__ running_var) {
  const double M = (double)N * (double)HW;
  const float mean = (float)(s / M);
  float var = (float)(s2 / M) - mean * mean;
  var = var > 0.f ? var : 0.f;
  mean_out[c] = mean;
  rstd_out[c] = rsqrtf(var + eps);
  if (running_mean) {
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    const float unbiased = M > 1.0 ? var * (float)(M / (M - 1.0)) : var;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
}

// Chunked partial sums: grid (C, nchunks) so small-C shapes still fill
// the chip (a C-block grid was 30% of the improve_nas step on 32 CUs,
// profiles/nasprof3_summary.txt). Each block writes its OWN workspace
// slot wsp[chunk][2][C]; the finalize kernel sums chunks in fixed order —
// deterministic, and the workspace needs no zero-fill (the at::zeros +
// .zero_() launches were 2.9% of the step, profiles/nasprof6_summary).
// A single chunk (N == 1 or C > 1024) finishes in place: no workspace, no
// second launch.
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(
    const bf16_t* __restrict__ x, float* __restrict__ wsp,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    float* __restrict__ running_mean, float* __restrict__ running_var, int N,
    int C, int64_t HW, float eps, float momentum) {
  const int c = blockIdx.x;
  const int n0 = (N * blockIdx.y) / gridDim.y;
  const int n1 = (N * (blockIdx.y + 1)) / gridDim.y;
  float acc[2] = {0.f, 0.f};  // sum x, sum x^2
  bn_sweep<1>({x}, n0, n1, C, c, HW, [&](const float(&e)[1]) {
    acc[0] += e[0];
    acc[1] += e[0] * e[0];
  });
  float tot[2];
  block_reduce_sum(acc, [&](int t, float v) { tot[t] = v; });
  if (threadIdx.x != 0) return;
  if (gridDim.y == 1) {
    bn_finish_stats(tot[0], tot[1], c, N, HW, eps, momentum, mean_out,
                    rstd_out, running_mean, running_var);
  } else {
    float* slot = wsp + (int64_t)blockIdx.y * 2 * C;
    slot[c] = tot[0];
    slot[C + c] = tot[1];
  }
}

// One wave per channel, lanes over chunks (fixed-tree reduce — the
// thread-per-channel loop serialized nchunks loads on a near-empty
// chip: 7 us/call, 1.2% of the NASNet step, profiles/nasprof8).
__global__ __launch_bounds__(256) void bn_stats_finalize_kernel(
    const float* __restrict__ wsp, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, float* __restrict__ running_mean,
    float* __restrict__ running_var, int N, int C, int64_t HW, float eps,
    float momentum, int nchunks) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const float s = wave_slot_sum(wsp + c, 2 * C, nchunks);
  const float s2 = wave_slot_sum(wsp + C + c, 2 * C, nchunks);
  if ((threadIdx.x & 63) != 0) return;
  bn_finish_stats(s, s2, c, N, HW, eps, momentum, mean_out, rstd_out,
                  running_mean, running_var);
}

// y = (x - mean[c]) * rstd[c] * gamma[c] + beta[c]
__global__ __launch_bounds__(256) void bn_norm_kernel(
    const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta, int C,
    int64_t HW, int64_t total) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)((p / HW) % C);
    const float g = gamma ? gamma[c] : 1.f;
    const float b = beta ? beta[c] : 0.f;
    y[p] = f2bf((bf2f(x[p]) - mean[c]) * rstd[c] * g + b);
  }
}

// Per-channel backward sums: sdy = sum dy (== dbeta), sdyx = sum dy*xhat
// (== dgamma). Grid (C, nchunks), per-chunk workspace slots wsp[chunk][2][C]
// + fixed-order finalize (deterministic; no host zero-fill); a single chunk
// writes sdy/sdyx itself.
__global__ __launch_bounds__(256) void bn_bwd_reduce_chunked_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ wsp, float* __restrict__ sdy,
    float* __restrict__ sdyx, int N, int C, int64_t HW) {
  const int c = blockIdx.x;
  const int n0 = (N * blockIdx.y) / gridDim.y;
  const int n1 = (N * (blockIdx.y + 1)) / gridDim.y;
  const float m = mean[c], r = rstd[c];
  float acc[2] = {0.f, 0.f};  // sum dy, sum dy*xhat
  bn_sweep<2>({dy, x}, n0, n1, C, c, HW, [&](const float(&e)[2]) {
    acc[0] += e[0];
    acc[1] += e[0] * (e[1] - m) * r;
  });
  float* slot = wsp + (int64_t)blockIdx.y * 2 * C;
  float* const out[2] = {gridDim.y == 1 ? sdy : slot,
                         gridDim.y == 1 ? sdyx : slot + C};
  block_reduce_sum(acc, [&](int t, float v) { out[t][c] = v; });
}

// sdy/sdyx[c] = sum over chunks: wave per channel, lanes over chunks.
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(
    const float* __restrict__ wsp, float* __restrict__ sdy,
    float* __restrict__ sdyx, int C, int nchunks) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const float a = wave_slot_sum(wsp + c, 2 * C, nchunks);
  const float b = wave_slot_sum(wsp + C + c, 2 * C, nchunks);
  if ((threadIdx.x & 63) == 0) {
    sdy[c] = a;
    sdyx[c] = b;
  }
}

// dx = gamma*rstd * (dy - sdy/M - xhat * sdyx/M)
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
    bf16_t* __restrict__ dx, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ sdy, const float* __restrict__ sdyx, int C,
    int64_t HW, int64_t total, float invM) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)((p / HW) % C);
    const float g = gamma ? gamma[c] : 1.f;
    const float xh = (bf2f(x[p]) - mean[c]) * rstd[c];
    dx[p] = f2bf(g * rstd[c] *
                 (bf2f(dy[p]) - sdy[c] * invM - xh * sdyx[c] * invM));
  }
}

int grid_for(int64_t total) {
  return (int)std::min<int64_t>((total + 255) / 256, 2048);
}

// Image chunks per channel for the two reductions: about 2048 blocks in
// all, at most one chunk per image and 64 chunks (one finalize lane each).
int bn_nchunks(int N, int C) {
  return (int)std::max<int64_t>(
      1, std::min<int64_t>(2048 / C, std::min<int64_t>(N, 64)));
}

float* opt_ptr(const c10::optional<at::Tensor>& t) {
  return t.has_value() && t->defined() ? t->data_ptr<float>() : nullptr;
}

}  // namespace

void batchnorm_stats(const at::Tensor& x, at::Tensor& mean, at::Tensor& rstd,
                     const c10::optional<at::Tensor>& running_mean,
                     const c10::optional<at::Tensor>& running_var,
                     double eps, double momentum) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.is_contiguous() &&
              x.scalar_type() == at::kBFloat16, "bn_stats: bf16 NCHW");
  const int N = (int)x.size(0), C = (int)x.size(1);
  const int64_t HW = x.size(2) * x.size(3);
  auto stream = at::cuda::getCurrentCUDAStream();
  float* rm = opt_ptr(running_mean);
  float* rv = opt_ptr(running_var);
  TORCH_CHECK((rm == nullptr) == (rv == nullptr),
              "bn_stats: running_mean and running_var come together");
  const int nchunks = bn_nchunks(N, C);
  float* wsp = nullptr;
  at::Tensor wsp_t;
  if (nchunks > 1) {
    wsp_t = at::empty({nchunks, 2, C}, x.options().dtype(at::kFloat));
    wsp = wsp_t.data_ptr<float>();
  }
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(C, nchunks), dim3(256), 0,
                     stream.stream(), (const bf16_t*)x.data_ptr(), wsp,
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), rm, rv,
                     N, C, HW, (float)eps, (float)momentum);
  if (wsp)
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((C + 3) / 4),
                       dim3(256), 0, stream.stream(), wsp,
                       mean.data_ptr<float>(), rstd.data_ptr<float>(), rm,
                       rv, N, C, HW, (float)eps, (float)momentum, nchunks);
  HIP_CHECK_KERNEL();
}

void batchnorm_norm(const at::Tensor& x, at::Tensor& y,
                    const at::Tensor& mean, const at::Tensor& rstd,
                    const c10::optional<at::Tensor>& gamma,
                    const c10::optional<at::Tensor>& beta) {
  const int C = (int)x.size(1);
  const int64_t HW = x.size(2) * x.size(3);
  const int64_t total = x.numel();
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(
      bn_norm_kernel, dim3(grid_for(total)), dim3(256), 0, stream.stream(),
      (const bf16_t*)x.data_ptr(), (bf16_t*)y.data_ptr(),
      mean.data_ptr<float>(), rstd.data_ptr<float>(), opt_ptr(gamma),
      opt_ptr(beta), C, HW, total);
  HIP_CHECK_KERNEL();
}

void batchnorm_bwd(const at::Tensor& x, const at::Tensor& dy, at::Tensor& dx,
                   const at::Tensor& mean, const at::Tensor& rstd,
                   const c10::optional<at::Tensor>& gamma, at::Tensor& sdy,
                   at::Tensor& sdyx) {
  const int N = (int)x.size(0), C = (int)x.size(1);
  const int64_t HW = x.size(2) * x.size(3);
  const int64_t total = x.numel();
  auto stream = at::cuda::getCurrentCUDAStream();
  const int nchunks = bn_nchunks(N, C);
  float* wsp = nullptr;
  at::Tensor wsp_t;
  if (nchunks > 1) {
    wsp_t = at::empty({nchunks, 2, C}, sdy.options());
    wsp = wsp_t.data_ptr<float>();
  }
  hipLaunchKernelGGL(bn_bwd_reduce_chunked_kernel, dim3(C, nchunks),
                     dim3(256), 0, stream.stream(),
                     (const bf16_t*)x.data_ptr(),
                     (const bf16_t*)dy.data_ptr(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), wsp, sdy.data_ptr<float>(),
                     sdyx.data_ptr<float>(), N, C, HW);
  if (wsp)
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 3) / 4),
                       dim3(256), 0, stream.stream(), wsp,
                       sdy.data_ptr<float>(), sdyx.data_ptr<float>(), C,
                       nchunks);
  HIP_CHECK_KERNEL();
  const float invM = 1.f / (float)((double)N * (double)HW);
  hipLaunchKernelGGL(
      bn_bwd_dx_kernel, dim3(grid_for(total)), dim3(256), 0, stream.stream(),
      (const bf16_t*)x.data_ptr(), (const bf16_t*)dy.data_ptr(),
      (bf16_t*)dx.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
      opt_ptr(gamma), sdy.data_ptr<float>(), sdyx.data_ptr<float>(), C, HW,
      total, invM);
  HIP_CHECK_KERNEL();
}
