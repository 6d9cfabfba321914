// Depthwise 2-D convolution (K9): the other half of the NASNet separable
// conv (reference nasnet_utils.py:182 _stacked_separable_conv = depthwise
// KxK then pointwise 1x1; the pointwise half runs on gemm_tr_batched).
// Depthwise conv has no reuse across channels, so it is bandwidth-bound
// elementwise work: one thread per output pixel, serial tap loop,
// coalesced along the contiguous W dimension. Works for any channel count
// (no GEMM alignment constraints), tap size and stride.
//
// Each of forward, dX and dW has three tiers, picked on the host from the
// shape alone (docs/KERNELS.md): LDS-staged (*_lds_kernel) while the images
// fit the LDS budget, register-tap (*_tmpl_kernel, dw_fused) for larger
// images, and a runtime-KS kernel for every other tap size or stride. The
// forward and dX tap loops are written once, below, and shared by all tiers.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <type_traits>
#include "common.h"

// ------------------------------------------------------- shared tap loops
// Tap weights come either from a register copy (float) or straight from
// memory (bf16_t).
__device__ __forceinline__ float tap2f(float v) { return v; }
__device__ __forceinline__ float tap2f(bf16_t v) { return bf2f(v); }

// Forward: sum over the KSxKS window whose top-left input pixel is
// (ih0, iw0) of image xi (LDS or global). KS = 0 takes the tap count at
// run time from ks_rt and leaves the loops rolled.
template <int KS, typename WT>
__device__ __forceinline__ float fwd_tap_sum(const WT* wt, const bf16_t* xi,
                                             int H, int W, int ih0, int iw0,
                                             int ks_rt = KS) {
  const int ks = KS ? KS : ks_rt;
  constexpr int UNROLL = KS ? KS : 1;  // full, or none for a runtime count
  float acc = 0.f;
#pragma unroll UNROLL
  for (int kh = 0; kh < ks; ++kh) {
    const int ih = ih0 + kh;
    if (ih < 0 || ih >= H) continue;
    // row pointer formed once per kh: written as xi[ih * W + iw] the
    // compiler rebuilt the row offset for every tap of the LDS kernels
    // (3 VALU per tap instead of 1; fwd_lds<5> measured 59.8 us vs 50.5)
    const bf16_t* xrow = xi + ih * W;
#pragma unroll UNROLL
    for (int kw = 0; kw < ks; ++kw) {
      const int iw = iw0 + kw;
      if (iw < 0 || iw >= W) continue;
      acc += tap2f(wt[kh * ks + kw]) * bf2f(xrow[iw]);
    }
  }
  return acc;
}

// dX at input pixel (ih, iw): full correlation with the flipped kernel over
// dy image di, honoring stride divisibility. KS = 0 / STRIDE = 0 take the
// value at run time.
template <int KS, int STRIDE, typename WT>
__device__ __forceinline__ float dx_tap_sum(const WT* wt, const bf16_t* di,
                                            int OH, int OW, int ih, int iw,
                                            int pad, int ks_rt = KS,
                                            int stride_rt = STRIDE) {
  const int ks = KS ? KS : ks_rt;
  const int st = STRIDE ? STRIDE : stride_rt;
  constexpr int UNROLL = KS ? KS : 1;
  float acc = 0.f;
#pragma unroll UNROLL
  for (int kh = 0; kh < ks; ++kh) {
    const int num_h = ih + pad - kh;
    if (num_h < 0 || (STRIDE != 1 && (num_h % st))) continue;
    const int oh = num_h / st;
    if (oh >= OH) continue;
#pragma unroll UNROLL
    for (int kw = 0; kw < ks; ++kw) {
      const int num_w = iw + pad - kw;
      if (num_w < 0 || (STRIDE != 1 && (num_w % st))) continue;
      const int ow = num_w / st;
      if (ow >= OW) continue;
      acc += tap2f(wt[kh * ks + kw]) * bf2f(di[oh * OW + ow]);
    }
  }
  return acc;
}

// Channel c's taps into registers (same c for the whole block -> broadcast
// from L1), so the tap loops run on fully unrolled register operands.
template <int KS>
__device__ __forceinline__ void load_taps(float (&wr)[KS * KS],
                                          const bf16_t* w, int c) {
#pragma unroll
  for (int i = 0; i < KS * KS; ++i) wr[i] = bf2f(w[c * KS * KS + i]);
}

// Block copy of one contiguous span of n pixels into LDS (256 threads), by
// uint4 when n is a multiple of 8 — image sizes are in practice.
__device__ __forceinline__ void stage_span(bf16_t* dst, const bf16_t* src,
                                           int n) {
  if ((n & 7) == 0) {
    for (int i = threadIdx.x; i < (n >> 3); i += 256)
      ((uint4*)dst)[i] = ((const uint4*)src)[i];
  } else {
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
  }
}

// ---------------------------------------------------------------- forward
// Runtime-KS kernel: any tap size, flat grid-stride loop over all outputs.
__global__ __launch_bounds__(256) void depthwise_fwd_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, int B, int C, int H, int W, int OH, int OW,
    int KS, int stride, int pad) {
  const int64_t total = (int64_t)B * C * OH * OW;
  const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += gstride) {
    const int ow = (int)(p % OW);
    const int oh = (int)((p / OW) % OH);
    const int c = (int)((p / ((int64_t)OW * OH)) % C);
    const int b = (int)(p / ((int64_t)OW * OH * C));
    const bf16_t* xp = x + ((int64_t)b * C + c) * H * W;
    y[p] = f2bf(fwd_tap_sum<0>(w + c * KS * KS, xp, H, W, oh * stride - pad,
                               ow * stride - pad, KS));
  }
}

// KS-templated register-tap kernel: one (batch, channel) image per
// blockIdx.y, so the taps load once into registers and the tap loops fully
// unroll.
template <int KS>
__global__ __launch_bounds__(256) void depthwise_fwd_tmpl_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, int C, int H, int W, int OH, int OW, int stride,
    int pad) {
  const int bc = blockIdx.y;
  const bf16_t* xp = x + (int64_t)bc * H * W;
  bf16_t* yp = y + (int64_t)bc * OH * OW;
  float wr[KS * KS];
  load_taps<KS>(wr, w, bc % C);
  const int total = OH * OW;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += gridDim.x * blockDim.x) {
    const int ow = p % OW, oh = p / OW;
    yp[p] = f2bf(fwd_tap_sum<KS>(wr, xp, H, W, oh * stride - pad,
                                 ow * stride - pad));
  }
}

// LDS-staged forward: the tap loop re-reads each input pixel KS^2 times;
// from L1 that measured ~25x off the bandwidth roofline (fwd<5> 141 us
// where x+y once is ~9 us, profiles/nasprof5_summary.txt). Stage a GROUP
// of P whole (b,c) images in LDS (images are contiguous in NCHW, so the
// group load is one coalesced span), then compute every output pixel
// from LDS. Weights stay in L1 (C*KS^2*2B is a few KB, fully resident).
template <int KS>
__global__ __launch_bounds__(256) void depthwise_fwd_lds_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, int C, int H, int W, int OH, int OW, int stride,
    int pad, int P, int BC) {
  __shared__ bf16_t xs[8192];  // 16 KB: P * H * W <= 8192 by host contract
  const int g0 = blockIdx.y * P;
  const int ni = min(P, BC - g0);
  stage_span(xs, x + (int64_t)g0 * H * W, ni * H * W);
  __syncthreads();
  const int opx = OH * OW;
  bf16_t* gy = y + (int64_t)g0 * opx;
  if (opx >= 256) {
    // image-outer: whole block works one image at a time so the KS^2 tap
    // weights live in registers (the flat loop re-read them from L1 per
    // pixel — measured slower than the old register-tap kernel).
    for (int img = 0; img < ni; ++img) {
      float wr[KS * KS];
      load_taps<KS>(wr, w, (g0 + img) % C);
      const bf16_t* xi = xs + img * H * W;
      bf16_t* yi = gy + (int64_t)img * opx;
      for (int p = threadIdx.x; p < opx; p += 256) {
        const int oh = p / OW, ow = p - (p / OW) * OW;
        yi[p] = f2bf(fwd_tap_sum<KS>(wr, xi, H, W, oh * stride - pad,
                                     ow * stride - pad));
      }
    }
    return;
  }
  // small images: flat loop over every output pixel of the group (weights
  // from L1 — C is large exactly when images are small).
  for (int p = threadIdx.x; p < ni * opx; p += 256) {
    const int img = p / opx;
    const int rem = p - img * opx;
    const int oh = rem / OW, ow = rem - (rem / OW) * OW;
    const int c = (g0 + img) % C;
    gy[p] = f2bf(fwd_tap_sum<KS>(w + c * KS * KS, xs + img * H * W, H, W,
                                 oh * stride - pad, ow * stride - pad));
  }
}

// --------------------------------------------------------------------- dX
// Runtime KS and stride, flat grid-stride loop. It measured 13.6% of the
// improve_nas step at 0.3 TB/s (branchy runtime tap loop, per-element
// weight reloads) before the templated kernels took the NASNet shapes.
__global__ __launch_bounds__(256) void depthwise_bwd_dx_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ dx, int B, int C, int H, int W, int OH, int OW,
    int KS, int stride, int pad) {
  const int64_t total = (int64_t)B * C * H * W;
  const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += gstride) {
    const int iw = (int)(p % W);
    const int ih = (int)((p / W) % H);
    const int c = (int)((p / ((int64_t)W * H)) % C);
    const int b = (int)(p / ((int64_t)W * H * C));
    const bf16_t* dyp = dy + ((int64_t)b * C + c) * OH * OW;
    dx[p] = f2bf(dx_tap_sum<0, 0>(w + c * KS * KS, dyp, OH, OW, ih, iw, pad,
                                  KS, stride));
  }
}

// Register-tap dX (KS, STRIDE compile-time): one (batch, channel) image
// per blockIdx.y, taps in registers, loops fully unrolled.
template <int KS, int STRIDE>
__global__ __launch_bounds__(256) void depthwise_bwd_dx_tmpl_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ dx, int C, int H, int W, int OH, int OW, int pad) {
  const int bc = blockIdx.y;
  const bf16_t* dyp = dy + (int64_t)bc * OH * OW;
  bf16_t* dxp = dx + (int64_t)bc * H * W;
  float wr[KS * KS];
  load_taps<KS>(wr, w, bc % C);
  const int total = H * W;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total;
       p += gridDim.x * blockDim.x) {
    dxp[p] = f2bf(dx_tap_sum<KS, STRIDE>(wr, dyp, OH, OW, p / W, p % W, pad));
  }
}

// LDS-staged dX: same grouping as the forward, dy staged in LDS.
template <int KS, int STRIDE>
__global__ __launch_bounds__(256) void depthwise_bwd_dx_lds_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ dx, int C, int H, int W, int OH, int OW, int pad,
    int P, int BC) {
  __shared__ bf16_t ds[8192];  // P * OH * OW <= 8192 by host contract
  const int g0 = blockIdx.y * P;
  const int ni = min(P, BC - g0);
  const int opx = OH * OW;
  stage_span(ds, dy + (int64_t)g0 * opx, ni * opx);
  __syncthreads();
  const int ipx = H * W;
  bf16_t* gdx = dx + (int64_t)g0 * ipx;
  if (ipx >= 256) {
    // image-outer: tap weights in registers for the whole image.
    for (int img = 0; img < ni; ++img) {
      float wr[KS * KS];
      load_taps<KS>(wr, w, (g0 + img) % C);
      const bf16_t* di = ds + img * opx;
      bf16_t* xo = gdx + (int64_t)img * ipx;
      for (int p = threadIdx.x; p < ipx; p += 256) {
        const int ih = p / W, iw = p - (p / W) * W;
        xo[p] = f2bf(dx_tap_sum<KS, STRIDE>(wr, di, OH, OW, ih, iw, pad));
      }
    }
    return;
  }
  // small images: flat loop, weights from L1 (as in the forward).
  for (int p = threadIdx.x; p < ni * ipx; p += 256) {
    const int img = p / ipx;
    const int rem = p - img * ipx;
    const int ih = rem / W, iw = rem - (rem / W) * W;
    const int c = (g0 + img) % C;
    gdx[p] = f2bf(dx_tap_sum<KS, STRIDE>(w + c * KS * KS, ds + img * opx, OH,
                                         OW, ih, iw, pad));
  }
}

// --------------------------------------------------------------------- dW
// LDS-staged dW: grid (C, nchunks); each block owns a span of images b for
// ONE channel, stages x[b,c] and dy[b,c] image groups in LDS, accumulates
// all KS^2 taps in registers from LDS, and writes its per-chunk partial
// into a workspace slot; depthwise_dw_reduce_kernel sums chunks in fixed
// order (deterministic — replaces the per-tap atomicAdd, whose fp32
// ordering varied run to run).
// This kernel keeps its hand-written staging and tap loop: built on the
// shared staging and tap helpers it kept its registers, occupancy and
// instruction mix but measured 4-9% slower, twice (256x32x32x32 5x5: 88.5 us
// against 81.0; BENCHMARKS.md). Only its final block sum is the shared one.
template <int KS>
__global__ __launch_bounds__(256) void depthwise_bwd_dw_lds_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
    float* __restrict__ wsp, int B, int C, int H, int W, int OH, int OW,
    int stride, int pad, int b_per_chunk, int G) {
  __shared__ bf16_t xs[4096];  // G * H * W <= 4096 by host contract
  __shared__ bf16_t ds[4096];  // G * OH * OW <= 4096
  const int c = blockIdx.x;
  const int b0 = blockIdx.y * b_per_chunk;
  const int b1 = min(B, b0 + b_per_chunk);
  const int ipx = H * W, opx = OH * OW;
  float acc[KS * KS];
#pragma unroll
  for (int t = 0; t < KS * KS; ++t) acc[t] = 0.f;
  for (int g = b0; g < b1; g += G) {
    const int ni = min(G, b1 - g);
    if ((ipx & 7) == 0) {
      for (int i = threadIdx.x; i < ((ni * ipx) >> 3); i += 256) {
        const int img = i / (ipx >> 3);
        ((uint4*)xs)[i] = ((const uint4*)(
            x + ((int64_t)(g + img) * C + c) * ipx))[i - img * (ipx >> 3)];
      }
    } else {
      for (int i = threadIdx.x; i < ni * ipx; i += 256) {
        const int img = i / ipx;
        xs[i] = x[((int64_t)(g + img) * C + c) * ipx + (i - img * ipx)];
      }
    }
    if ((opx & 7) == 0) {
      for (int i = threadIdx.x; i < ((ni * opx) >> 3); i += 256) {
        const int img = i / (opx >> 3);
        ((uint4*)ds)[i] = ((const uint4*)(
            dy + ((int64_t)(g + img) * C + c) * opx))[i - img * (opx >> 3)];
      }
    } else {
      for (int i = threadIdx.x; i < ni * opx; i += 256) {
        const int img = i / opx;
        ds[i] = dy[((int64_t)(g + img) * C + c) * opx + (i - img * opx)];
      }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < ni * opx; p += 256) {
      const int img = p / opx;
      const int rem = p - img * opx;
      const int oh = rem / OW, ow = rem - (rem / OW) * OW;
      const float dyv = bf2f(ds[p]);
      const bf16_t* xi = xs + img * ipx;
      const int ih0 = oh * stride - pad, iw0 = ow * stride - pad;
#pragma unroll
      for (int kh = 0; kh < KS; ++kh) {
        const int ih = ih0 + kh;
        if (ih < 0 || ih >= H) continue;
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
          const int iw = iw0 + kw;
          if (iw < 0 || iw >= W) continue;
          acc[kh * KS + kw] += dyv * bf2f(xi[ih * W + iw]);
        }
      }
    }
    __syncthreads();
  }
  float* slot = wsp + ((int64_t)blockIdx.y * C + c) * (KS * KS);
  block_reduce_sum(acc, [&](int t, float v) { slot[t] = v; });
}

// dw[c*KSQ+t] = sum over chunks of wsp[(chunk*C + c)*KSQ + t], fixed order.
__global__ __launch_bounds__(256) void depthwise_dw_reduce_kernel(
    const float* __restrict__ wsp, float* __restrict__ dw, int C, int KSQ,
    int nchunks) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * KSQ) return;
  float s = 0.f;
  for (int r = 0; r < nchunks; ++r) s += wsp[(int64_t)r * C * KSQ + i];
  dw[i] = s;
}

// Single-pass dW for images too large for LDS: each thread reads dy ONCE
// per output point and accumulates all KS*KS taps in registers
// (neighboring x reads hit L2), instead of the KS^2 full re-reads of the
// tap-per-block kernel (measured 14.5% of the improve_nas step at
// 0.7 TB/s, profiles/nasprof_summary.txt). grid = (C, chunks); one
// atomicAdd per (block, tap) onto a zeroed dw, so with more than one chunk
// the fp32 sum order, and the last bits of dw, vary run to run.
template <int KS>
__global__ __launch_bounds__(256) void depthwise_bwd_dw_fused_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
    float* __restrict__ dw, int B, int C, int H, int W, int OH, int OW,
    int stride, int pad, int64_t chunk) {
  const int c = blockIdx.x;
  const int64_t total = (int64_t)B * OH * OW;
  const int64_t start = (int64_t)blockIdx.y * chunk;
  const int64_t end = min(total, start + chunk);
  float acc[KS * KS] = {};
  for (int64_t p = start + threadIdx.x; p < end; p += blockDim.x) {
    const int ow = (int)(p % OW);
    const int oh = (int)((p / OW) % OH);
    const int b = (int)(p / ((int64_t)OW * OH));
    const float dyv =
        bf2f(dy[((int64_t)b * C + c) * OH * OW + oh * OW + ow]);
    const bf16_t* xp = x + ((int64_t)b * C + c) * H * W;
    const int ih0 = oh * stride - pad, iw0 = ow * stride - pad;
#pragma unroll
    for (int kh = 0; kh < KS; ++kh) {
      const int ih = ih0 + kh;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const int iw = iw0 + kw;
        if (iw < 0 || iw >= W) continue;
        acc[kh * KS + kw] += dyv * bf2f(xp[ih * W + iw]);
      }
    }
  }
  block_reduce_sum(
      acc, [&](int t, float v) { atomicAdd(&dw[c * KS * KS + t], v); });
}

// Runtime-KS dW: one block per (channel, tap); block-parallel reduction
// over b,oh,ow. Re-reads x and dy once per tap.
__global__ __launch_bounds__(256) void depthwise_bwd_dw_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
    float* __restrict__ dw, int B, int C, int H, int W, int OH, int OW,
    int KS, int stride, int pad) {
  const int c = blockIdx.x;
  const int kh = blockIdx.y / KS, kw = blockIdx.y % KS;
  const int64_t total = (int64_t)B * OH * OW;
  float acc[1] = {0.f};
  for (int64_t p = threadIdx.x; p < total; p += blockDim.x) {
    const int ow = (int)(p % OW);
    const int oh = (int)((p / OW) % OH);
    const int b = (int)(p / ((int64_t)OW * OH));
    const int ih = oh * stride + kh - pad;
    const int iw = ow * stride + kw - pad;
    if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
    acc[0] += bf2f(dy[((int64_t)b * C + c) * OH * OW + oh * OW + ow]) *
              bf2f(x[((int64_t)b * C + c) * H * W + ih * W + iw]);
  }
  block_reduce_sum(
      acc, [&](int, float v) { dw[c * KS * KS + kh * KS + kw] = v; });
}

// ------------------------------------------------------------------- host
namespace {

struct DwShape {
  int B, C, H, W, OH, OW, KS;
};

void check_bf16(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == at::kBFloat16,
              "depthwise: ", name, " must be a contiguous bf16 CUDA tensor");
}

// Shared argument check: x-like [B,C,H,W] and y-like [B,C,OH,OW] bf16
// images whose spatial sizes agree under (KS, stride, pad). The kernels
// index raw pointers from these sizes, so a mismatch would read or write
// out of bounds.
DwShape check_images(const at::Tensor& x, const char* xname,
                     const at::Tensor& y, const char* yname, int64_t taps,
                     int64_t stride, int64_t pad) {
  check_bf16(x, xname);
  check_bf16(y, yname);
  TORCH_CHECK(x.dim() == 4 && y.dim() == 4 && x.size(0) == y.size(0) &&
                  x.size(1) == y.size(1),
              "depthwise: ", xname, " and ", yname,
              " must be [B,C,H,W] with equal B and C");
  TORCH_CHECK(x.numel() > 0 && y.numel() > 0, "depthwise: empty ", xname,
              " or ", yname);
  const int64_t C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t KS = std::llround(std::sqrt((double)(taps / C)));
  TORCH_CHECK(KS >= 1 && taps == C * KS * KS,
              "depthwise: weight numel must be C*KS*KS, got ", taps,
              " for C=", C);
  TORCH_CHECK(stride >= 1 && pad >= 0, "depthwise: bad stride or pad");
  TORCH_CHECK(H + 2 * pad >= KS && W + 2 * pad >= KS &&
                  y.size(2) == (H + 2 * pad - KS) / stride + 1 &&
                  y.size(3) == (W + 2 * pad - KS) / stride + 1,
              "depthwise: ", yname, " spatial size ", y.size(2), "x",
              y.size(3), " does not match ", xname, " ", H, "x", W,
              " with KS=", KS, " stride=", stride, " pad=", pad);
  return {(int)x.size(0), (int)C,         (int)H, (int)W,
          (int)y.size(2), (int)y.size(3), (int)KS};
}

// Calls f(std::integral_constant<int, v>) for the v among Vs that equals
// the runtime value: turns KS or stride into a template argument.
template <int... Vs, typename F>
void with_const(int value, F&& f) {
  const bool found =
      ((value == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) ||
       ...);
  TORCH_CHECK(found, "depthwise: no kernel instance for ", value);
}

bool tmpl_ks(int KS) { return KS == 3 || KS == 5 || KS == 7; }

int dw_grid(int64_t n) {
  return (int)std::min<int64_t>((n + 255) / 256, 4096);
}

// Images per block for the LDS fwd/dX kernels: bounded by LDS (8192 staged
// pixels) AND by output work per block (keep blocks small enough that
// ceil(BC/P) fills the chip).
int lds_group(int staged_px, int out_px) {
  return std::max(1, std::min(8192 / staged_px, std::max(1, 4096 / out_px)));
}

// grid.x of the *_tmpl kernels: split an image over blocks only while
// B*C alone does not fill the chip.
int tmpl_px_blocks(int out_px, int64_t bc) {
  return std::max(1, std::min((out_px + 255) / 256, (int)(2048 / bc) + 1));
}

}  // namespace

void depthwise_fwd(const at::Tensor& x, const at::Tensor& w, at::Tensor& y,
                   int64_t stride, int64_t pad) {
  check_bf16(w, "w");
  const DwShape s = check_images(x, "x", y, "y", w.numel(), stride, pad);
  const bf16_t* xp = (const bf16_t*)x.data_ptr();
  const bf16_t* wp = (const bf16_t*)w.data_ptr();
  bf16_t* yp = (bf16_t*)y.data_ptr();
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const int64_t bc = (int64_t)s.B * s.C;
  if (tmpl_ks(s.KS) && s.H * s.W <= 8192) {
    const int P = lds_group(s.H * s.W, s.OH * s.OW);
    const int groups = (int)((bc + P - 1) / P);
    with_const<3, 5, 7>(s.KS, [&](auto ks) {
      constexpr int K = decltype(ks)::value;
      hipLaunchKernelGGL(depthwise_fwd_lds_kernel<K>,
                         dim3(1, (unsigned)groups), dim3(256), 0, stream, xp,
                         wp, yp, s.C, s.H, s.W, s.OH, s.OW, (int)stride,
                         (int)pad, P, (int)bc);
    });
  } else if ((s.KS == 3 || s.KS == 5) && bc <= 65535) {
    // no <7> instance: 7x7 taps on images this large take the runtime kernel
    const int px_blocks = tmpl_px_blocks(s.OH * s.OW, bc);
    with_const<3, 5>(s.KS, [&](auto ks) {
      constexpr int K = decltype(ks)::value;
      hipLaunchKernelGGL(depthwise_fwd_tmpl_kernel<K>,
                         dim3((unsigned)px_blocks, (unsigned)bc), dim3(256), 0,
                         stream, xp, wp, yp, s.C, s.H, s.W, s.OH, s.OW,
                         (int)stride, (int)pad);
    });
  } else {
    hipLaunchKernelGGL(depthwise_fwd_kernel,
                       dim3(dw_grid(bc * s.OH * s.OW)), dim3(256), 0, stream,
                       xp, wp, yp, s.B, s.C, s.H, s.W, s.OH, s.OW, s.KS,
                       (int)stride, (int)pad);
  }
  HIP_CHECK_KERNEL();
}

void depthwise_bwd_dx(const at::Tensor& dy, const at::Tensor& w,
                      at::Tensor& dx, int64_t stride, int64_t pad) {
  check_bf16(w, "w");
  const DwShape s = check_images(dx, "dx", dy, "dy", w.numel(), stride, pad);
  const bf16_t* dyp = (const bf16_t*)dy.data_ptr();
  const bf16_t* wp = (const bf16_t*)w.data_ptr();
  bf16_t* dxp = (bf16_t*)dx.data_ptr();
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const int64_t bc = (int64_t)s.B * s.C;
  const bool tmpl = tmpl_ks(s.KS) && (stride == 1 || stride == 2);
  if (tmpl && s.OH * s.OW <= 8192) {
    const int P = lds_group(s.OH * s.OW, s.H * s.W);
    const int groups = (int)((bc + P - 1) / P);
    with_const<3, 5, 7>(s.KS, [&](auto ks) {
      with_const<1, 2>((int)stride, [&](auto st) {
        constexpr int K = decltype(ks)::value, S = decltype(st)::value;
        hipLaunchKernelGGL((depthwise_bwd_dx_lds_kernel<K, S>),
                           dim3(1, (unsigned)groups), dim3(256), 0, stream,
                           dyp, wp, dxp, s.C, s.H, s.W, s.OH, s.OW, (int)pad,
                           P, (int)bc);
      });
    });
  } else if (tmpl && bc <= 65535) {
    const int px_blocks = tmpl_px_blocks(s.H * s.W, bc);
    with_const<3, 5, 7>(s.KS, [&](auto ks) {
      with_const<1, 2>((int)stride, [&](auto st) {
        constexpr int K = decltype(ks)::value, S = decltype(st)::value;
        hipLaunchKernelGGL((depthwise_bwd_dx_tmpl_kernel<K, S>),
                           dim3((unsigned)px_blocks, (unsigned)bc), dim3(256),
                           0, stream, dyp, wp, dxp, s.C, s.H, s.W, s.OH, s.OW,
                           (int)pad);
      });
    });
  } else {
    hipLaunchKernelGGL(depthwise_bwd_dx_kernel,
                       dim3(dw_grid(bc * s.H * s.W)), dim3(256), 0, stream,
                       dyp, wp, dxp, s.B, s.C, s.H, s.W, s.OH, s.OW, s.KS,
                       (int)stride, (int)pad);
  }
  HIP_CHECK_KERNEL();
}

void depthwise_bwd_dw(const at::Tensor& x, const at::Tensor& dy,
                      at::Tensor& dw, int64_t stride, int64_t pad) {
  TORCH_CHECK(dw.is_cuda() && dw.is_contiguous() &&
                  dw.scalar_type() == at::kFloat,
              "depthwise dW: dw must be a contiguous fp32 CUDA tensor");
  const DwShape s = check_images(x, "x", dy, "dy", dw.numel(), stride, pad);
  const bf16_t* xp = (const bf16_t*)x.data_ptr();
  const bf16_t* dyp = (const bf16_t*)dy.data_ptr();
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const int64_t total = (int64_t)s.B * s.OH * s.OW;
  if (tmpl_ks(s.KS) && s.H * s.W <= 4096 && s.OH * s.OW <= 4096) {
    // LDS-staged deterministic path: per-chunk workspace + ordered reduce.
    const int nchunks =
        (int)std::max<int64_t>(1, std::min<int64_t>(1024 / s.C, s.B));
    const int b_per_chunk = (s.B + nchunks - 1) / nchunks;
    const int G = std::max(
        1, std::min({4096 / (s.H * s.W), 4096 / (s.OH * s.OW), s.B}));
    auto wsp = at::empty({nchunks, s.C, s.KS * s.KS}, dw.options());
    with_const<3, 5, 7>(s.KS, [&](auto ks) {
      constexpr int K = decltype(ks)::value;
      hipLaunchKernelGGL(depthwise_bwd_dw_lds_kernel<K>,
                         dim3((unsigned)s.C, (unsigned)nchunks), dim3(256), 0,
                         stream, xp, dyp, wsp.data_ptr<float>(), s.B, s.C, s.H,
                         s.W, s.OH, s.OW, (int)stride, (int)pad, b_per_chunk,
                         G);
    });
    hipLaunchKernelGGL(depthwise_dw_reduce_kernel,
                       dim3((unsigned)((s.C * s.KS * s.KS + 255) / 256)),
                       dim3(256), 0, stream, wsp.data_ptr<float>(),
                       dw.data_ptr<float>(), s.C, s.KS * s.KS, nchunks);
  } else if (tmpl_ks(s.KS)) {
    // single-pass register-tap kernel; it accumulates onto dw atomically
    const int nchunks =
        (int)std::max<int64_t>(1, std::min<int64_t>(1024 / s.C, 64));
    const int64_t chunk = (total + nchunks - 1) / nchunks;
    dw.zero_();
    with_const<3, 5, 7>(s.KS, [&](auto ks) {
      constexpr int K = decltype(ks)::value;
      hipLaunchKernelGGL(depthwise_bwd_dw_fused_kernel<K>,
                         dim3((unsigned)s.C, (unsigned)nchunks), dim3(256), 0,
                         stream, xp, dyp, dw.data_ptr<float>(), s.B, s.C, s.H,
                         s.W, s.OH, s.OW, (int)stride, (int)pad, chunk);
    });
  } else {
    hipLaunchKernelGGL(depthwise_bwd_dw_kernel,
                       dim3((unsigned)s.C, (unsigned)(s.KS * s.KS)), dim3(256),
                       0, stream, xp, dyp, dw.data_ptr<float>(), s.B, s.C, s.H,
                       s.W, s.OH, s.OW, s.KS, (int)stride, (int)pad);
  }
  HIP_CHECK_KERNEL();
}
