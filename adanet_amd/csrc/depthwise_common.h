// Tap loops, staging and argument checks shared by the depthwise kernels
// (depthwise.hip) and the ReLU-fused ones (relu_depthwise.hip,
// relu_depthwise_strip.hip).
#pragma once

#include <torch/extension.h>
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

// Block barrier of the ReLU-fused files (relu_depthwise.hip,
// relu_depthwise_strip.hip): they are built without some target features,
// and the runtime header's __syncthreads is not inlined into such code.
__device__ __forceinline__ void rd_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Zero each bf16 lane of a 32-bit word whose sign bit is set (-0 included).
__device__ __forceinline__ uint32_t relu_bf16x2(uint32_t v) {
  const uint32_t neg = (v >> 15) & 0x00010001u;  // 1 per negative lane
  return v & ~(neg * 0xffffu);
}

__device__ __forceinline__ uint4 relu_bf16x8(uint4 v) {
  v.x = relu_bf16x2(v.x);
  v.y = relu_bf16x2(v.y);
  v.z = relu_bf16x2(v.z);
  v.w = relu_bf16x2(v.w);
  return v;
}

__device__ __forceinline__ bf16_t relu_bf16(bf16_t v) {
  return bf2f(v) > 0.f ? v : f2bf(0.f);
}

// Channel c's planes of images g .. g+ni-1 (px pixels each, C * px apart in
// memory) into a dense LDS array, clamped in flight if RELU; by uint4 when
// px is a multiple of 8.
template <bool RELU>
__device__ __forceinline__ void stage_planes(bf16_t* dst, const bf16_t* src,
                                             int g, int ni, int C, int c,
                                             int px) {
  if ((px & 7) == 0) {
    const int v = px >> 3;
    for (int i = threadIdx.x; i < ni * v; i += 256) {
      const int img = i / v;
      uint4 q = ((const uint4*)(
          src + ((int64_t)(g + img) * C + c) * px))[i - img * v];
      if (RELU) q = relu_bf16x8(q);
      ((uint4*)dst)[i] = q;
    }
  } else {
    for (int i = threadIdx.x; i < ni * px; i += 256) {
      const int img = i / px;
      const bf16_t q = src[((int64_t)(g + img) * C + c) * px + (i - img * px)];
      dst[i] = RELU ? relu_bf16(q) : q;
    }
  }
}

// dw[c*KSQ+t] = sum over chunks of wsp[(chunk*C + c)*KSQ + t], in fixed
// order, on `stream` (depthwise_dw_reduce_kernel; defined in depthwise.hip
// so the kernel has one code object).
void launch_depthwise_dw_reduce(const float* wsp, float* dw, int C, int KSQ,
                                int nchunks, hipStream_t stream);

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

}  // namespace
