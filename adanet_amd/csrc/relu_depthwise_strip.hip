// Strip-tiled ReLU -> depthwise for the large planes of a training-mode
// SepConv half, where the one-thread-per-pixel kernels are bound by LDS
// issue and address arithmetic (one 2-byte LDS read per tap operand):
//   relu_depthwise_strip_fwd     y  = depthwise(relu(x))
//   relu_depthwise_strip_bwd_dx  dx = (x > 0) ? dX(dy) : +0
//   relu_depthwise_strip_bwd_dw  dw = dW(relu(x), dy), the bits of
//                                relu_depthwise_bwd's dW (see the kernel)
//
// A 256-thread block stages a group of whole planes into LDS by 16-byte
// chunks (x clamped in flight; dy as it is). A thread owns a strip: 8
// consecutive outputs of one row, one 16-byte store, times R = 2 vertically
// adjacent rows. Per source row it reads the window the strip needs as whole
// chunks (its own and the neighbours), converts it to fp32 registers once and
// feeds it to every accumulator that uses the row, the channel's taps in
// registers: a 5x5 strip at stride 1 issues 3 LDS reads per source row where
// the per-pixel kernels issue 40, and R rows share K + R - 1 source rows.
//
// Each output is one fp32 accumulator that starts at +0 and takes its taps
// in the order of fwd_tap_sum / dx_tap_sum (kh ascending, kw ascending
// inside), the multiply-add in their source form, so the results equal the
// chain's bit for bit. Rows outside the plane are skipped as there; columns
// outside it meet a zero in the window, which leaves the accumulator's bits
// alone (finite taps: +0 plus +-0 is +0).

#include <ATen/cuda/CUDAContext.h>
#include "depthwise_common.h"

// As relu_depthwise.hip: no packed-fp32 forms in any function of this file.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {
constexpr int STRIP_LDS = 8192;  // staged pixels per block (16 KB)
// Rows per strip. Measured 2 against 4 (BENCHMARKS.md): 4 shares more source
// rows but halves the strips per plane, and lost by 15 to 25 % on 16x16
// planes and at stride 2; on 32x32 it won the forward by 2 %.
constexpr int STRIP_ROWS = 2;
// Outputs per strip of the dW kernel, whose lanes are 256 / S strips times K
// tap rows: 4 is the narrowest that fits 256 lanes at K = 3 (192 lanes), 8
// at K = 5 (160) and K = 7 (224); OW % 16 != 0 in the class rules out 16.
// At K = 3, 8 (96 lanes) measured 18 to 21 % slower than 4 (BENCHMARKS.md).
constexpr int strip_dw_width(int ks) { return ks == 3 ? 4 : 8; }
}

__device__ __forceinline__ float bf_lo(uint32_t v) {
  return __uint_as_float(v << 16);
}
__device__ __forceinline__ float bf_hi(uint32_t v) {
  return __uint_as_float(v & 0xffff0000u);
}
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  return (uint32_t)__bfloat16_as_ushort(f2bf(a)) |
         ((uint32_t)__bfloat16_as_ushort(f2bf(b)) << 16);
}

// N units of U pixels (U = 8: 16-byte reads, U = 4: 8-byte reads) of LDS row
// `row`, from unit u0 on, as fp32; units outside [0, nu) read as zero.
template <int U, int N>
__device__ __forceinline__ void load_window(float (&win)[U * N],
                                            const bf16_t* row, int u0,
                                            int nu) {
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const int u = u0 + q;
    const bool in = u >= 0 && u < nu;
    if constexpr (U == 8) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (in) v = ((const uint4*)row)[u];
      win[8 * q + 0] = bf_lo(v.x), win[8 * q + 1] = bf_hi(v.x);
      win[8 * q + 2] = bf_lo(v.y), win[8 * q + 3] = bf_hi(v.y);
      win[8 * q + 4] = bf_lo(v.z), win[8 * q + 5] = bf_hi(v.z);
      win[8 * q + 6] = bf_lo(v.w), win[8 * q + 7] = bf_hi(v.w);
    } else {
      uint2 v = make_uint2(0, 0);
      if (in) v = ((const uint2*)row)[u];
      win[4 * q + 0] = bf_lo(v.x), win[4 * q + 1] = bf_hi(v.x);
      win[4 * q + 2] = bf_lo(v.y), win[4 * q + 3] = bf_hi(v.y);
    }
  }
}

// Strip s of the group: plane img, first row r0 (a multiple of R), chunk c.
struct Strip {
  int img, r0, c;
};
template <int R>
__device__ __forceinline__ Strip strip_of(int s, int spp, int wc) {
  const int img = s / spp, rem = s - img * spp;
  const int rg = rem / wc;
  return {img, rg * R, rem - rg * wc};
}

// ---------------------------------------------------------------- forward
// Group of P whole (b,c) planes of x, one contiguous span, clamped into LDS.
// A strip's source rows run upwards, ih = r0 * STRIDE - pad + t; row t is
// tap row kh = t - r * STRIDE of the strip's output row r. The window starts
// one chunk left of the strip's first input chunk: output i, tap kw reads
// window element 8 + STRIDE * i - pad + kw.
template <int KS, int STRIDE, int R>
__global__ __launch_bounds__(256) void relu_depthwise_strip_fwd_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ y, int C, int H, int W, int OH, int OW, int P,
    int BC) {
  __shared__ __align__(16) bf16_t xs[STRIP_LDS];  // P * H * W (host)
  constexpr int PAD = KS / 2;
  constexpr int NCH = STRIDE == 1 || KS == 3 ? 3 : 4;
  constexpr int NROWS = (R - 1) * STRIDE + KS;
  const int g0 = blockIdx.x * P;
  const int ni = min(P, BC - g0);
  const int ipx = H * W;
  const uint4* gx = (const uint4*)(x + (int64_t)g0 * ipx);
  for (int i = threadIdx.x; i < (ni * ipx) >> 3; i += 256)
    ((uint4*)xs)[i] = relu_bf16x8(gx[i]);
  rd_sync();
  const int wc = OW >> 3;
  const int spp = ((OH + R - 1) / R) * wc;
  for (int s = threadIdx.x; s < ni * spp; s += 256) {
    const Strip st = strip_of<R>(s, spp, wc);
    float wr[KS * KS];
    load_taps<KS>(wr, w, (g0 + st.img) % C);
    const bf16_t* xi = xs + st.img * ipx;
    float acc[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
#pragma unroll
    for (int t = 0; t < NROWS; ++t) {
      const int ih = st.r0 * STRIDE - PAD + t;
      if (ih < 0 || ih >= H) continue;
      float win[8 * NCH];
      load_window<8, NCH>(win, xi + ih * W, STRIDE * st.c - 1, W >> 3);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int kh = t - r * STRIDE;
        if (kh < 0 || kh >= KS) continue;
#pragma unroll
        for (int kw = 0; kw < KS; ++kw)
#pragma unroll
          for (int i = 0; i < 8; ++i)
            acc[r][i] += wr[kh * KS + kw] * win[8 + STRIDE * i - PAD + kw];
      }
    }
    bf16_t* yo = y + ((int64_t)(g0 + st.img) * OH + st.r0) * OW + 8 * st.c;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (st.r0 + r < OH)
        *(uint4*)(yo + r * OW) = make_uint4(
            pack_bf16x2(acc[r][0], acc[r][1]), pack_bf16x2(acc[r][2], acc[r][3]),
            pack_bf16x2(acc[r][4], acc[r][5]), pack_bf16x2(acc[r][6], acc[r][7]));
  }
}

// --------------------------------------------------------------------- dX
// Group of P whole (b,c) planes of dy in LDS; a strip is 8 pixels of dx row
// ih = r0 + r. dy rows run downwards so that kh ascends, and inside a row
// the taps run kw ascending, that is dy columns right to left.
//   stride 1  dy row r0 + u is tap row kh = r + pad - u; tap kw of pixel i
//             is window element 8 + i + pad - kw of the three chunks from
//             c - 1 on.
//   stride 2  r0 is even (R is), so parity is known at compile time: dy row
//             r0 / 2 + u is tap row kh = r + pad - 2u, and pixel i takes tap
//             kw only where i + pad - kw is even, from dy column
//             4c + (i + pad - kw) / 2: element 4 + that of three 8-byte
//             units from 4c - 4 on.
// The mask is x at the strip's own offset, one 16-byte global load per row;
// every dx element of the plane is stored exactly once.
template <int KS, int STRIDE, int R>
__global__ __launch_bounds__(256) void relu_depthwise_strip_dx_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
    const bf16_t* __restrict__ w, bf16_t* __restrict__ dx, int C, int H,
    int W, int OH, int OW, int P, int BC) {
  static_assert(STRIDE == 1 || R % 2 == 0, "stride 2 needs even r0");
  __shared__ __align__(16) bf16_t ds[STRIP_LDS];  // P * OH * OW (host)
  constexpr int PAD = KS / 2;
  // dy rows relative to r0 / STRIDE: from UMAX down to UMIN
  constexpr int UMAX = (R - 1 + PAD) / STRIDE;
  constexpr int UMIN = -(PAD / STRIDE);
  constexpr int U = STRIDE == 1 ? 8 : 4;
  const int g0 = blockIdx.x * P;
  const int ni = min(P, BC - g0);
  const int opx = OH * OW;
  const uint4* gd = (const uint4*)(dy + (int64_t)g0 * opx);
  for (int i = threadIdx.x; i < (ni * opx) >> 3; i += 256)
    ((uint4*)ds)[i] = gd[i];
  rd_sync();
  const int wc = W >> 3;
  const int spp = ((H + R - 1) / R) * wc;
  for (int s = threadIdx.x; s < ni * spp; s += 256) {
    const Strip st = strip_of<R>(s, spp, wc);
    float wr[KS * KS];
    load_taps<KS>(wr, w, (g0 + st.img) % C);
    const int64_t off = ((int64_t)(g0 + st.img) * H + st.r0) * W + 8 * st.c;
    uint4 xm[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (st.r0 + r < H) xm[r] = *(const uint4*)(x + off + r * W);
    const bf16_t* di = ds + st.img * opx;
    float acc[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
#pragma unroll
    for (int u = UMAX; u >= UMIN; --u) {
      const int oh = st.r0 / STRIDE + u;
      if (oh < 0 || oh >= OH) continue;
      float win[U * 3];
      load_window<U, 3>(win, di + oh * OW, st.c - 1, OW / U);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int kh = r + PAD - STRIDE * u;
        if (kh < 0 || kh >= KS) continue;
#pragma unroll
        for (int kw = 0; kw < KS; ++kw)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int num = i + PAD - kw;
            if (STRIDE == 2 && (num & 1)) continue;
            acc[r][i] += wr[kh * KS + kw] * win[U + num / STRIDE];
          }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (st.r0 + r >= H) continue;
      const uint32_t m[4] = {xm[r].x, xm[r].y, xm[r].z, xm[r].w};
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = pack_bf16x2(bf_lo(m[j]) > 0.f ? acc[r][2 * j] : 0.f,
                           bf_hi(m[j]) > 0.f ? acc[r][2 * j + 1] : 0.f);
      *(uint4*)(dx + off + r * W) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

// --------------------------------------------------------------------- dW
// The dW phase of relu_depthwise_bwd_kernel, re-tiled without changing a bit.
// Partition, staging, slot and block sum are that kernel's: grid (C, nchunks),
// a block owns channel c and the images [b0, b1) of its chunk in groups of G,
// stages the clamped x planes and the dy planes of a group, and sums 256
// per-thread values per tap with block_reduce_sum into workspace slot
// (chunk, c). There thread v adds, per tap, the products of the group's
// outputs p = v, v + 256, ... in that order, groups ascending. Here those
// 256 threads are virtual: a lane is (strip j, tap row kh) and owns the tap
// row's KS sums of the S adjacent virtual threads S*j .. S*j + S - 1. In pass
// k these are the outputs p = S*j + i + 256*k, S consecutive ow of one output
// row (S divides OW and 256), so the lane reads the dy strip in one LDS read
// and the x row ih = oh * STRIDE - pad + kh as whole units of S pixels, one
// unit left of the strip's first input pixel: output i, tap kw is window
// element S + STRIDE * i - pad + kw. Every (virtual thread, tap) sum sees its
// terms in the order above; a column outside the plane, which that kernel
// skips, meets a zero here, and adding +-0 to a sum that started at +0
// leaves its bits alone (finite inputs). A row outside the plane is skipped
// as there. At the end the sums go through LDS to thread v = virtual thread
// v, 16 taps per round over the staging array, and into the same
// block_reduce_sum on the same lane layout.
template <int KS, int STRIDE, int S>
__global__ __launch_bounds__(256) void relu_depthwise_strip_dw_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
    float* __restrict__ wsp, int B, int C, int H, int W, int OH, int OW,
    int b_per_chunk, int G) {
  constexpr int PAD = KS / 2, KSQ = KS * KS;
  constexpr int NS = 256 / S;  // strips per pass
  constexpr int NU = (S + STRIDE * (S - 1) - PAD + KS - 1) / S + 1;
  constexpr int RT = STRIP_LDS * 2 / (256 * 4);  // taps per hand-over round
  static_assert((S == 4 || S == 8) && NS * KS <= 256 && S >= PAD, "lanes");
  // G * H * W <= 4096 and G * OH * OW <= 4096 (host)
  __shared__ __align__(16) bf16_t lds[STRIP_LDS];
  bf16_t* xs = lds;
  bf16_t* ds = lds + STRIP_LDS / 2;
  const int c = blockIdx.x;
  const int b0 = blockIdx.y * b_per_chunk;
  const int b1 = min(B, b0 + b_per_chunk);
  const int ipx = H * W, opx = OH * OW;
  const int kh = threadIdx.x / NS, j = threadIdx.x - kh * NS;
  const bool lane = kh < KS;  // the rest only stages
  // (img, oh, ow) of the strip's first output S*j, and of a step of 256
  // outputs: three digits that advance with one carry each, no division
  // per pass
  const int img0 = S * j / opx, rem0 = S * j - img0 * opx;
  const int oh0 = rem0 / OW, ow0 = rem0 - oh0 * OW;
  const int dimg = 256 / opx, drem = 256 - dimg * opx;
  const int doh = drem / OW, dow = drem - doh * OW;
  float acc[S][KS];
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int kw = 0; kw < KS; ++kw) acc[i][kw] = 0.f;
  for (int g = b0; g < b1; g += G) {
    const int ni = min(G, b1 - g);
    stage_planes<true>(xs, x, g, ni, C, c, ipx);
    stage_planes<false>(ds, dy, g, ni, C, c, opx);
    rd_sync();
    if (lane) {
      int img = img0, oh = oh0, ow = ow0;
      // S divides opx, so a strip is inside the group or outside it
      for (int p = S * j; p < ni * opx; p += 256) {
        const int ih = oh * STRIDE - PAD + kh;
        if (ih >= 0 && ih < H) {
          float d[S], win[S * NU];
          load_window<S, 1>(d, ds, p / S, STRIP_LDS / 2 / S);
          load_window<S, NU>(win, xs + img * ipx + ih * W,
                             STRIDE * (ow / S) - 1, W / S);
#pragma unroll
          for (int i = 0; i < S; ++i)
#pragma unroll
            for (int kw = 0; kw < KS; ++kw)
              acc[i][kw] += d[i] * win[S + STRIDE * i - PAD + kw];
        }
        ow += dow;
        if (ow >= OW) ow -= OW, ++oh;
        oh += doh;
        if (oh >= OH) oh -= OH, ++img;
        img += dimg;
      }
    }
    rd_sync();
  }
  // hand-over: red[tap of the round][virtual thread] over the staging array
  // (the group loop ended on a barrier)
  float* red = (float*)lds;
  float out[KSQ];
#pragma unroll
  for (int r0 = 0; r0 < KSQ; r0 += RT) {
    if (lane) {
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const int t = kh * KS + kw - r0;
        if (t < 0 || t >= RT) continue;
#pragma unroll
        for (int q = 0; q < S; q += 4)
          *(float4*)(red + t * 256 + S * j + q) =
              make_float4(acc[q][kw], acc[q + 1][kw], acc[q + 2][kw],
                          acc[q + 3][kw]);
      }
    }
    rd_sync();
#pragma unroll
    for (int t = 0; t < RT; ++t)
      if (r0 + t < KSQ) out[r0 + t] = red[t * 256 + threadIdx.x];
    rd_sync();
  }
  float* slot = wsp + ((int64_t)blockIdx.y * C + c) * KSQ;
  block_reduce_sum(
      out, [&](int t, float v) { slot[t] = v; }, [] { rd_sync(); });
}

// ------------------------------------------------------------------- host
namespace {

bool strip_shape_ok(int64_t C, int64_t H, int64_t W, int64_t KS,
                    int64_t stride, int64_t pad) {
  if (C < 1 || H < 1 || W < 1 || (KS != 3 && KS != 5 && KS != 7) ||
      (stride != 1 && stride != 2) || pad != KS / 2 || W % 8 || H * W > 4096)
    return false;
  // stride 2: even planes, so that OH = H / 2 and OW = W / 2, whole chunks
  return stride == 1 || (H % 2 == 0 && W % 16 == 0);
}

DwShape check_strip(const at::Tensor& x, const char* xname,
                    const at::Tensor& y, const char* yname, int64_t taps,
                    int64_t stride, int64_t pad) {
  const DwShape s = check_images(x, xname, y, yname, taps, stride, pad);
  TORCH_CHECK(strip_shape_ok(s.C, s.H, s.W, s.KS, stride, pad),
              "relu_depthwise_strip: unsupported shape (KS in {3,5,7}, "
              "stride in {1,2}, pad == KS/2, W%8==0, H*W<=4096; stride 2: H "
              "even, W%16==0): H=", s.H, " W=", s.W, " KS=", s.KS,
              " stride=", stride, " pad=", pad);
  TORCH_CHECK((int64_t)s.B * s.C < (1LL << 31),
              "relu_depthwise_strip: B*C must stay below 2^31");
  for (const at::Tensor* t : {&x, &y})
    TORCH_CHECK((uintptr_t)t->data_ptr() % 16 == 0,
                "relu_depthwise_strip: tensors must be 16-byte aligned");
  return s;
}

DwShape check_strip(const at::Tensor& x, const char* xname,
                    const at::Tensor& y, const char* yname,
                    const at::Tensor& w, int64_t stride, int64_t pad) {
  check_bf16(w, "w");
  TORCH_CHECK((uintptr_t)w.data_ptr() % 16 == 0,
              "relu_depthwise_strip: tensors must be 16-byte aligned");
  return check_strip(x, xname, y, yname, w.numel(), stride, pad);
}

// Planes per block: enough strips for the 256 threads, within the LDS array.
int planes_per_block(int rows_out, int cols_out, int staged_px) {
  const int spp =
      ((rows_out + STRIP_ROWS - 1) / STRIP_ROWS) * (cols_out / 8);
  return std::max(1, std::min((256 + spp - 1) / spp, STRIP_LDS / staged_px));
}

}  // namespace

bool relu_depthwise_strip_supported(int64_t C, int64_t H, int64_t W,
                                    int64_t KS, int64_t stride, int64_t pad) {
  return strip_shape_ok(C, H, W, KS, stride, pad);
}

void relu_depthwise_strip_fwd(const at::Tensor& x, const at::Tensor& w,
                              at::Tensor& y, int64_t stride, int64_t pad) {
  const DwShape s = check_strip(x, "x", y, "y", w, stride, pad);
  const int bc = s.B * s.C;
  const int P = planes_per_block(s.OH, s.OW, s.H * s.W);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  with_const<3, 5, 7>(s.KS, [&](auto ks) {
    with_const<1, 2>((int)stride, [&](auto st) {
      hipLaunchKernelGGL(
          (relu_depthwise_strip_fwd_kernel<decltype(ks)::value,
                                           decltype(st)::value, STRIP_ROWS>),
          dim3((unsigned)((bc + P - 1) / P)), dim3(256), 0, stream,
          (const bf16_t*)x.data_ptr(), (const bf16_t*)w.data_ptr(),
          (bf16_t*)y.data_ptr(), s.C, s.H, s.W, s.OH, s.OW, P, bc);
    });
  });
  HIP_CHECK_KERNEL();
}

void relu_depthwise_strip_bwd_dx(const at::Tensor& x, const at::Tensor& dy,
                                 const at::Tensor& w, at::Tensor& dx,
                                 int64_t stride, int64_t pad) {
  const DwShape s = check_strip(x, "x", dy, "dy", w, stride, pad);
  check_bf16(dx, "dx");
  TORCH_CHECK(dx.sizes() == x.sizes() && (uintptr_t)dx.data_ptr() % 16 == 0,
              "relu_depthwise_strip: dx must have the shape of x and be "
              "16-byte aligned");
  const int bc = s.B * s.C;
  const int P = planes_per_block(s.H, s.W, s.OH * s.OW);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  with_const<3, 5, 7>(s.KS, [&](auto ks) {
    with_const<1, 2>((int)stride, [&](auto st) {
      hipLaunchKernelGGL(
          (relu_depthwise_strip_dx_kernel<decltype(ks)::value,
                                          decltype(st)::value, STRIP_ROWS>),
          dim3((unsigned)((bc + P - 1) / P)), dim3(256), 0, stream,
          (const bf16_t*)x.data_ptr(), (const bf16_t*)dy.data_ptr(),
          (const bf16_t*)w.data_ptr(), (bf16_t*)dx.data_ptr(), s.C, s.H, s.W,
          s.OH, s.OW, P, bc);
    });
  });
  HIP_CHECK_KERNEL();
}

void relu_depthwise_strip_bwd_dw(const at::Tensor& x, const at::Tensor& dy,
                                 at::Tensor& dw, int64_t stride,
                                 int64_t pad) {
  TORCH_CHECK(dw.is_cuda() && dw.is_contiguous() &&
                  dw.scalar_type() == at::kFloat,
              "relu_depthwise_strip: dw must be a contiguous fp32 CUDA "
              "tensor of C*KS*KS elements");
  const DwShape s = check_strip(x, "x", dy, "dy", dw.numel(), stride, pad);
  // relu_depthwise_bwd's partition (depthwise_bwd_dw's LDS tier): part of
  // the bit contract
  const int nchunks =
      (int)std::max<int64_t>(1, std::min<int64_t>(1024 / s.C, s.B));
  const int b_per_chunk = (s.B + nchunks - 1) / nchunks;
  const int G = std::max(
      1, std::min({STRIP_LDS / 2 / (s.H * s.W),
                   STRIP_LDS / 2 / (s.OH * s.OW), s.B}));
  const int ksq = s.KS * s.KS;
  at::Tensor wsp = at::empty({nchunks, s.C, ksq}, dw.options());
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  with_const<3, 5, 7>(s.KS, [&](auto ks) {
    with_const<1, 2>((int)stride, [&](auto st) {
      constexpr int K = decltype(ks)::value;
      hipLaunchKernelGGL(
          (relu_depthwise_strip_dw_kernel<K, decltype(st)::value,
                                          strip_dw_width(K)>),
          dim3((unsigned)s.C, (unsigned)nchunks), dim3(256), 0, stream,
          (const bf16_t*)x.data_ptr(), (const bf16_t*)dy.data_ptr(),
          wsp.data_ptr<float>(), s.B, s.C, s.H, s.W, s.OH, s.OW, b_per_chunk,
          G);
    });
  });
  launch_depthwise_dw_reduce(wsp.data_ptr<float>(), dw.data_ptr<float>(), s.C,
                             ksq, nchunks, stream);
  HIP_CHECK_KERNEL();
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
