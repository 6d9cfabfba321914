// Pointwise (1x1) conv, forward and input gradient, for channel counts off
// the 32 grid (any Ci >= 1, Co >= 1), operands where they lie:
//
//   y[b]  = bf16(W @ x[b])        x  [B, Ci, HW], W [Co, Ci]    K = Ci
//   dx[b] = bf16(W^T @ dy[b])     dy [B, Co, HW]                K = Co
//
// Both are out[b][n][p] = sum_k Wop(n, k) act[b][k][p] with Wop(n, k) =
// W[n][k] (forward) or W[k][n] (dX: TRW), one kernel. No operand is padded
// in memory; the raggedness is handled in three places:
//
//   * K tail. The K loop runs ceil(K / 32) chunks of one MFMA K-step
//     (mfma_f32_16x16x32_bf16). Rows k >= K of the last activation slice
//     are written to LDS as zeros and never loaded (RpStage::prefetch_rows),
//     so neither the next image nor memory past the buffer can reach a sum:
//     zero weights alone would leave 0 * Inf = NaN. The weight tile is zero
//     there too.
//   * Weight rows are not 16 B aligned once Ci % 8 != 0. W is small and
//     L2-resident, so each block stages its [16 CF n][32 k] slice per chunk
//     with guarded narrow loads, 4 bytes when Ci is even (and W is 4-byte
//     aligned) and 2 bytes otherwise, zero past N and K, straight into the
//     layout the MFMA B operand reads: fragment c, lane l holds the 8
//     consecutive k = 8 (l / 16) + j of row 16 c + l % 16 as one 16 B
//     vector. The four k-groups of a fragment are 320 B apart (64 B mod
//     256), so the 64 forward pair-writes of a wave (4 rows x 16 pairs) hit
//     64 distinct banks and the 16 B fragment reads of any 16 lanes are
//     contiguous.
//   * Output rows n >= N and pixels >= HW are masked in the epilogue.
//
// Everything else is relu_pointwise.hip's discipline (pointwise_tile.h):
// pixels are the MFMA rows and channels the columns, so a lane's four
// accumulators are four consecutive pixels of one channel and the epilogue
// is one 8 B store; activations are staged channel-major with 16 B writes
// and transposed on the read; two LDS buffers, operands of the next chunk
// carried in registers across the MFMA work, one barrier per chunk.
//
// Work split: grid (pixel tiles, N tiles, B), 256 threads. A block owns 128
// pixels (64 where the image has no more) times 16 CF output channels,
// CF in {1, 2, 4, 8} by min(N, 128); wave w owns pixels 32 w .. 32 w + 31 of
// every channel, so no activation fragment is read by two waves. N above
// 128 takes more tiles on grid.y, each re-reading the (L2-resident)
// activation tile.
//
// One fp32 accumulator per output element over ascending 32-wide K steps,
// rounded once: gemm_tr_kernel's order, so the results equal the aligned
// path's on zero-padded operands bit for bit (the extra products are +0).
//
// The weight gradient at these counts is conv1x1_dw (gemm.hip): K = B*HW is
// never ragged there and its kernel already clamps and masks both output
// axes and stores 2 bytes at a time.
//
// No allocation, no atomics, no host sync; launches on the current stream.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "pointwise_tile.h"

namespace {

constexpr int PWR_WKG = 160;             // bf16 between k-groups (320 B)
constexpr int PWR_WFRAG = 4 * PWR_WKG;   // bf16 per 16-channel fragment
constexpr int PWR_MAX_C = 1 << 16;
constexpr int PWR_MAX_HW = 1 << 24;

// element (n, k) of a staged weight slice
__device__ __forceinline__ int pwr_widx(int n, int k) {
  return (n >> 4) * PWR_WFRAG + (k >> 3) * PWR_WKG + (n & 15) * 8 + (k & 7);
}

// The [16 CF n][32 k] weight slice of one chunk. A unit is U = 1 or 2
// (PAIR) elements along the axis that is contiguous in memory: k for the
// forward, n for dX. Thread t carries units t, t + 256, ...; neighbouring
// threads read neighbouring addresses.
template <int CF, bool TRW, bool PAIR>
struct PwrWeights {
  static constexpr int NT = 16 * CF;
  static constexpr int U = PAIR ? 2 : 1;
  static constexpr int PER = NT * RP_KC / U / 256;
  static constexpr int UPR = (TRW ? NT : RP_KC) / U;  // units per memory row
  unsigned st[PER];

  __device__ __forceinline__ static void unit(int i, int& n, int& k) {
    const int q = threadIdx.x + 256 * i;
    const int major = q / UPR, minor = (q % UPR) * U;
    n = TRW ? minor : major;
    k = TRW ? major : minor;
  }
  // With PAIR both the unit's first index and the extent of its axis are
  // even, so a unit lies inside or outside as a whole.
  __device__ __forceinline__ void prefetch(const u16* w, int n0, int k0, int N,
                                           int K, int Ci) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      int n, k;
      unit(i, n, k);
      n += n0, k += k0;
      st[i] = 0;
      if (n < N && k < K) {
        const u16* at = w + (TRW ? (int64_t)k * Ci + n : (int64_t)n * Ci + k);
        st[i] = PAIR ? *(const unsigned*)at : (unsigned)*at;
      }
    }
  }
  __device__ __forceinline__ void commit(u16* tile) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      int n, k;
      unit(i, n, k);
      if (PAIR && !TRW) {
        *(unsigned*)(tile + pwr_widx(n, k)) = st[i];  // k even: same vector
      } else {
        tile[pwr_widx(n, k)] = (u16)st[i];
        if (PAIR) tile[pwr_widx(n + 1, k)] = (u16)(st[i] >> 16);
      }
    }
  }
};

template <int CF, int FN, bool TRW, bool PAIR>
__global__ __launch_bounds__(256, 2) void conv1x1_ragged_kernel(
    const bf16_t* __restrict__ act, const bf16_t* __restrict__ w,
    bf16_t* __restrict__ out, int N, int K, int Ci, int hw, int64_t act_img,
    int64_t out_img) {
  constexpr int XS = rp_xsub<FN>();
  __shared__ __align__(16) u16 xs[2][4 * FN * XS];
  __shared__ __align__(16) u16 ws[2][CF * PWR_WFRAG];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.z, n0 = blockIdx.y * (16 * CF);
  const int p0 = blockIdx.x * (64 * FN);

  RpStage<FN, false> sg;
  PwrWeights<CF, TRW, PAIR> wg;
  const bool live = p0 + sg.pv * 8 < hw;
  const u16* ab = (const u16*)act + (int64_t)b * act_img + p0;
  const u16* wp = (const u16*)w;

  f32x4 acc[FN][CF];
#pragma unroll
  for (int f = 0; f < FN; ++f)
#pragma unroll
    for (int c = 0; c < CF; ++c) acc[f][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nch = (K + RP_KC - 1) / RP_KC;
  sg.prefetch_rows(ab, hw, live, K);
  wg.prefetch(wp, n0, 0, N, K, Ci);
  sg.commit(xs[0]);
  wg.commit(ws[0]);
  rp_sync();

  for (int ch = 0; ch < nch; ++ch) {
    const bool more = ch + 1 < nch;
    if (more) {
      const int k1 = (ch + 1) * RP_KC;
      sg.prefetch_rows(ab + (int64_t)k1 * hw, hw, live, K - k1);
      wg.prefetch(wp, n0, k1, N, K, Ci);
    }
    s16x8 a[FN], bw[CF];
#pragma unroll
    for (int f = 0; f < FN; ++f)
      a[f] = rp_frag(xs[ch & 1] + (wid * FN + f) * XS, lane);
#pragma unroll
    for (int c = 0; c < CF; ++c)
      bw[c] = *(const s16x8*)(ws[ch & 1] + c * PWR_WFRAG +
                              (lane >> 4) * PWR_WKG + (lane & 15) * 8);
    rp_wait_lds();
#pragma unroll
    for (int f = 0; f < FN; ++f)
#pragma unroll
      for (int c = 0; c < CF; ++c)
        acc[f][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[f], bw[c], acc[f][c], 0, 0, 0);
    // the other buffers were last read before the previous barrier
    if (more) {
      sg.commit(xs[(ch + 1) & 1]);
      wg.commit(ws[(ch + 1) & 1]);
    }
    rp_sync();
  }

  // a lane's registers: pixels px..px+3 of channel n0 + c * 16 + lane % 16
  u16* ob = (u16*)out + (int64_t)b * out_img;
#pragma unroll
  for (int f = 0; f < FN; ++f) {
    const int px = p0 + (wid * FN + f) * 16 + (lane >> 4) * 4;
    if (px >= hw) continue;  // HW % 8 == 0: all four pixels or none
#pragma unroll
    for (int c = 0; c < CF; ++c) {
      const int n = n0 + c * 16 + (lane & 15);
      if (n < N) *(u32x2*)(ob + (int64_t)n * hw + px) = rp_pack(acc[f][c]);
    }
  }
}

// ------------------------------------------------------------------- host
// act [B, C, HW] with dense images (any batch stride that keeps 16 B
// alignment), bf16, on the GPU
void pwr_check_act(const at::Tensor& t, const char* fn, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                  t.dim() == 3 && t.numel() > 0 && t.stride(2) == 1 &&
                  t.stride(1) == t.size(2) && t.stride(0) % 8 == 0 &&
                  t.stride(0) >= t.size(1) * t.size(2) &&
                  ((uintptr_t)t.data_ptr() & 15) == 0,
              fn, ": ", name, " must be a non-empty, 16-byte aligned bf16 "
              "CUDA tensor [B,C,HW] with dense images");
}

template <int CF, int FN, bool TRW>
void pwr_launch_pair(bool pair, dim3 grid, hipStream_t stream,
                     const at::Tensor& act, const at::Tensor& w,
                     at::Tensor& out, int N, int K, int Ci, int hw) {
  auto k = pair ? conv1x1_ragged_kernel<CF, FN, TRW, true>
                : conv1x1_ragged_kernel<CF, FN, TRW, false>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, stream,
                     (const bf16_t*)act.data_ptr(),
                     (const bf16_t*)w.data_ptr(), (bf16_t*)out.data_ptr(), N,
                     K, Ci, hw, (int64_t)act.stride(0), (int64_t)out.stride(0));
}

// out[b] = Wop @ act[b], Wop = w (forward) or w^T (TRW)
template <bool TRW>
void pwr_run(const char* fn, const at::Tensor& act, const at::Tensor& w,
             at::Tensor& out) {
  pwr_check_act(act, fn, TRW ? "dy" : "x");
  pwr_check_act(out, fn, TRW ? "dx" : "y");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 &&
                  w.dim() == 2 && w.is_contiguous() &&
                  ((uintptr_t)w.data_ptr() & 1) == 0,
              fn, ": w must be a contiguous bf16 CUDA tensor [Co,Ci]");
  TORCH_CHECK(act.get_device() == w.get_device() &&
                  act.get_device() == out.get_device(),
              fn, ": tensors on different devices");
  const int64_t Co = w.size(0), Ci = w.size(1);
  const int64_t N = TRW ? Ci : Co, K = TRW ? Co : Ci;
  const int64_t B = act.size(0), HW = act.size(2);
  TORCH_CHECK(act.size(1) == K && out.size(0) == B && out.size(1) == N &&
                  out.size(2) == HW,
              fn, ": shapes disagree: act ", act.sizes(), ", w ", w.sizes(),
              ", out ", out.sizes());
  TORCH_CHECK(Co >= 1 && Ci >= 1 && Co <= PWR_MAX_C && Ci <= PWR_MAX_C, fn,
              ": channel counts must lie in [1, ", PWR_MAX_C, "]");
  TORCH_CHECK(HW % 8 == 0 && HW <= PWR_MAX_HW, fn,
              ": needs HW % 8 == 0 and HW <= ", PWR_MAX_HW, ", got ", HW);
  TORCH_CHECK(B <= 65535, fn, ": B must be at most 65535");

  const int hw = (int)HW;
  const int fnp = hw > 64 ? 2 : 1;  // 128-pixel tiles, 64 for small images
  const int nmin = (int)std::min<int64_t>(N, 128);
  const int cf = nmin <= 16 ? 1 : nmin <= 32 ? 2 : nmin <= 64 ? 4 : 8;
  const dim3 grid((unsigned)((hw + 64 * fnp - 1) / (64 * fnp)),
                  (unsigned)((N + 16 * cf - 1) / (16 * cf)), (unsigned)B);
  const bool pair = Ci % 2 == 0 && ((uintptr_t)w.data_ptr() & 3) == 0;
  auto stream = at::cuda::getCurrentCUDAStream().stream();
#define PWR_CASE(CF_, FN_)                                                 \
  if (cf == CF_ && fnp == FN_)                                             \
    pwr_launch_pair<CF_, FN_, TRW>(pair, grid, stream, act, w, out, (int)N, \
                                   (int)K, (int)Ci, hw)
  PWR_CASE(1, 1); PWR_CASE(2, 1); PWR_CASE(4, 1); PWR_CASE(8, 1);
  PWR_CASE(1, 2); PWR_CASE(2, 2); PWR_CASE(4, 2); PWR_CASE(8, 2);
#undef PWR_CASE
  HIP_CHECK_KERNEL();
}

}  // namespace

// y3 [B,Co,HW] = w [Co,Ci] @ x3 [B,Ci,HW] per image, any Ci, Co >= 1
void conv1x1_ragged_fwd(const at::Tensor& x3, const at::Tensor& w,
                        at::Tensor& y3) {
  pwr_run<false>("conv1x1_ragged_fwd", x3, w, y3);
}

// dx3 [B,Ci,HW] = w^T @ dy3 [B,Co,HW] per image, any Ci, Co >= 1
void conv1x1_ragged_dx(const at::Tensor& dy3, const at::Tensor& w,
                       at::Tensor& dx3) {
  pwr_run<true>("conv1x1_ragged_dx", dy3, w, dx3);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
