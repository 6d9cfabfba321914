// The activation tile of the pointwise-conv kernels (relu_pointwise.hip,
// conv1x1_ragged.hip): channel-major staging with 16 B writes, MFMA A
// fragments through the transposing LDS read. The layout and its padding
// are documented at the top of relu_pointwise.hip.
//
// Include inside the file's no-packed-fp32-ops region: every function here
// must be compiled like its callers.
#pragma once

#include "common.h"

namespace {

constexpr int RP_KC = 32;             // channels per chunk = one MFMA K-step
constexpr int RP_ROWS = 48;           // row slots of a subtile: 32 + 4 x 4 pad
constexpr int RP_SUB = RP_ROWS * 16;  // bf16 per subtile before stride padding

typedef unsigned short u16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// activation subtile stride for tiles of 64 * FN pixels (1600 B / 1568 B)
template <int FN>
constexpr int rp_xsub() { return RP_SUB + 32 / FN; }

__device__ __forceinline__ void rp_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ReLU on two packed bf16: clear every half whose sign bit is set.
__device__ __forceinline__ unsigned rp_relu_pk(unsigned w) {
  const unsigned neg = (w >> 15) & 0x00010001u;
  return w & ~(neg * 0xffffu);
}
__device__ __forceinline__ unsigned rp_bf16_bits(float v) {
  const bf16_t h = f2bf(v);
  return *(const u16*)&h;
}
// four accumulator rows -> four packed bf16
__device__ __forceinline__ u32x2 rp_pack(const f32x4& a) {
  return u32x2{rp_bf16_bits(a[0]) | (rp_bf16_bits(a[1]) << 16),
               rp_bf16_bits(a[2]) | (rp_bf16_bits(a[3]) << 16)};
}

// first element of row k of a subtile (four pad rows after every eight)
__device__ __forceinline__ int rp_row(int k) { return (k + (k >> 3) * 4) * 16; }

__device__ __forceinline__ u32x2 rp_tr_read(const u16* lds) {
  const unsigned off = (unsigned)(uintptr_t)(
      __attribute__((address_space(3))) const u16*)lds;
  u32x2 out;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(out) : "v"(off) : "memory");
  return out;
}

// MFMA fragment of subtile T: lane l gets T[8 (l / 16) + j][l % 16], j = 0..7.
// ds_read_b64_tr_b16 hands lane l, for j = 0..3, element l % 4 of the 8 bytes
// that lane 16 (l / 16) + 4 j + (l / 4) % 4 addressed (gemm_tn.hip,
// tr_frag_addrs), so lane m addresses row 8 (m / 16) + (m / 4) % 4, column
// 4 (m % 4); the second read takes rows + 4. The caller waits (rp_wait_lds)
// before it uses the result.
__device__ __forceinline__ s16x8 rp_frag(const u16* sub, int lane) {
  const u16* a = sub + rp_row(8 * (lane >> 4) + ((lane >> 2) & 3)) +
                 4 * (lane & 3);
  union {
    s16x8 f;
    struct { u32x2 lo, hi; } u;
  } pack;
  pack.u.lo = rp_tr_read(a);
  pack.u.hi = rp_tr_read(a + 4 * 16);
  return pack.f;
}
// The compiler does not order MFMAs against inline-asm LDS reads.
__device__ __forceinline__ void rp_wait_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// One 32-channel slice of an activation tile of 64 * FN pixels: thread t
// carries vector t % VPR (8 pixels) of channels (t + 256 j) / VPR.
template <int FN, bool RELU>
struct RpStage {
  static constexpr int VPR = 8 * FN;  // 16 B vectors per channel row
  u32x4 st[FN];
  int pv, c0;

  __device__ __forceinline__ RpStage()
      : pv(threadIdx.x % VPR), c0(threadIdx.x / VPR) {}

  // src: channel 0 of the slice at the tile's first pixel; live: the
  // thread's vector lies inside the image
  __device__ __forceinline__ void prefetch(const u16* src, int hw, bool live) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      st[j] = u32x4{0, 0, 0, 0};
      if (live)
        st[j] = *(const u32x4*)(src + (int64_t)(c0 + j * (256 / VPR)) * hw +
                                pv * 8);
    }
  }
  // prefetch for a slice of which only the first `rows` channels exist:
  // the others are zero in LDS and are never read from memory
  __device__ __forceinline__ void prefetch_rows(const u16* src, int hw,
                                                bool live, int rows) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int c = c0 + j * (256 / VPR);
      st[j] = u32x4{0, 0, 0, 0};
      if (live && c < rows)
        st[j] = *(const u32x4*)(src + (int64_t)c * hw + pv * 8);
    }
  }
  __device__ __forceinline__ void commit(u16* tile) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      u32x4 q = st[j];
      if (RELU)
        q = u32x4{rp_relu_pk(q.x), rp_relu_pk(q.y), rp_relu_pk(q.z),
                  rp_relu_pk(q.w)};
      *(u32x4*)(tile + (pv >> 1) * rp_xsub<FN>() +
                rp_row(c0 + j * (256 / VPR)) + (pv & 1) * 8) = q;
    }
  }
};

}  // namespace
