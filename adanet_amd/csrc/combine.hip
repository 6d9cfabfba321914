// NASNet cell combine (K3): per-sample drop-path scale, left+right add and
// channel concat of up to 8 blocks in ONE launch, plus the matching
// backward. Replaces, per block, two broadcast multiplies, one add and a
// share of torch.cat (16 launches and nine passes over each block's
// activation per normal cell) with three passes: read left, read right,
// write the concat slot.
//
// Bit-exact with the unfused torch composition by construction: every
// intermediate torch materialises in bf16 is rounded to bf16 here too
// (product, product, sum — round-to-nearest-even, NaN-safe f2bf), and the
// drop-path scale is always MULTIPLIED, never selected on, so inf * 0 stays
// NaN and -x * 0 stays -0 exactly as in torch.
//
// Pointers travel in a by-value kernel-argument struct (like CopyPtrs in
// elementwise.hip): launch count is independent of the block count and
// hipGraph capture bakes the addresses. grid.y = block pair (uniform per
// workgroup, so the pointer pick is a scalar kernarg load); grid.x
// grid-strides over the B * chunk elements of that pair. No atomics, no
// reductions: deterministic by construction. Inputs are read-only and may
// alias each other (the `id` op hands the cell input itself to a block).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

// The three roundings must survive the optimiser. With contraction on, a
// product whose operands were both widened from bf16 is narrowed to a bf16
// multiply and then fused with the add into one fma — a single rounding that
// differs from torch in the last bit. Contraction stays off in this file and
// bf16 values are widened with integer shifts, never a float extension.
#pragma clang fp contract(off)

#define COMBINE_MAX 8

struct CombineFwdPtrs {
  const bf16_t* l[COMBINE_MAX];
  const bf16_t* r[COMBINE_MAX];
  const bf16_t* sl[COMBINE_MAX];  // per-sample scale, B elements (or null)
  const bf16_t* sr[COMBINE_MAX];
};

struct CombineBwdPtrs {
  bf16_t* dl[COMBINE_MAX];  // null = that input needs no gradient
  bf16_t* dr[COMBINE_MAX];
  const bf16_t* sl[COMBINE_MAX];
  const bf16_t* sr[COMBINE_MAX];
};

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_cb;

__device__ __forceinline__ float cb_lo(unsigned int u) {
  return __uint_as_float(u << 16);
}
__device__ __forceinline__ float cb_hi(unsigned int u) {
  return __uint_as_float(u & 0xffff0000u);
}
__device__ __forceinline__ float cb_ld(const bf16_t* p) {
  return __uint_as_float((unsigned int)__bfloat16_as_ushort(*p) << 16);
}
__device__ __forceinline__ unsigned int cb_pack(float a, float b) {
  return (unsigned int)__bfloat16_as_ushort(f2bf(a)) |
         ((unsigned int)__bfloat16_as_ushort(f2bf(b)) << 16);
}
// bf16(x * s) widened back to fp32: the intermediate torch materialises.
__device__ __forceinline__ float cb_mul(float x, float s) {
  return __uint_as_float((unsigned int)__bfloat16_as_ushort(f2bf(x * s))
                         << 16);
}

// out[b, (i0 + i) * chunk + e] = bf16(bf16(l*sl[b]) + bf16(r*sr[b])).
// `per` = work items per sample: chunk / 8 (VEC) or chunk (scalar).
// `out` already points at block i0's slot of sample 0; `out_bstride` is the
// full concat row, n_total * chunk.
template <bool VEC, bool SCALED>
__global__ __launch_bounds__(256) void cell_combine_fwd_kernel(
    CombineFwdPtrs P, bf16_t* __restrict__ out, int64_t B, int64_t per,
    int64_t chunk, int64_t out_bstride) {
  const int i = blockIdx.y;
  const bf16_t* l = P.l[i];
  const bf16_t* r = P.r[i];
  const bf16_t* sl = P.sl[i];
  const bf16_t* sr = P.sr[i];
  bf16_t* o = out + (int64_t)i * chunk;
  const int64_t total = B * per;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int64_t b = t / per;
    const int64_t e = (t - b * per) * (VEC ? 8 : 1);
    const int64_t src = b * chunk + e;
    const int64_t dst = b * out_bstride + e;
    float fl = 1.f, fr = 1.f;
    if (SCALED) {  // one scale load per vector, not per element
      fl = cb_ld(sl + b);
      fr = cb_ld(sr + b);
    }
    if (VEC) {
      const u32x4_cb a = *(const u32x4_cb*)(l + src);
      const u32x4_cb c = *(const u32x4_cb*)(r + src);
      u32x4_cb y;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float a0 = cb_lo(a[k]), a1 = cb_hi(a[k]);
        float c0 = cb_lo(c[k]), c1 = cb_hi(c[k]);
        if (SCALED) {
          a0 = cb_mul(a0, fl);
          a1 = cb_mul(a1, fl);
          c0 = cb_mul(c0, fr);
          c1 = cb_mul(c1, fr);
        }
        y[k] = cb_pack(a0 + c0, a1 + c1);
      }
      *(u32x4_cb*)(o + dst) = y;
    } else {
      float a0 = cb_ld(l + src), c0 = cb_ld(r + src);
      if (SCALED) {
        a0 = cb_mul(a0, fl);
        c0 = cb_mul(c0, fr);
      }
      o[dst] = f2bf(a0 + c0);
    }
  }
}

// dl_i[b, e] = bf16(dy[b, (i0+i)*chunk + e] * sl[b]); dr_i likewise. Each dy
// element is read once; a null output slot is skipped.
template <bool VEC>
__global__ __launch_bounds__(256) void cell_combine_bwd_kernel(
    CombineBwdPtrs P, const bf16_t* __restrict__ dy, int64_t B, int64_t per,
    int64_t chunk, int64_t dy_bstride) {
  const int i = blockIdx.y;
  bf16_t* dl = P.dl[i];
  bf16_t* dr = P.dr[i];
  if (dl == nullptr && dr == nullptr) return;
  const bf16_t* sl = P.sl[i];
  const bf16_t* sr = P.sr[i];
  const bf16_t* g = dy + (int64_t)i * chunk;
  const int64_t total = B * per;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int64_t b = t / per;
    const int64_t e = (t - b * per) * (VEC ? 8 : 1);
    const int64_t src = b * dy_bstride + e;
    const int64_t dst = b * chunk + e;
    const float fl = cb_ld(sl + b);
    const float fr = cb_ld(sr + b);
    if (VEC) {
      const u32x4_cb v = *(const u32x4_cb*)(g + src);
      u32x4_cb yl, yr;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float v0 = cb_lo(v[k]), v1 = cb_hi(v[k]);
        yl[k] = cb_pack(v0 * fl, v1 * fl);
        yr[k] = cb_pack(v0 * fr, v1 * fr);
      }
      if (dl != nullptr) *(u32x4_cb*)(dl + dst) = yl;
      if (dr != nullptr) *(u32x4_cb*)(dr + dst) = yr;
    } else {
      const float v0 = cb_ld(g + src);
      if (dl != nullptr) dl[dst] = f2bf(v0 * fl);
      if (dr != nullptr) dr[dst] = f2bf(v0 * fr);
    }
  }
}

static bool cb_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// grid.x for `total` work items per pair over `n` pairs: ~2048 blocks in
// all (256 CUs x 8), the rest grid-strided.
static unsigned cb_grid_x(int64_t total, int n) {
  const int64_t cap = std::max<int64_t>(1, 2048 / n);
  return (unsigned)std::max<int64_t>(1, std::min((total + 255) / 256, cap));
}

static void cb_check(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                  t.is_contiguous(),
              "cell_combine: ", what, " must be contiguous bf16 on the GPU");
}

// `out` is the full [B, n_total*F, H, W] concat buffer; this call fills
// blocks [block_offset, block_offset + n). scales_l/scales_r are both empty
// (no drop-path) or both hold n tensors of B elements.
void cell_combine_fwd(const std::vector<at::Tensor>& lefts,
                      const std::vector<at::Tensor>& rights,
                      const std::vector<at::Tensor>& scales_l,
                      const std::vector<at::Tensor>& scales_r, at::Tensor& out,
                      int64_t block_offset) {
  const int n = (int)lefts.size();
  TORCH_CHECK(n >= 1 && n <= COMBINE_MAX, "cell_combine_fwd: 1..8 pairs");
  TORCH_CHECK((int)rights.size() == n, "cell_combine_fwd: pair count");
  const bool scaled = !scales_l.empty() || !scales_r.empty();
  if (scaled)
    TORCH_CHECK((int)scales_l.size() == n && (int)scales_r.size() == n,
                "cell_combine_fwd: scale lists must both hold one per pair");
  cb_check(out, "out");
  TORCH_CHECK(lefts[0].dim() == 4 && out.dim() == 4, "cell_combine_fwd: NCHW");
  const int64_t B = lefts[0].size(0);
  const int64_t chunk = lefts[0].numel() / std::max<int64_t>(B, 1);
  TORCH_CHECK(out.size(0) == B && chunk > 0 && B > 0 &&
                  out.numel() % (B * chunk) == 0,
              "cell_combine_fwd: out shape");
  const int64_t n_total = out.numel() / (B * chunk);
  TORCH_CHECK(block_offset >= 0 && block_offset + n <= n_total,
              "cell_combine_fwd: block range outside out");
  TORCH_CHECK(chunk < ((int64_t)1 << 40), "cell_combine_fwd: chunk too large");
  const int64_t out_bstride = n_total * chunk;
  bf16_t* o = (bf16_t*)out.data_ptr() + block_offset * chunk;

  CombineFwdPtrs P;
  bool vec = chunk % 8 == 0 && cb_al16(o);
  for (int k = 0; k < COMBINE_MAX; ++k) {
    P.l[k] = P.r[k] = P.sl[k] = P.sr[k] = nullptr;
  }
  for (int k = 0; k < n; ++k) {
    cb_check(lefts[k], "lefts");
    cb_check(rights[k], "rights");
    TORCH_CHECK(lefts[k].sizes() == lefts[0].sizes() &&
                    rights[k].sizes() == lefts[0].sizes(),
                "cell_combine_fwd: all inputs share one [B,F,H,W] shape");
    P.l[k] = (const bf16_t*)lefts[k].data_ptr();
    P.r[k] = (const bf16_t*)rights[k].data_ptr();
    vec = vec && cb_al16(P.l[k]) && cb_al16(P.r[k]);
    if (scaled) {
      cb_check(scales_l[k], "scales_l");
      cb_check(scales_r[k], "scales_r");
      TORCH_CHECK(scales_l[k].numel() == B && scales_r[k].numel() == B,
                  "cell_combine_fwd: a scale holds one element per sample");
      P.sl[k] = (const bf16_t*)scales_l[k].data_ptr();
      P.sr[k] = (const bf16_t*)scales_r[k].data_ptr();
    }
  }
  const int64_t per = vec ? chunk / 8 : chunk;
  const dim3 grid(cb_grid_x(B * per, n), (unsigned)n);
  auto stream = at::cuda::getCurrentCUDAStream();
#define CB_FWD(V, S)                                                         \
  hipLaunchKernelGGL((cell_combine_fwd_kernel<V, S>), grid, dim3(256), 0,    \
                     stream.stream(), P, o, B, per, chunk, out_bstride)
  if (vec) {
    if (scaled) CB_FWD(true, true); else CB_FWD(true, false);
  } else {
    if (scaled) CB_FWD(false, true); else CB_FWD(false, false);
  }
#undef CB_FWD
  HIP_CHECK_KERNEL();
}

// dy is the full [B, n_total*F, H, W] gradient; this call handles blocks
// [block_offset, block_offset + n). dlefts[k] / drights[k] undefined (None)
// = no gradient wanted for that input.
void cell_combine_bwd(const at::Tensor& dy,
                      const std::vector<at::Tensor>& scales_l,
                      const std::vector<at::Tensor>& scales_r,
                      const std::vector<c10::optional<at::Tensor>>& dlefts,
                      const std::vector<c10::optional<at::Tensor>>& drights,
                      int64_t block_offset) {
  const int n = (int)scales_l.size();
  TORCH_CHECK(n >= 1 && n <= COMBINE_MAX, "cell_combine_bwd: 1..8 pairs");
  TORCH_CHECK((int)scales_r.size() == n && (int)dlefts.size() == n &&
                  (int)drights.size() == n,
              "cell_combine_bwd: pair count");
  // dy may be a channel slice of an enclosing concat's gradient: each
  // sample dense, any batch stride that keeps samples apart.
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
                  dy.dim() == 4,
              "cell_combine_bwd: dy must be a 4-d bf16 GPU tensor");
  const int64_t B = dy.size(0);
  TORCH_CHECK(B > 0 && dy.numel() > 0, "cell_combine_bwd: empty dy");
  const int64_t dy_row = dy.numel() / B;
  TORCH_CHECK(dy.select(0, 0).is_contiguous() &&
                  (B == 1 || dy.stride(0) >= dy_row),
              "cell_combine_bwd: dy samples must be dense and disjoint");
  const int64_t dy_bstride = B == 1 ? dy_row : dy.stride(0);

  CombineBwdPtrs P;
  for (int k = 0; k < COMBINE_MAX; ++k) {
    P.dl[k] = P.dr[k] = nullptr;
    P.sl[k] = P.sr[k] = nullptr;
  }
  int64_t chunk = -1;
  bool any = false, vec = true;
  for (int k = 0; k < n; ++k) {
    cb_check(scales_l[k], "scales_l");
    cb_check(scales_r[k], "scales_r");
    TORCH_CHECK(scales_l[k].numel() == B && scales_r[k].numel() == B,
                "cell_combine_bwd: a scale holds one element per sample");
    P.sl[k] = (const bf16_t*)scales_l[k].data_ptr();
    P.sr[k] = (const bf16_t*)scales_r[k].data_ptr();
    for (int side = 0; side < 2; ++side) {
      const c10::optional<at::Tensor>& d = side ? drights[k] : dlefts[k];
      if (!d.has_value() || !d->defined()) continue;
      cb_check(*d, "gradient output");
      TORCH_CHECK(d->size(0) == B && d->numel() % B == 0,
                  "cell_combine_bwd: gradient output batch");
      const int64_t c = d->numel() / B;
      TORCH_CHECK(chunk < 0 || c == chunk,
                  "cell_combine_bwd: gradient outputs share one shape");
      chunk = c;
      bf16_t* p = (bf16_t*)d->data_ptr();
      vec = vec && cb_al16(p);
      (side ? P.dr[k] : P.dl[k]) = p;
      any = true;
    }
  }
  if (!any) return;
  TORCH_CHECK(chunk > 0 && dy.numel() % (B * chunk) == 0,
              "cell_combine_bwd: dy shape");
  const int64_t n_total = dy.numel() / (B * chunk);
  TORCH_CHECK(block_offset >= 0 && block_offset + n <= n_total,
              "cell_combine_bwd: block range outside dy");
  const bf16_t* g = (const bf16_t*)dy.data_ptr() + block_offset * chunk;
  vec = vec && chunk % 8 == 0 && dy_bstride % 8 == 0 && cb_al16(g);
  const int64_t per = vec ? chunk / 8 : chunk;
  const dim3 grid(cb_grid_x(B * per, n), (unsigned)n);
  auto stream = at::cuda::getCurrentCUDAStream();
  if (vec) {
    hipLaunchKernelGGL((cell_combine_bwd_kernel<true>), grid, dim3(256), 0,
                       stream.stream(), P, g, B, per, chunk, dy_bstride);
  } else {
    hipLaunchKernelGGL((cell_combine_bwd_kernel<false>), grid, dim3(256), 0,
                       stream.stream(), P, g, B, per, chunk, dy_bstride);
  }
  HIP_CHECK_KERNEL();
}
