// Device-resident image pipeline: the whole dataset lives in HBM as uint8
// (or fp32 for the synthetic provider) and a training batch is produced by
// two launches, with no host pixel work and no host-to-device copy.
//
//   augment_draw   one thread per batch slot: draws (index, oy, ox, flip,
//                  cy, cx) from the stateless counter RNG (hash_rng) and
//                  gathers the label. Batch s of a stream is a pure function
//                  of (seed, s, rank, world), so it can be regenerated
//                  anywhere, in any order.
//   augment_apply  gather + pad-crop + flip + cutout + normalise + bf16 cast
//                  in one pass: reads 1 byte (4 for fp32 data), writes 2
//                  bytes per pixel.
//
// Each thread of augment_apply produces 8 consecutive x of one output row and
// stores them with one 16-byte store (scalar variant when W % 8 != 0 or `out`
// is not 16-byte aligned). Source pixels are read with scalar loads: after
// the crop shift they are unaligned and under flip they run backwards, and a
// 3 KB image stays in cache. No LDS, no atomics, no reductions: deterministic
// by construction.
//
// The parameters live on the device and cannot be validated from the host
// without a sync, so the kernel trusts none of them: `index` is clamped to
// [0, N-1], every source coordinate is tested against the image, and the
// coordinate arithmetic is 64-bit. Whatever `params` holds, no read leaves
// `data`.

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

// value = bf16(float(src) * scale + shift) with the multiply and the add as
// two fp32 roundings, so that a torch fp32 reference is bit-identical.
#pragma clang fp contract(off)

#define AUG_FIELDS 6  // index, oy, ox, flip, cy, cx

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_ag;

__device__ __forceinline__ float ag_ld(const uint8_t* p) { return (float)*p; }
__device__ __forceinline__ float ag_ld(const float* p) { return *p; }

__device__ __forceinline__ unsigned int ag_pack(float a, float b) {
  return (unsigned int)__bfloat16_as_ushort(f2bf(a)) |
         ((unsigned int)__bfloat16_as_ushort(f2bf(b)) << 16);
}

__device__ __forceinline__ int64_t ag_max(int64_t a, int64_t b) {
  return a > b ? a : b;
}
__device__ __forceinline__ int64_t ag_min(int64_t a, int64_t b) {
  return a < b ? a : b;
}

// [0, n) from a 32-bit draw, without modulo bias worth the name and without
// a division.
__device__ __forceinline__ int ag_range(uint32_t r, int64_t n) {
  return (int)(((uint64_t)r * (uint64_t)n) >> 32);
}

__global__ __launch_bounds__(256) void augment_draw_kernel(
    const int64_t* __restrict__ labels, int* __restrict__ params,
    int64_t* __restrict__ labels_out, uint64_t seed, uint64_t step,
    uint64_t rank, uint64_t world, int64_t N, int64_t B, int64_t pad,
    int64_t H, int64_t W, int augment) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint64_t ctr = (step * world + rank) * (uint64_t)B + (uint64_t)b;
  const uint64_t base = ctr * 8;
  const int index = ag_range(hash_rng(seed, base + 0), N);
  int oy = ag_range(hash_rng(seed, base + 1), 2 * pad + 1);
  int ox = ag_range(hash_rng(seed, base + 2), 2 * pad + 1);
  int flip = (int)(hash_rng(seed, base + 3) >> 31);
  const int cy = ag_range(hash_rng(seed, base + 4), H);
  const int cx = ag_range(hash_rng(seed, base + 5), W);
  if (!augment) {  // centre crop, no flip; the caller turns cutout off
    oy = ox = (int)pad;
    flip = 0;
  }
  int* p = params + b * AUG_FIELDS;
  p[0] = index;
  p[1] = oy;
  p[2] = ox;
  p[3] = flip;
  p[4] = cy;
  p[5] = cx;
  labels_out[b] = labels[index];  // index < N by construction
}

// One work item = 8 consecutive x (VEC) or one x of an output row; work item
// t writes out[t * 8 ..] (resp. out[t]) because it enumerates [B, C, H, W]
// in memory order. `per_img` = work items per sample, < 2^31.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void augment_apply_kernel(
    const T* __restrict__ data, const int* __restrict__ params,
    const float* __restrict__ scale, const float* __restrict__ shift,
    bf16_t* __restrict__ out, int64_t N, int64_t B, int C, int H, int W,
    int per_row, int per_img, int64_t pad, int64_t cutout_pad) {
  constexpr int V = VEC ? 8 : 1;
  const int64_t total = B * per_img;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const int64_t b = t / per_img;
    int rem = (int)(t - b * per_img);
    const int x0 = (rem % per_row) * V;
    rem /= per_row;
    const int y = rem % H;
    const int c = rem / H;

    // One parameter load per thread, not per element.
    const int* p = params + b * AUG_FIELDS;
    int64_t index = p[0];
    index = index < 0 ? 0 : (index >= N ? N - 1 : index);
    const int64_t oy = p[1], ox = p[2];
    const bool flip = p[3] != 0;
    const int64_t cy = p[4], cx = p[5];

    const int64_t sy = (int64_t)y + oy - pad;
    const bool row_ok = sy >= 0 && sy < H;
    const bool cut_row = cutout_pad > 0 &&
                         (int64_t)y >= ag_max(0, cy - cutout_pad) &&
                         (int64_t)y < ag_min(H, cy + cutout_pad);
    const int64_t cut_x0 = ag_max(0, cx - cutout_pad);
    const int64_t cut_x1 = ag_min(W, cx + cutout_pad);
    const T* src = data + ((index * C + c) * H + (row_ok ? sy : 0)) * W;
    const float sc = scale[c], sh = shift[c];

    float v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int64_t x = x0 + k;
      const int64_t sx = (flip ? (int64_t)W - 1 - x : x) + ox - pad;
      const bool cut = cut_row && x >= cut_x0 && x < cut_x1;
      const bool ok = row_ok && sx >= 0 && sx < W && !cut;
      float val = 0.f;
      if (ok) {
        val = ag_ld(src + sx) * sc;
        val = val + sh;
      }
      v[k] = val;
    }
    if constexpr (VEC) {
      u32x4_ag o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = ag_pack(v[2 * k], v[2 * k + 1]);
      *(u32x4_ag*)(out + t * 8) = o;
    } else {
      out[t] = f2bf(v[0]);
    }
  }
}

static bool ag_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// params [B, 6] int32 and labels_out [B] int64 are written; labels [N] int64
// is read. B comes from params.
void augment_draw(const at::Tensor& labels, at::Tensor& params,
                  at::Tensor& labels_out, uint64_t seed, int64_t step,
                  int64_t rank, int64_t world, int64_t N, int64_t pad,
                  int64_t H, int64_t W, bool augment) {
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong &&
                  labels.is_contiguous() && labels.dim() == 1,
              "augment_draw: labels must be a contiguous 1-d int64 GPU tensor");
  TORCH_CHECK(params.is_cuda() && params.scalar_type() == at::kInt &&
                  params.is_contiguous() && params.dim() == 2 &&
                  params.size(1) == AUG_FIELDS,
              "augment_draw: params must be a contiguous [B, 6] int32 GPU "
              "tensor");
  const int64_t B = params.size(0);
  TORCH_CHECK(labels_out.is_cuda() && labels_out.scalar_type() == at::kLong &&
                  labels_out.is_contiguous() && labels_out.dim() == 1 &&
                  labels_out.size(0) == B,
              "augment_draw: labels_out must be a contiguous [B] int64 GPU "
              "tensor");
  TORCH_CHECK(labels.device() == params.device() &&
                  labels.device() == labels_out.device(),
              "augment_draw: tensors on different devices");
  const int64_t lim = (int64_t)1 << 31;
  TORCH_CHECK(N >= 1 && N < lim && labels.numel() == N,
              "augment_draw: need 1 <= N < 2^31 labels, one per example");
  TORCH_CHECK(pad >= 0 && 2 * pad + 1 < lim, "augment_draw: bad pad");
  TORCH_CHECK(H >= 1 && H < lim && W >= 1 && W < lim,
              "augment_draw: bad image size");
  TORCH_CHECK(step >= 0 && world >= 1 && rank >= 0 && rank < world,
              "augment_draw: need step >= 0 and 0 <= rank < world");
  TORCH_CHECK(B < lim, "augment_draw: batch too large");
  if (B == 0) return;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(augment_draw_kernel, dim3((unsigned)((B + 255) / 256)),
                     dim3(256), 0, stream.stream(),
                     (const int64_t*)labels.data_ptr(),
                     (int*)params.data_ptr(), (int64_t*)labels_out.data_ptr(),
                     seed, (uint64_t)step, (uint64_t)rank, (uint64_t)world, N,
                     B, pad, H, W, augment ? 1 : 0);
  HIP_CHECK_KERNEL();
}

template <typename T>
static void ag_launch(const at::Tensor& data, const at::Tensor& params,
                      const at::Tensor& scale, const at::Tensor& shift,
                      at::Tensor& out, int64_t pad, int64_t cutout_pad) {
  const int64_t N = data.size(0), B = out.size(0);
  const int C = (int)data.size(1), H = (int)data.size(2),
            W = (int)data.size(3);
  bf16_t* o = (bf16_t*)out.data_ptr();
  const bool vec = W % 8 == 0 && ag_al16(o);
  const int per_row = vec ? W / 8 : W;
  const int per_img = C * H * per_row;
  const int64_t total = B * per_img;
  // ~2048 blocks (256 CUs x 8), the rest grid-strided.
  const unsigned grid =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256,
                                                       2048));
  auto stream = at::cuda::getCurrentCUDAStream();
#define AG_APPLY(V)                                                          \
  hipLaunchKernelGGL((augment_apply_kernel<T, V>), dim3(grid), dim3(256), 0, \
                     stream.stream(), (const T*)data.data_ptr(),             \
                     (const int*)params.data_ptr(),                          \
                     (const float*)scale.data_ptr(),                         \
                     (const float*)shift.data_ptr(), o, N, B, C, H, W,       \
                     per_row, per_img, pad, cutout_pad)
  if (vec) AG_APPLY(true); else AG_APPLY(false);
#undef AG_APPLY
  HIP_CHECK_KERNEL();
}

// out[b] = normalise(cutout(flip(crop(data[params[b].index])))) as bf16.
void augment_apply(const at::Tensor& data, const at::Tensor& params,
                   const at::Tensor& scale, const at::Tensor& shift,
                   at::Tensor& out, int64_t pad, int64_t cutout_pad) {
  TORCH_CHECK(data.is_cuda() && data.is_contiguous() && data.dim() == 4 &&
                  (data.scalar_type() == at::kByte ||
                   data.scalar_type() == at::kFloat),
              "augment_apply: data must be a contiguous [N,C,H,W] uint8 or "
              "float32 GPU tensor");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 4 &&
                  out.scalar_type() == at::kBFloat16,
              "augment_apply: out must be a contiguous [B,C,H,W] bf16 GPU "
              "tensor");
  const int64_t N = data.size(0), C = data.size(1), H = data.size(2),
                W = data.size(3), B = out.size(0);
  TORCH_CHECK(out.size(1) == C && out.size(2) == H && out.size(3) == W,
              "augment_apply: out and data disagree on [C,H,W]");
  TORCH_CHECK(params.is_cuda() && params.scalar_type() == at::kInt &&
                  params.is_contiguous() && params.dim() == 2 &&
                  params.size(0) == B && params.size(1) == AUG_FIELDS,
              "augment_apply: params must be a contiguous [B, 6] int32 GPU "
              "tensor");
  for (const at::Tensor* t : {&scale, &shift})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat &&
                    t->is_contiguous() && t->dim() == 1 && t->size(0) == C,
                "augment_apply: scale and shift must be contiguous float32 "
                "GPU tensors of C elements");
  TORCH_CHECK(data.device() == out.device() &&
                  data.device() == params.device() &&
                  data.device() == scale.device() &&
                  data.device() == shift.device(),
              "augment_apply: tensors on different devices");
  const int64_t lim = (int64_t)1 << 31;
  TORCH_CHECK(N >= 1 && N < lim, "augment_apply: need 1 <= N < 2^31");
  TORCH_CHECK(C >= 1 && H >= 1 && W >= 1 && C * H * W < lim,
              "augment_apply: one image must hold fewer than 2^31 elements");
  TORCH_CHECK(pad >= 0 && pad < lim, "augment_apply: need 0 <= pad < 2^31");
  TORCH_CHECK(cutout_pad >= 0 && cutout_pad < lim,
              "augment_apply: need 0 <= cutout_pad < 2^31");
  // 64-bit indexing inside the kernel: both element counts fit with room.
  TORCH_CHECK(B < lim && data.numel() < ((int64_t)1 << 62),
              "augment_apply: tensor too large");
  if (B == 0) return;
  if (data.scalar_type() == at::kByte)
    ag_launch<uint8_t>(data, params, scale, shift, out, pad, cutout_pad);
  else
    ag_launch<float>(data, params, scale, shift, out, pad, cutout_pad);
}
