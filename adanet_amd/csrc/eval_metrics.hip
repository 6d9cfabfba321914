// Streaming eval metrics (K10): each update kernel folds one batch of logits
// and labels into a persistent fp64 device state, so evaluation needs no
// host sync per batch and is read back once (ops/metrics.py, head.py
// streaming_metrics()).
//
// State layouts (flat fp64):
//   multiclass  [n, loss_sum, correct_1, correct_k, (label_count[C],
//                correct_count[C])]
//   binary      [n, loss_sum, correct, hist[2][T]]   (positives in row 0)
//   regression  [n_elems, sq_err_sum, abs_err_sum]
//
// Accumulation: per-row / per-element values are fp32, every partial after
// that is fp64. The scalar slots never see an atomic: each block overwrites
// the scratch slots it owns (scratch is never pre-zeroed; the grid is a pure
// function of the shape, so a slot is written iff it is summed) and a
// one-wave finisher sums them in fixed order into the state - bit-identical
// from run to run. Histogram and per-class slots hold exact integers, whose
// adds commute, so those use atomics.
//
// Logits are bf16 or fp32 with an explicit row stride (the engine hands the
// narrow view of logits padded to 8).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

namespace {

constexpr int kMaxBlocks = 2048;

__device__ __forceinline__ float ldf(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ float ldf(const float* p) { return *p; }

__device__ __forceinline__ double wave_reduce_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int wave_reduce_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Per-block tail shared by the three kernels: lane 0 of each wave holds that
// wave's N fp64 partials; thread 0 adds them in wave order and overwrites
// the block's scratch slots.
template <int N>
__device__ __forceinline__ void block_store_partials(
    const double (&acc)[N], double* __restrict__ partials) {
  __shared__ double part[4][N];
  const int wave_in_block = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) part[wave_in_block][j] = acc[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nwaves = blockDim.x >> 6;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double s = 0.0;
      for (int w = 0; w < nwaves; ++w) s += part[w][j];
      partials[(int64_t)blockIdx.x * N + j] = s;
    }
  }
}

// One wave per row, as softmax_xent_fwd_kernel, and the same fp32 loss
// arithmetic. rank = #{c : v_c > v_y or (v_c == v_y and c < y)}: rank 0 is
// first-index argmax == y, rank < k is top-k.
template <typename T>
__global__ __launch_bounds__(256) void metrics_multiclass_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ labels, int B,
    int C, int ldl, float eps, int k, double* __restrict__ partials,
    double* __restrict__ per_class) {
  const int wave_in_block = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int waves = (gridDim.x * blockDim.x) >> 6;
  double acc[3] = {0.0, 0.0, 0.0};  // loss, correct_1, correct_k (lane 0)
  for (int row = blockIdx.x * (blockDim.x >> 6) + wave_in_block; row < B;
       row += waves) {
    const T* lrow = logits + (int64_t)row * ldl;
    const int64_t y = labels[row];
    // A label outside [0, C) reads nothing and turns the loss into NaN.
    const bool valid = y >= 0 && y < C;
    const float vy = valid ? ldf(lrow + y) : NAN;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, ldf(lrow + c));
    mx = wave_reduce_max(mx);
    float se = 0.f, sum_logits = 0.f;
    int rank = 0;
    for (int c = lane; c < C; c += 64) {
      const float v = ldf(lrow + c);
      se += __expf(v - mx);
      sum_logits += v;
      rank += (v > vy || (v == vy && c < (int)y)) ? 1 : 0;
    }
    se = wave_reduce_sum(se);
    sum_logits = wave_reduce_sum(sum_logits);
    rank = wave_reduce_sum_i32(rank);
    if (lane == 0) {
      const float lse = __logf(se) + mx;
      const float l = lse - (1.f - eps) * vy - (eps / C) * sum_logits;
      acc[0] += (double)l;
      if (valid) {
        const bool top1 = rank == 0;
        if (top1) acc[1] += 1.0;
        if (rank < k) acc[2] += 1.0;
        if (per_class) {
          atomicAdd(&per_class[y], 1.0);
          if (top1) atomicAdd(&per_class[C + y], 1.0);
        }
      }
    }
  }
  block_store_partials<3>(acc, partials);
}

// Sigmoid cross-entropy, sign-of-logit accuracy and the [2,T] score
// histogram of binary_histogram_kernel (reduce.hip) in one pass.
template <typename T>
__global__ __launch_bounds__(256) void metrics_binary_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ labels, int B,
    int64_t ld, int T_bins, double* __restrict__ partials,
    double* __restrict__ hist) {
  extern __shared__ int lh[];  // [2][T]
  for (int i = threadIdx.x; i < 2 * T_bins; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  double acc[2] = {0.0, 0.0};  // loss, correct
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B;
       i += stride) {
    const float x = ldf(logits + i * ld);
    const bool pos = labels[i] != 0;
    const float l = fmaxf(x, 0.f) - (pos ? x : 0.f) +
                    log1pf(__expf(-fabsf(x)));
    acc[0] += (double)l;
    if ((x > 0.f) == pos) acc[1] += 1.0;
    float s = 1.f / (1.f + expf(-x));
    s = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
    int b = (int)(s * T_bins);
    b = b >= T_bins ? T_bins - 1 : (b < 0 ? 0 : b);  // b < 0: NaN score
    atomicAdd(&lh[(pos ? 0 : 1) * T_bins + b], 1);
  }
  acc[0] = wave_reduce_sum_f64(acc[0]);
  acc[1] = wave_reduce_sum_f64(acc[1]);
  block_store_partials<2>(acc, partials);  // its barrier covers lh too
  for (int i = threadIdx.x; i < 2 * T_bins; i += blockDim.x) {
    if (lh[i]) atomicAdd(&hist[i], (double)lh[i]);
  }
}

// Elementwise squared and absolute error over [B, D].
template <typename T>
__global__ __launch_bounds__(256) void metrics_regression_kernel(
    const T* __restrict__ logits, const float* __restrict__ labels,
    int64_t n, int D, int64_t ldl, double* __restrict__ partials) {
  double acc[2] = {0.0, 0.0};  // sq_err, abs_err
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const int64_t r = i / D;
    const float d = ldf(logits + r * ldl + (i - r * D)) - labels[i];
    acc[0] += (double)(d * d);
    acc[1] += (double)fabsf(d);
  }
  acc[0] = wave_reduce_sum_f64(acc[0]);
  acc[1] = wave_reduce_sum_f64(acc[1]);
  block_store_partials<2>(acc, partials);
}

// One wave: state[1 + j] += sum over blocks of partials[block][j] (lanes
// stride the blocks, fixed xor tree), state[0] += n_add.
__global__ __launch_bounds__(64) void metrics_finish_kernel(
    const double* __restrict__ partials, int nblocks, int nslots,
    double n_add, double* __restrict__ state) {
  for (int j = 0; j < nslots; ++j) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 64)
      s += partials[(int64_t)i * nslots + j];
    s = wave_reduce_sum_f64(s);
    if (threadIdx.x == 0) state[1 + j] += s;
  }
  if (threadIdx.x == 0) state[0] += n_add;
}

void check_common(const char* op, const at::Tensor& state,
                  const at::Tensor& logits, int64_t state_numel) {
  TORCH_CHECK(logits.is_cuda() && state.is_cuda() &&
                  state.device() == logits.device(),
              op, ": state and logits on the same GPU required");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 ||
                  logits.scalar_type() == at::kFloat,
              op, ": bf16 or fp32 logits required");
  TORCH_CHECK(state.scalar_type() == at::kDouble && state.is_contiguous() &&
                  state.numel() == state_numel,
              op, ": contiguous fp64 state of ", state_numel,
              " elements required");
}

void launch_finish(const at::Tensor& scratch, int blocks, int nslots,
                   double n_add, at::Tensor& state, hipStream_t stream) {
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(64), 0, stream,
                     scratch.data_ptr<double>(), blocks, nslots, n_add,
                     state.data_ptr<double>());
  HIP_CHECK_KERNEL();
}

}  // namespace

int64_t metrics_max_blocks() { return kMaxBlocks; }

void metrics_multiclass_update(at::Tensor& state, const at::Tensor& logits,
                               const at::Tensor& labels, int64_t k,
                               double eps, bool per_class) {
  TORCH_CHECK(logits.dim() == 2, "metrics_multiclass: [B, C] logits");
  const int64_t B64 = logits.size(0), C64 = logits.size(1);
  check_common("metrics_multiclass", state, logits,
               4 + (per_class ? 2 * C64 : 0));
  TORCH_CHECK(B64 < (1LL << 31) && C64 >= 1 && C64 < (1LL << 31),
              "metrics_multiclass: B and C must fit int32, C >= 1");
  TORCH_CHECK(B64 == 0 || logits.stride(1) == 1,
              "metrics_multiclass: contiguous class dim");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong &&
                  labels.is_contiguous() && labels.numel() == B64,
              "metrics_multiclass: contiguous int64 GPU labels [B]");
  TORCH_CHECK(k >= 1, "metrics_multiclass: k >= 1");
  const int B = (int)B64, C = (int)C64;
  if (B == 0) return;
  TORCH_CHECK(logits.stride(0) >= 0 && logits.stride(0) < (1LL << 31),
              "metrics_multiclass: row stride must fit int32");
  auto stream = at::cuda::getCurrentCUDAStream();
  const int blocks = std::min((B + 3) / 4, kMaxBlocks);
  auto scratch = at::empty({(int64_t)blocks * 3}, state.options());
  double* pc = per_class ? state.data_ptr<double>() + 4 : nullptr;
  const int kk = (int)std::min<int64_t>(k, C);
  if (logits.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL(metrics_multiclass_kernel<bf16_t>, dim3(blocks),
                       dim3(256), 0, stream.stream(),
                       (const bf16_t*)logits.data_ptr(),
                       labels.data_ptr<int64_t>(), B, C,
                       (int)logits.stride(0), (float)eps, kk,
                       scratch.data_ptr<double>(), pc);
  } else {
    hipLaunchKernelGGL(metrics_multiclass_kernel<float>, dim3(blocks),
                       dim3(256), 0, stream.stream(),
                       logits.data_ptr<float>(), labels.data_ptr<int64_t>(),
                       B, C, (int)logits.stride(0), (float)eps, kk,
                       scratch.data_ptr<double>(), pc);
  }
  HIP_CHECK_KERNEL();
  launch_finish(scratch, blocks, 3, (double)B, state, stream.stream());
}

void metrics_binary_update(at::Tensor& state, const at::Tensor& logits,
                           const at::Tensor& labels, int64_t T) {
  TORCH_CHECK(logits.dim() == 1, "metrics_binary: [B] logits");
  TORCH_CHECK(T >= 1 && T <= 4096, "metrics_binary: 1 <= T <= 4096");
  check_common("metrics_binary", state, logits, 3 + 2 * T);
  const int64_t B64 = logits.size(0);
  TORCH_CHECK(B64 < (1LL << 31), "metrics_binary: B must fit int32");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong &&
                  labels.is_contiguous() && labels.numel() == B64,
              "metrics_binary: contiguous int64 GPU labels [B]");
  const int B = (int)B64;
  if (B == 0) return;
  const int64_t ld = B > 1 ? logits.stride(0) : 1;
  TORCH_CHECK(ld >= 0, "metrics_binary: non-negative stride");
  auto stream = at::cuda::getCurrentCUDAStream();
  const int blocks = std::min((B + 255) / 256, kMaxBlocks);
  auto scratch = at::empty({(int64_t)blocks * 2}, state.options());
  double* hist = state.data_ptr<double>() + 3;
  const size_t lds = 2 * (size_t)T * sizeof(int);
  if (logits.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL(metrics_binary_kernel<bf16_t>, dim3(blocks),
                       dim3(256), lds, stream.stream(),
                       (const bf16_t*)logits.data_ptr(),
                       labels.data_ptr<int64_t>(), B, ld, (int)T,
                       scratch.data_ptr<double>(), hist);
  } else {
    hipLaunchKernelGGL(metrics_binary_kernel<float>, dim3(blocks), dim3(256),
                       lds, stream.stream(), logits.data_ptr<float>(),
                       labels.data_ptr<int64_t>(), B, ld, (int)T,
                       scratch.data_ptr<double>(), hist);
  }
  HIP_CHECK_KERNEL();
  launch_finish(scratch, blocks, 2, (double)B, state, stream.stream());
}

void metrics_regression_update(at::Tensor& state, const at::Tensor& logits,
                               const at::Tensor& labels) {
  TORCH_CHECK(logits.dim() == 2, "metrics_regression: [B, D] logits");
  check_common("metrics_regression", state, logits, 3);
  const int64_t B = logits.size(0), D = logits.size(1);
  TORCH_CHECK(D >= 1 && D < (1LL << 31), "metrics_regression: 1 <= D < 2^31");
  TORCH_CHECK(B == 0 || logits.stride(1) == 1,
              "metrics_regression: contiguous last dim");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kFloat &&
                  labels.is_contiguous() && labels.numel() == B * D,
              "metrics_regression: contiguous fp32 GPU labels [B, D]");
  const int64_t n = B * D;
  if (n == 0) return;
  const int64_t ldl = B > 1 ? logits.stride(0) : D;
  TORCH_CHECK(ldl >= 0, "metrics_regression: non-negative row stride");
  auto stream = at::cuda::getCurrentCUDAStream();
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, kMaxBlocks);
  auto scratch = at::empty({(int64_t)blocks * 2}, state.options());
  if (logits.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL(metrics_regression_kernel<bf16_t>, dim3(blocks),
                       dim3(256), 0, stream.stream(),
                       (const bf16_t*)logits.data_ptr(),
                       labels.data_ptr<float>(), n, (int)D, ldl,
                       scratch.data_ptr<double>());
  } else {
    hipLaunchKernelGGL(metrics_regression_kernel<float>, dim3(blocks),
                       dim3(256), 0, stream.stream(),
                       logits.data_ptr<float>(), labels.data_ptr<float>(), n,
                       (int)D, ldl, scratch.data_ptr<double>());
  }
  HIP_CHECK_KERNEL();
  launch_finish(scratch, blocks, 2, (double)n, state, stream.stream());
}
