// Global average pool over H, W on NHWC bf16 — the op between the last
// strided conv stage and the linear head of the max_pooling=False
// backbone (reference meta_neural_network_architectures.py:609,654-655).
//
//   fwd : y[n, c]       = mean_{h,w} x[n, h, w, c]     fp32 accumulate
//   bwd : dx[n, h, w, c] = dy[n, c] / (H*W)
// The op is linear, so the backward of bwd is fwd applied to the incoming
// grad: custom kernels at every derivative order.
//
// The final maps are tiny (2x2 .. 6x6): a few lanes own one (n, 8-channel
// group), walk the H*W positions serially and combine in a fixed shuffle
// tree — a FIXED summation order, bitwise reproducible, 16-byte loads when
// C % 8 == 0 (one thread per (n, c) otherwise).

#include "common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

using bf16 = __hip_bfloat16;

// GAP_SPLIT adjacent lanes share one (n, 8-channel group): lane s sums the
// positions s, s+GAP_SPLIT, ... and a fixed xor-shuffle tree combines them
// (same order every run).  Whole waves stay in the loop so the shuffles
// always see all their lanes.
#define GAP_SPLIT 4

__global__ void gavgpool_fwd_vec_kernel(const bf16* __restrict__ x,
                                        bf16* __restrict__ y,
                                        long N, int HW, int C) {
  const int cg = C / 8;
  const long total = N * cg * GAP_SPLIT;
  for (long base = (long)blockIdx.x * blockDim.x; base < total;
       base += grid_stride()) {
    const long i = base + threadIdx.x;
    const bool live = i < total;
    const int s = (int)(i % GAP_SPLIT);
    const long e = live ? i / GAP_SPLIT : 0;
    const int g = (int)(e % cg);
    const long n = e / cg;
    const bf16* xp = x + n * HW * (long)C + g * 8;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
#pragma unroll 4
      for (int p = s; p < HW; p += GAP_SPLIT) {
        float v[8];
        load8(xp + (long)p * C, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += v[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[j] += __shfl_xor(acc[j], 1, WAVE);
      acc[j] += __shfl_xor(acc[j], 2, WAVE);
      acc[j] /= (float)HW;
    }
    if (live && s == 0) store8(y + n * C + g * 8, acc);
  }
}

__global__ void gavgpool_fwd_kernel(const bf16* __restrict__ x,
                                    bf16* __restrict__ y,
                                    long N, int HW, int C) {
  const long total = N * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int c = (int)(i % C);
    const long n = i / C;
    const bf16* xp = x + n * HW * (long)C + c;
    float acc = 0.f;
    for (int p = 0; p < HW; ++p) acc += __bfloat162float(xp[(long)p * C]);
    y[i] = __float2bfloat16(acc / (float)HW);
  }
}

__global__ void gavgpool_bwd_vec_kernel(const bf16* __restrict__ dy,
                                        bf16* __restrict__ dx,
                                        long N, int HW, int C) {
  const int cg = C / 8;
  const long total = N * HW * cg;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int g = (int)(i % cg);
    const long n = i / ((long)cg * HW);
    float v[8];
    load8(dy + n * C + g * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] /= (float)HW;
    store8(dx + i * 8, v);
  }
}

__global__ void gavgpool_bwd_kernel(const bf16* __restrict__ dy,
                                    bf16* __restrict__ dx,
                                    long N, int HW, int C) {
  const long total = N * HW * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int c = (int)(i % C);
    const long n = i / ((long)C * HW);
    dx[i] = __float2bfloat16(__bfloat162float(dy[n * C + c]) / (float)HW);
  }
}

// x [N, H, W, C] bf16 contiguous (caller flattens T*NS -> N) -> y [N, C]
torch::Tensor gavgpool_fwd(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "gavgpool_fwd needs bf16");
  const long N = x.size(0);
  const int HW = (int)(x.size(1) * x.size(2)), C = (int)x.size(3);
  TORCH_CHECK(HW >= 1 && C >= 1);
  auto y = torch::empty({N, C}, x.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  if (C % 8 == 0) {
    hipLaunchKernelGGL(gavgpool_fwd_vec_kernel,
                       dim3(ew_grid(N * (C / 8) * GAP_SPLIT, 256)), dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       reinterpret_cast<bf16*>(y.data_ptr()), N, HW, C);
  } else {
    hipLaunchKernelGGL(gavgpool_fwd_kernel, dim3(ew_grid(N * C, 256)),
                       dim3(256), 0, stream.stream(),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       reinterpret_cast<bf16*>(y.data_ptr()), N, HW, C);
  }
  return y;
}

// dy [N, C] bf16 -> dx [N, H, W, C] = dy / (H*W)
torch::Tensor gavgpool_bwd(torch::Tensor dy, long H, long W) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 2 && H >= 1 && W >= 1);
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16, "gavgpool_bwd needs bf16");
  auto dyc = dy.contiguous();
  const long N = dy.size(0);
  const int C = (int)dy.size(1), HW = (int)(H * W);
  auto dx = torch::empty({N, H, W, C}, dy.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  if (C % 8 == 0) {
    hipLaunchKernelGGL(gavgpool_bwd_vec_kernel,
                       dim3(ew_grid(N * HW * (C / 8), 256)), dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const bf16*>(dyc.data_ptr()),
                       reinterpret_cast<bf16*>(dx.data_ptr()), N, HW, C);
  } else {
    hipLaunchKernelGGL(gavgpool_bwd_kernel, dim3(ew_grid(N * HW * C, 256)),
                       dim3(256), 0, stream.stream(),
                       reinterpret_cast<const bf16*>(dyc.data_ptr()),
                       reinterpret_cast<bf16*>(dx.data_ptr()), N, HW, C);
  }
  return dx;
}
