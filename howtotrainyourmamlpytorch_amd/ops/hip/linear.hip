// Task-batched linear head (reference: F.linear via
// meta_neural_network_architectures.py:141) — the LAST library op on the
// training path.  torch.bmm routes to hipBLASLt, whose first-call
// autotuning made run #1 of a process numerically different from runs
// #2+ (measured: identical 5e-3 theta drift after 3 Adam steps, gone on
// CPU).  These kernels are pure functions of their inputs: deterministic
// across calls, processes and allocator states.
//
// Math (per task):  y = x @ w^T + b     x [M,K] bf16, w [ways,K] fp32
//   dx = dy @ w        dw = dy^T @ x        db = sum_m dy
// The three ops are mutually bilinear, so each backward composes the
// other two — custom kernels at every derivative order (second-order
// MAML included), mirroring the conv trio.
// w/b are read in fp32 and ROUNDED to bf16 in-kernel — numerically
// identical to the previous bmm-on-bf16-cast path, with fp32 dw/db out.
// The kernels are templated on the activation type AT: with fp32
// activations (--compute_dtype fp32, --fp32_support_pass) w/b are used
// UNROUNDED and every output is fp32, in the same fixed reduction orders.
// Shapes are tiny (M <= ~500, ways <= 64, K <= ~3200): VALU kernels.

#include "common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

using bf16 = __hip_bfloat16;

DEVINL float rb(float v) {  // round fp32 -> bf16 -> fp32
  return __bfloat162float(__float2bfloat16(v));
}
DEVINL float ld_bf(const short* p) {
  return __bfloat162float(__hip_bfloat16(__hip_bfloat16_raw{(unsigned short)*p}));
}

// Per-activation-type element access: the storage type, the load to fp32,
// the rounding applied to the fp32 weights/bias and the output store.
template <typename AT> struct Act;
template <> struct Act<bf16> {
  using raw = short;
  static DEVINL float ld(const raw* p) { return ld_bf(p); }
  static DEVINL float wr(float v) { return rb(v); }
  static DEVINL void st(raw* p, float v) {
    *p = (short)__bfloat16_as_short(__float2bfloat16(v));
  }
};
template <> struct Act<float> {
  using raw = float;
  static DEVINL float ld(const raw* p) { return *p; }
  static DEVINL float wr(float v) { return v; }
  static DEVINL void st(raw* p, float v) { *p = v; }
};

// y[t,m,w] = sum_k x[t,m,k] * bf16(w[t,w,k]) + bf16(b[t,w]); one wave per
// (t, m) row, lanes k-parallel with a wave reduction per way.
template <typename AT>
__global__ void lin_fwd_kernel(const AT* __restrict__ X,
                               const float* __restrict__ W,
                               const float* __restrict__ B,
                               AT* __restrict__ Y,
                               int T, int M, int K, int ways) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long rows = (long)T * M;
  const long wave_id = ((long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const long nwaves = grid_stride() / WAVE;
  for (long row = wave_id; row < rows; row += nwaves) {
    const long t = row / M;
    using A = Act<AT>;
    const typename A::raw* xr = (const typename A::raw*)X + row * K;
    for (int w = 0; w < ways; ++w) {
      const float* wr = W + (t * ways + w) * (long)K;
      float acc = 0.f;
      for (int k = lane; k < K; k += WAVE) {
        acc = fmaf(A::ld(xr + k), A::wr(wr[k]), acc);
      }
      acc = wave_reduce_sum(acc);
      if (lane == 0) {
        if (B) acc += A::wr(B[t * ways + w]);
        A::st((typename A::raw*)Y + row * ways + w, acc);
      }
    }
  }
}

// dx[t,m,k] = sum_w dy[t,m,w] * bf16(W[t,w,k]); thread per element.
template <typename AT>
__global__ void lin_dx_kernel(const AT* __restrict__ dY,
                              const float* __restrict__ W,
                              AT* __restrict__ dX,
                              int T, int M, int K, int ways) {
  const long total = (long)T * M * K;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int k = (int)(i % K);
    const long row = i / K;
    const long t = row / M;
    using A = Act<AT>;
    const typename A::raw* dyr = (const typename A::raw*)dY + row * ways;
    float acc = 0.f;
    for (int w = 0; w < ways; ++w) {
      acc = fmaf(A::ld(dyr + w), A::wr(W[(t * ways + w) * (long)K + k]), acc);
    }
    A::st((typename A::raw*)dX + i, acc);
  }
}

// dw[t,w,k] = sum_m dy[t,m,w] * x[t,m,k] (fp32 out, fixed m order ->
// deterministic); thread per element with a serial m loop.
template <typename AT>
__global__ void lin_wgrad_kernel(const AT* __restrict__ dY,
                                 const AT* __restrict__ X,
                                 float* __restrict__ dW,
                                 int T, int M, int K, int ways) {
  const long total = (long)T * ways * K;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int k = (int)(i % K);
    const int w = (int)((i / K) % ways);
    const long t = i / ((long)K * ways);
    using A = Act<AT>;
    const typename A::raw* dyt = (const typename A::raw*)dY + t * (long)M * ways + w;
    const typename A::raw* xt = (const typename A::raw*)X + t * (long)M * K + k;
    float acc = 0.f;
    for (int m = 0; m < M; ++m) {
      acc = fmaf(A::ld(dyt + (long)m * ways), A::ld(xt + (long)m * K), acc);
    }
    dW[i] = acc;
  }
}

// db[t,w] = sum_m dy[t,m,w] (fp32, fixed order)
template <typename AT>
__global__ void lin_db_kernel(const AT* __restrict__ dY,
                              float* __restrict__ dB,
                              int T, int M, int ways) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * ways) return;
  const int w = i % ways;
  const long t = i / ways;
  using A = Act<AT>;
  const typename A::raw* dyt = (const typename A::raw*)dY + t * (long)M * ways + w;
  float acc = 0.f;
  for (int m = 0; m < M; ++m) acc += A::ld(dyt + (long)m * ways);
  dB[i] = acc;
}

static bool lin_is_f32(const torch::Tensor& a, const char* what) {
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 ||
                  a.scalar_type() == torch::kFloat32,
              what, ": activations must be bf16 or fp32");
  return a.scalar_type() == torch::kFloat32;
}

torch::Tensor lin_fwd(torch::Tensor x, torch::Tensor w,
                      c10::optional<torch::Tensor> b) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3);
  const bool f32 = lin_is_f32(x, "lin_fwd");
  auto xc = x.contiguous();
  auto wc = w.contiguous().to(torch::kFloat32);
  const int T = (int)x.size(0), M = (int)x.size(1), K = (int)x.size(2);
  const int ways = (int)w.size(1);
  TORCH_CHECK(w.size(0) == T && w.size(2) == K);
  auto y = torch::empty({T, M, ways}, x.options());
  const float* bptr = nullptr;
  torch::Tensor bc;
  if (b.has_value()) {
    bc = b->contiguous().to(torch::kFloat32);
    bptr = bc.data_ptr<float>();
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid(ew_grid((long)T * M * WAVE, 256));
  if (f32) {
    hipLaunchKernelGGL(lin_fwd_kernel<float>, grid, dim3(256), 0,
                       stream.stream(), xc.data_ptr<float>(),
                       wc.data_ptr<float>(), bptr, y.data_ptr<float>(),
                       T, M, K, ways);
  } else {
    hipLaunchKernelGGL(lin_fwd_kernel<bf16>, grid, dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const bf16*>(xc.data_ptr()),
                       wc.data_ptr<float>(), bptr,
                       reinterpret_cast<bf16*>(y.data_ptr()), T, M, K, ways);
  }
  return y;
}

torch::Tensor lin_dx(torch::Tensor dy, torch::Tensor w) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 3);
  const bool f32 = lin_is_f32(dy, "lin_dx");
  auto dyc = dy.contiguous();
  auto wc = w.contiguous().to(torch::kFloat32);
  const int T = (int)dy.size(0), M = (int)dy.size(1), ways = (int)dy.size(2);
  const int K = (int)w.size(2);
  auto dx = torch::empty({T, M, K}, dy.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid(ew_grid((long)T * M * K, 256));
  if (f32) {
    hipLaunchKernelGGL(lin_dx_kernel<float>, grid, dim3(256), 0,
                       stream.stream(), dyc.data_ptr<float>(),
                       wc.data_ptr<float>(), dx.data_ptr<float>(),
                       T, M, K, ways);
  } else {
    hipLaunchKernelGGL(lin_dx_kernel<bf16>, grid, dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const bf16*>(dyc.data_ptr()),
                       wc.data_ptr<float>(),
                       reinterpret_cast<bf16*>(dx.data_ptr()), T, M, K, ways);
  }
  return dx;
}

std::vector<torch::Tensor> lin_wgrad(torch::Tensor dy, torch::Tensor x,
                                     bool with_bias) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && dy.dim() == 3 && x.dim() == 3);
  const bool f32 = lin_is_f32(dy, "lin_wgrad");
  TORCH_CHECK(x.scalar_type() == dy.scalar_type(),
              "lin_wgrad: dy and x must share a dtype");
  auto dyc = dy.contiguous();
  auto xc = x.contiguous();
  const int T = (int)dy.size(0), M = (int)dy.size(1), ways = (int)dy.size(2);
  const int K = (int)x.size(2);
  auto dw = torch::empty({T, ways, K}, x.options().dtype(torch::kFloat32));
  auto db = torch::empty({T, ways}, x.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid(ew_grid((long)T * ways * K, 256));
  const dim3 bgrid((T * ways + 255) / 256);
  if (f32) {
    hipLaunchKernelGGL(lin_wgrad_kernel<float>, grid, dim3(256), 0,
                       stream.stream(), dyc.data_ptr<float>(),
                       xc.data_ptr<float>(), dw.data_ptr<float>(),
                       T, M, K, ways);
    if (with_bias) {
      hipLaunchKernelGGL(lin_db_kernel<float>, bgrid, dim3(256), 0,
                         stream.stream(), dyc.data_ptr<float>(),
                         db.data_ptr<float>(), T, M, ways);
    }
  } else {
    hipLaunchKernelGGL(lin_wgrad_kernel<bf16>, grid, dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const bf16*>(dyc.data_ptr()),
                       reinterpret_cast<const bf16*>(xc.data_ptr()),
                       dw.data_ptr<float>(), T, M, K, ways);
    if (with_bias) {
      hipLaunchKernelGGL(lin_db_kernel<bf16>, bgrid, dim3(256), 0,
                         stream.stream(),
                         reinterpret_cast<const bf16*>(dyc.data_ptr()),
                         db.data_ptr<float>(), T, M, ways);
    }
  }
  return {dw, db};
}
