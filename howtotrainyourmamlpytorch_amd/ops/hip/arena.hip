// Gradient of the arena's per-parameter views in one launch.
//
// ParamArena.views() hands the layers slices arena[:, off_i : off_i + n_i] of
// the [T, P] fast-weight arena.  The gradient of the arena is then the
// per-parameter gradients [T, n_i] written side by side, zero where a
// parameter got none.  Autograd's own backward of the slices builds one
// zero-filled [T, P] tensor per view and adds them up; arena_scatter writes
// the [T, P] result once: every output element is stored exactly once, no
// atomics, no arithmetic (so the values are the inputs' bits).
//
// The parameter table (pointers, offsets, sizes) is passed by value in the
// kernel-arg block, as adam.hip does.  A (t, parameter) segment is copied
// with 16-byte stores wherever its destination allows, with 16-byte loads
// too where the source happens to share the alignment; the arena's offsets
// and P are arbitrary, so every segment has a scalar head and tail.

#include "common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cstdint>

using namespace maml355;

#define ARENA_MAX_PARAMS 32

struct ArenaTable {
  const float* g[ARENA_MAX_PARAMS];  // [T, numel] contiguous, or null
  long offset[ARENA_MAX_PARAMS];
  long numel[ARENA_MAX_PARAMS];
};

typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4_t;

// grid: (x-blocks striding over a segment, parameter, task)
__global__ __launch_bounds__(256)
void arena_scatter_kernel(ArenaTable tab, float* __restrict__ out, long P) {
  const int e = blockIdx.y;
  const long t = blockIdx.z;
  const long n = tab.numel[e];
  float* dst = out + t * P + tab.offset[e];
  const float* src = tab.g[e] ? tab.g[e] + t * n : nullptr;

  // head: scalars up to the first 16-byte boundary of dst
  long head = (long)(((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(float));
  if (head > n) head = n;
  const long nvec = (n - head) / 4;
  const long tail0 = head + nvec * 4;

  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = grid_stride();
  f32x4_t* dv = (f32x4_t*)(dst + head);
  if (src == nullptr) {
    const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
    for (long v = tid; v < nvec; v += stride) dv[v] = z;
  } else if (((uintptr_t)(src + head) & 15) == 0) {
    const f32x4_t* sv = (const f32x4_t*)(src + head);
    for (long v = tid; v < nvec; v += stride) dv[v] = sv[v];
  } else {
    const float* s = src + head;
    for (long v = tid; v < nvec; v += stride) {
      const f32x4_t x = {s[4 * v], s[4 * v + 1], s[4 * v + 2], s[4 * v + 3]};
      dv[v] = x;
    }
  }
  // head and tail elements (at most 3 each), one thread per element
  if (blockIdx.x == 0) {
    const long nedge = head + (n - tail0);
    for (long j = threadIdx.x; j < nedge; j += blockDim.x) {
      const long i = j < head ? j : tail0 + (j - head);
      dst[i] = src ? src[i] : 0.f;
    }
  }
}

// grads[j]: the gradient of parameter slots[j], an fp32 CUDA tensor of
// T * numels[slots[j]] elements; a parameter no entry names has none and
// reads as zero.  offsets / numels must tile [0, P) in order.  Returns
// [T, P] fp32.
torch::Tensor arena_scatter(std::vector<torch::Tensor> grads,
                            std::vector<int64_t> slots,
                            std::vector<int64_t> offsets,
                            std::vector<int64_t> numels, int64_t T, int64_t P) {
  const int n = (int)offsets.size();
  TORCH_CHECK(n > 0 && n <= ARENA_MAX_PARAMS,
              "arena_scatter supports 1..32 parameters, got ", n);
  TORCH_CHECK((int)numels.size() == n && grads.size() == slots.size() &&
              !grads.empty());
  TORCH_CHECK(T >= 1 && T <= 65535 && P >= 1);
  ArenaTable tab;
  std::vector<torch::Tensor> keep;  // contiguous copies stay alive to launch
  long off = 0, max_n = 0;
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(offsets[i] == off && numels[i] >= 1,
                "arena_scatter: parameters must tile the arena in order");
    tab.offset[i] = offsets[i];
    tab.numel[i] = numels[i];
    tab.g[i] = nullptr;
    off += numels[i];
    max_n = std::max<long>(max_n, numels[i]);
  }
  keep.reserve(grads.size());
  for (size_t j = 0; j < grads.size(); ++j) {
    const int64_t i = slots[j];
    const torch::Tensor& g = grads[j];
    TORCH_CHECK(i >= 0 && i < n && tab.g[i] == nullptr,
                "arena_scatter: bad or repeated slot ", i);
    TORCH_CHECK(g.is_cuda() && g.scalar_type() == torch::kFloat32 &&
                    g.numel() == T * numels[i],
                "arena_scatter: gradient of slot ", i, " is not fp32 [T, numel]");
    keep.push_back(g.contiguous());
    tab.g[i] = keep.back().data_ptr<float>();
  }
  TORCH_CHECK(off == P, "arena_scatter: parameters cover ", off, " of ", P);
  auto out = torch::empty({T, P}, grads[0].options());
  const int bx = (int)std::min<long>(std::max<long>((max_n / 4 + 255) / 256, 1), 64);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(arena_scatter_kernel, dim3(bx, n, (unsigned)T), dim3(256),
                     0, stream.stream(), tab, out.data_ptr<float>(), (long)P);
  return out;
}
