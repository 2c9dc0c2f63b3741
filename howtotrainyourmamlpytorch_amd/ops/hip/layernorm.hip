// Fused task-batched LayerNorm (over the whole H*W*C image) + elementwise
// learnable bias + leaky-ReLU, with its first backward and the analytic
// backward of that backward, for x[T, NS, D] (D = H*W*C, contiguous per
// image).
//
// Replaces the reference's F.layer_norm + F.leaky_relu pair
// (meta_neural_network_architectures.py:261-322, :383): weight frozen at
// 1, bias of the full feature shape — [D] when it is a meta-only
// parameter, [T, D] when it is an inner-loop fast weight.
//
// Notation per image, means <.> over the D elements:
//   r = rstd, xh = (x - mu) * r, pre = xh + b, s = pre > 0 ? 1 : slope
//   forward:         y = act ? lrelu(pre) : pre
//   first backward:  u = dy * s, m1 = <u>, m2 = <u * xh>
//                    dx = r * (u - m1 - xh * m2)
//                    dbias_t[t, d] = sum_n u[t, n, d]      (ascending n)
//   second backward, cotangents gx of dx and gb of dbias_t:
//                    a = <gx>, q = <gx * xh>, c = <gx * u>
//                    d_u = r * (gx - a - xh * q) + gb[t],  d_dy = d_u * s
//                    d_x = r^2 * ( -xh * (c - a*m1 - 3*q*m2)
//                                  - m2 * (gx - a) - q * (u - m1) )
// (the leaky-ReLU side is treated as constant — a.e. exact, as in
// bn_dbwd.hip; the bias therefore gets no gradient from the second
// backward.)
//
// The reduction runs along contiguous memory, so one workgroup owns one
// image: it sums, finishes the statistics and applies them while the image
// is L2-hot — one launch.  Few large images (the support pass's first
// stages) would leave most CUs idle, so from kSplitMinD elements on an
// image is split over S workgroups: a sums kernel writes one private
// partials slice per chunk (NO atomics) and every chunk of the apply kernel
// adds the S slices in ascending order.  Every reduction has a fixed
// order: per-thread strided sum -> wave shuffle tree -> waves in ascending
// order -> chunks in ascending order; the result is bitwise run-to-run
// deterministic.
//
// The forward variance uses sums shifted by the image's first element K:
// var = <(x-K)^2> - <x-K>^2.  K is a sample of the data, so |mu - K| is of
// the order of the image's own spread and nothing cancels, whatever the
// mean (a bare E[x^2] - mean^2 loses (mean/std)^2 of fp32's precision).

#include "common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;
using bf16 = __hip_bfloat16;

namespace {

constexpr int LN_FWD = 0, LN_BWD = 1, LN_DBWD = 2;
constexpr int kLnThreads = 256;
constexpr int kLnWaves = kLnThreads / WAVE;
constexpr int kLnMaxBlocks = 2048;     // capped grid; work items stride it
constexpr int kSplitMinD = 32768;      // smallest D that is split
constexpr int kSplitChunk = 16384;     // smallest chunk of a split image
constexpr int kSplitMaxS = 64;
constexpr int kSplitBlocks = 1024;     // split only up to this many blocks

__host__ __device__ constexpr int ln_nsums(int mode) {
  return mode == LN_DBWD ? 5 : 2;
}

template <typename scalar_t>
struct LnParams {
  const scalar_t* x;
  const scalar_t* dy;     // bwd, dbwd
  const scalar_t* gx;     // dbwd
  scalar_t* o0;           // fwd: y      bwd: dx      dbwd: d_dy
  scalar_t* o1;           //                          dbwd: d_x
  const float* bias;      // [D] or [T, D]
  const float* gb;        // dbwd: [T, D]
  float* mean;            // [NIMG]  fwd writes, bwd/dbwd read
  float* rstd;            // [NIMG]
  float* partials;        // split only: [NIMG, S, nsums]
  long nimg;
  int NS, D, S, chunk;
  float eps, slope;
  int vec_ok;             // all activation pointers 16-byte aligned
};

// [lo, hi) of one image as  scalar head [lo, a0) | 8-wide body [a0, a1) |
// scalar tail [a1, hi), the body starting at the first element whose
// address is a multiple of 8 elements (an image base is img * D, any
// residue when D % 8 != 0).
struct LnRange {
  int lo, a0, a1, hi;
};

DEVINL LnRange ln_range(long base, int lo, int hi, int vec_ok) {
  LnRange g;
  g.lo = lo;
  g.hi = hi;
  int a0 = hi;
  if (vec_ok) {
    const int mis = (int)((base + lo) & 7);
    a0 = min(hi, lo + ((8 - mis) & 7));
  }
  g.a0 = a0;
  g.a1 = a0 + ((hi - a0) & ~7);
  return g;
}

template <typename scalar_t, int N>
DEVINL void ln_load(const scalar_t* p, float* v) {
  if constexpr (N == 8) load8(p, v);
  else v[0] = to_f32(*p);
}

template <typename scalar_t, int N>
DEVINL void ln_store(scalar_t* p, const float* v) {
  if constexpr (N == 8) store8(p, v);
  else *p = from_f32<scalar_t>(v[0]);
}

template <int N>
DEVINL float ln_sum(const float* v) {
  if constexpr (N == 8)
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  else
    return v[0];
}

// The per-image constants of one work item.  c0 is the forward's shift K
// in the sums and the mean afterwards.
struct LnStats {
  float c0, r;                 // K or mu, rstd
  float m1, m2, a, q, cc;      // bwd / dbwd means; cc = c - a*m1 - 3*q*m2
};

// N elements at image offset d into the sums acc[nsums]
template <typename scalar_t, int MODE, bool ACT, int N>
DEVINL void ln_accum(const LnParams<scalar_t>& p, long gi, const float* bptr,
                     const LnStats& st, float* acc) {
  float xv[N];
  ln_load<scalar_t, N>(p.x + gi, xv);
  if constexpr (MODE == LN_FWD) {
    float sq[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      xv[j] -= st.c0;
      sq[j] = xv[j] * xv[j];
    }
    acc[0] += ln_sum<N>(xv);
    acc[1] += ln_sum<N>(sq);
  } else {
    float uv[N], t1[N];
    ln_load<scalar_t, N>(p.dy + gi, uv);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      xv[j] = (xv[j] - st.c0) * st.r;                       // xh
      if (ACT) uv[j] *= ((xv[j] + bptr[j]) > 0.f) ? 1.f : p.slope;
      t1[j] = uv[j] * xv[j];
    }
    acc[0] += ln_sum<N>(uv);
    acc[1] += ln_sum<N>(t1);
    if constexpr (MODE == LN_DBWD) {
      float gv[N], t2[N];
      ln_load<scalar_t, N>(p.gx + gi, gv);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        t1[j] = gv[j] * xv[j];
        t2[j] = gv[j] * uv[j];
      }
      acc[2] += ln_sum<N>(gv);
      acc[3] += ln_sum<N>(t1);
      acc[4] += ln_sum<N>(t2);
    }
  }
}

// N output elements at image offset d
template <typename scalar_t, int MODE, bool ACT, int N>
DEVINL void ln_apply(const LnParams<scalar_t>& p, long gi, const float* bptr,
                     const float* gbptr, const LnStats& st) {
  float xv[N];
  ln_load<scalar_t, N>(p.x + gi, xv);
  if constexpr (MODE == LN_FWD) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float o = (xv[j] - st.c0) * st.r + bptr[j];
      if (ACT) o = o > 0.f ? o : o * p.slope;
      xv[j] = o;
    }
    ln_store<scalar_t, N>(p.o0 + gi, xv);
  } else {
    float uv[N], sv[N];
    ln_load<scalar_t, N>(p.dy + gi, uv);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      xv[j] = (xv[j] - st.c0) * st.r;                       // xh
      sv[j] = 1.f;
      if (ACT) sv[j] = ((xv[j] + bptr[j]) > 0.f) ? 1.f : p.slope;
      uv[j] *= sv[j];
    }
    if constexpr (MODE == LN_BWD) {
#pragma unroll
      for (int j = 0; j < N; ++j)
        uv[j] = st.r * (uv[j] - st.m1 - xv[j] * st.m2);
      ln_store<scalar_t, N>(p.o0 + gi, uv);
    } else {
      float gv[N];
      ln_load<scalar_t, N>(p.gx + gi, gv);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float gc = gv[j] - st.a;
        const float du = st.r * (gc - xv[j] * st.q) + gbptr[j];
        const float dxv = st.r * st.r *
                          (-xv[j] * st.cc - st.m2 * gc -
                           st.q * (uv[j] - st.m1));
        gv[j] = du * sv[j];
        uv[j] = dxv;
      }
      ln_store<scalar_t, N>(p.o0 + gi, gv);
      ln_store<scalar_t, N>(p.o1 + gi, uv);
    }
  }
}

// this block's strided share of [lo, hi) of image img into acc
template <typename scalar_t, int MODE, bool PER_TASK, bool ACT>
DEVINL void ln_accum_range(const LnParams<scalar_t>& p, long img, int lo,
                           int hi, const LnStats& st, float* acc) {
  const long base = img * p.D;
  const float* bias = p.bias + (PER_TASK ? (img / p.NS) * (long)p.D : 0);
  const LnRange g = ln_range(base, lo, hi, p.vec_ok);
  for (int d = g.a0 + (int)threadIdx.x * 8; d < g.a1; d += kLnThreads * 8)
    ln_accum<scalar_t, MODE, ACT, 8>(p, base + d, bias + d, st, acc);
  const int nhead = g.a0 - g.lo, nsc = nhead + (g.hi - g.a1);
  for (int e = threadIdx.x; e < nsc; e += kLnThreads) {
    const int d = e < nhead ? g.lo + e : g.a1 + (e - nhead);
    ln_accum<scalar_t, MODE, ACT, 1>(p, base + d, bias + d, st, acc);
  }
}

template <typename scalar_t, int MODE, bool PER_TASK, bool ACT>
DEVINL void ln_apply_range(const LnParams<scalar_t>& p, long img, int lo,
                           int hi, const LnStats& st) {
  const long base = img * p.D;
  const long toff = (img / p.NS) * (long)p.D;
  const float* bias = p.bias + (PER_TASK ? toff : 0);
  const float* gb = MODE == LN_DBWD ? p.gb + toff : bias;
  const LnRange g = ln_range(base, lo, hi, p.vec_ok);
  for (int d = g.a0 + (int)threadIdx.x * 8; d < g.a1; d += kLnThreads * 8)
    ln_apply<scalar_t, MODE, ACT, 8>(p, base + d, bias + d, gb + d, st);
  const int nhead = g.a0 - g.lo, nsc = nhead + (g.hi - g.a1);
  for (int e = threadIdx.x; e < nsc; e += kLnThreads) {
    const int d = e < nhead ? g.lo + e : g.a1 + (e - nhead);
    ln_apply<scalar_t, MODE, ACT, 1>(p, base + d, bias + d, gb + d, st);
  }
}

// Block-wide sums of acc[NSUM], the total left in acc of EVERY thread:
// shuffle tree inside a wave, then the waves in ascending order.
template <int NSUM>
DEVINL void ln_block_sums(float* acc, float (*red)[kLnWaves]) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  __syncthreads();                       // red free again (previous item)
#pragma unroll
  for (int k = 0; k < NSUM; ++k) {
    const float v = wave_reduce_sum(acc[k]);
    if (lane == 0) red[k][wid] = v;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NSUM; ++k) {
    float s = red[k][0];
#pragma unroll
    for (int w = 1; w < kLnWaves; ++w) s += red[k][w];
    acc[k] = s;
  }
}

template <typename scalar_t, int MODE>
DEVINL void ln_item_begin(const LnParams<scalar_t>& p, long img, LnStats& st) {
  if constexpr (MODE == LN_FWD) {
    st.c0 = to_f32(p.x[img * p.D]);      // the shift K
    st.r = 1.f;
  } else {
    st.c0 = p.mean[img];
    st.r = p.rstd[img];
  }
}

// split images only: the sums of one chunk into its private partials slice
template <typename scalar_t, int MODE, bool PER_TASK, bool ACT>
__global__ __launch_bounds__(kLnThreads) void ln_sums_kernel(
    LnParams<scalar_t> p) {
  constexpr int NSUM = ln_nsums(MODE);
  __shared__ float red[NSUM][kLnWaves];
  const long work = p.nimg * p.S;
  for (long w = blockIdx.x; w < work; w += gridDim.x) {
    const long img = w / p.S;
    const int lo = (int)(w % p.S) * p.chunk;
    const int hi = min(lo + p.chunk, p.D);
    LnStats st;
    ln_item_begin<scalar_t, MODE>(p, img, st);
    float acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.f;
    ln_accum_range<scalar_t, MODE, PER_TASK, ACT>(p, img, lo, hi, st, acc);
    ln_block_sums<NSUM>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < NSUM; ++k) p.partials[w * NSUM + k] = acc[k];
    }
  }
}

// One work item = one chunk of one image (the whole image when S == 1):
// total sums (own reduction, or the S partial slices in ascending order),
// statistics, then the elementwise pass over the chunk.
template <typename scalar_t, int MODE, bool PER_TASK, bool ACT, bool SPLIT>
__global__ __launch_bounds__(kLnThreads) void ln_main_kernel(
    LnParams<scalar_t> p) {
  constexpr int NSUM = ln_nsums(MODE);
  __shared__ float red[NSUM][kLnWaves];
  const long work = p.nimg * p.S;
  const float invD = 1.f / (float)p.D;
  for (long w = blockIdx.x; w < work; w += gridDim.x) {
    const long img = w / p.S;
    const int ck = (int)(w % p.S);
    const int lo = ck * p.chunk;
    const int hi = min(lo + p.chunk, p.D);
    LnStats st;
    ln_item_begin<scalar_t, MODE>(p, img, st);
    float acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.f;
    if (SPLIT) {
      const float* pt = p.partials + img * p.S * NSUM;
      for (int s = 0; s < p.S; ++s) {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) acc[k] += pt[s * NSUM + k];
      }
    } else {
      ln_accum_range<scalar_t, MODE, PER_TASK, ACT>(p, img, 0, p.D, st, acc);
      ln_block_sums<NSUM>(acc, red);
    }
    if constexpr (MODE == LN_FWD) {
      const float m = acc[0] * invD;
      const float var = fmaxf(acc[1] * invD - m * m, 0.f);
      st.c0 += m;
      st.r = rsqrtf(var + p.eps);
      if (ck == 0 && threadIdx.x == 0) {
        p.mean[img] = st.c0;
        p.rstd[img] = st.r;
      }
    } else {
      st.m1 = acc[0] * invD;
      st.m2 = acc[1] * invD;
      if constexpr (MODE == LN_DBWD) {
        st.a = acc[2] * invD;
        st.q = acc[3] * invD;
        st.cc = acc[4] * invD - st.a * st.m1 - 3.f * st.q * st.m2;
      }
    }
    ln_apply_range<scalar_t, MODE, PER_TASK, ACT>(p, img, lo, hi, st);
  }
}

// dbias_t[t, d] = sum_n dy[t, n, d] * s[t, n, d], ascending n.  One thread
// per N consecutive d of one task; N = 8 needs D % 8 == 0 (every image
// base aligned), otherwise N = 1.
template <typename scalar_t, bool PER_TASK, bool ACT, int N>
__global__ void ln_dbias_kernel(const scalar_t* __restrict__ dy,
                                const scalar_t* __restrict__ x,
                                const float* __restrict__ mean,
                                const float* __restrict__ rstd,
                                const float* __restrict__ bias,
                                float* __restrict__ dbias,  // [T, D]
                                int T, int NS, int D, float slope) {
  const int groups = D / N;
  const long total = (long)T * groups;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int t = (int)(i / groups);
    const int d = (int)(i % groups) * N;
    const float* bptr = bias + (PER_TASK ? (long)t * D : 0) + d;
    float acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    for (int n = 0; n < NS; ++n) {
      const long img = (long)t * NS + n;
      const long gi = img * D + d;
      float uv[N];
      ln_load<scalar_t, N>(dy + gi, uv);
      if (ACT) {
        const float mu = mean[img], r = rstd[img];
        float xv[N];
        ln_load<scalar_t, N>(x + gi, xv);
#pragma unroll
        for (int j = 0; j < N; ++j)
          uv[j] *= (((xv[j] - mu) * r + bptr[j]) > 0.f) ? 1.f : slope;
      }
#pragma unroll
      for (int j = 0; j < N; ++j) acc[j] += uv[j];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) dbias[(long)t * D + d + j] = acc[j];
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
struct LnGeom {
  int T, NS, D, S, chunk;
  long nimg;
};

// S and chunk are functions of the shape alone (determinism).
LnGeom ln_geom(const torch::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.dim() >= 3 && x.is_contiguous(),
              "layernorm: x must be a contiguous GPU tensor [T, NS, ...]");
  LnGeom g;
  g.T = (int)x.size(0);
  g.NS = (int)x.size(1);
  g.nimg = (long)g.T * g.NS;
  TORCH_CHECK(g.nimg > 0 && x.numel() > 0, "layernorm: empty input");
  const long D = x.numel() / g.nimg;
  TORCH_CHECK(D < (1L << 30), "layernorm: image too large");
  g.D = (int)D;
  int S = 1;
  if (g.D >= kSplitMinD && g.nimg < kSplitBlocks) {
    S = std::min<long>(std::min<long>(g.D / kSplitChunk,
                                      kSplitBlocks / g.nimg), kSplitMaxS);
    S = std::max(S, 1);
  }
  g.chunk = (((g.D + S - 1) / S) + 7) & ~7;
  g.S = (g.D + g.chunk - 1) / g.chunk;
  return g;
}

bool ln_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs)
    if (q != nullptr && (reinterpret_cast<uintptr_t>(q) & 15) != 0) return false;
  return true;
}

void ln_check_bias(const torch::Tensor& b, const LnGeom& g, const char* what) {
  TORCH_CHECK(b.is_cuda() && b.scalar_type() == torch::kFloat32 &&
                  b.is_contiguous() &&
                  ((b.dim() == 1 && b.size(0) == g.D) ||
                   (b.dim() == 2 && b.size(0) == g.T && b.size(1) == g.D)),
              "layernorm: ", what, " must be fp32 [D] or [T, D]");
}

template <typename scalar_t, int MODE>
void ln_launch(LnParams<scalar_t>& p, const LnGeom& g, bool per_task, bool act,
               const torch::Tensor& like) {
  auto stream = at::cuda::getCurrentCUDAStream();
  p.nimg = g.nimg;
  p.NS = g.NS;
  p.D = g.D;
  p.S = g.S;
  p.chunk = g.chunk;
  const bool split = g.S > 1;
  torch::Tensor partials;
  if (split) {
    partials = torch::empty({g.nimg, (long)g.S, (long)ln_nsums(MODE)},
                            like.options().dtype(torch::kFloat32));
    p.partials = partials.data_ptr<float>();
  } else {
    p.partials = nullptr;
  }
  const dim3 grid((unsigned)std::min<long>(g.nimg * g.S, kLnMaxBlocks));
  const dim3 block(kLnThreads);
#define LN_GO(PT, ACT_)                                                        \
  do {                                                                         \
    if (split) {                                                               \
      hipLaunchKernelGGL((ln_sums_kernel<scalar_t, MODE, PT, ACT_>), grid,     \
                         block, 0, stream.stream(), p);                        \
      hipLaunchKernelGGL((ln_main_kernel<scalar_t, MODE, PT, ACT_, true>),     \
                         grid, block, 0, stream.stream(), p);                  \
    } else {                                                                   \
      hipLaunchKernelGGL((ln_main_kernel<scalar_t, MODE, PT, ACT_, false>),    \
                         grid, block, 0, stream.stream(), p);                  \
    }                                                                          \
  } while (0)
  if (per_task) { if (act) LN_GO(true, true); else LN_GO(true, false); }
  else { if (act) LN_GO(false, true); else LN_GO(false, false); }
#undef LN_GO
}

template <typename scalar_t>
void ln_dbias_launch(const torch::Tensor& dy, const torch::Tensor& x,
                     const torch::Tensor& mean, const torch::Tensor& rstd,
                     const torch::Tensor& bias, torch::Tensor& dbias,
                     const LnGeom& g, double slope, bool act, bool vec) {
  auto stream = at::cuda::getCurrentCUDAStream();
  const bool per_task = bias.dim() == 2;
  const long total = (long)g.T * (vec ? g.D / 8 : g.D);
  const dim3 grid((unsigned)std::min<long>((total + 255) / 256, 4096));
#define LN_DB(PT, ACT_, N_)                                                    \
  hipLaunchKernelGGL((ln_dbias_kernel<scalar_t, PT, ACT_, N_>), grid,          \
                     dim3(256), 0, stream.stream(),                            \
                     reinterpret_cast<const scalar_t*>(dy.data_ptr()),         \
                     reinterpret_cast<const scalar_t*>(x.data_ptr()),          \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),           \
                     bias.data_ptr<float>(), dbias.data_ptr<float>(),          \
                     g.T, g.NS, g.D, (float)slope)
#define LN_DB2(PT, ACT_)                                                       \
  do { if (vec) LN_DB(PT, ACT_, 8); else LN_DB(PT, ACT_, 1); } while (0)
  if (per_task) { if (act) LN_DB2(true, true); else LN_DB2(true, false); }
  else { if (act) LN_DB2(false, true); else LN_DB2(false, false); }
#undef LN_DB2
#undef LN_DB
}

template <typename scalar_t>
std::vector<torch::Tensor> ln_fwd_impl(const torch::Tensor& x,
                                       const torch::Tensor& bias, double eps,
                                       double slope, bool act,
                                       const LnGeom& g) {
  auto fopts = x.options().dtype(torch::kFloat32);
  auto y = torch::empty_like(x);
  auto mean = torch::empty({g.T, g.NS}, fopts);
  auto rstd = torch::empty({g.T, g.NS}, fopts);
  LnParams<scalar_t> p{};
  p.x = reinterpret_cast<const scalar_t*>(x.data_ptr());
  p.o0 = reinterpret_cast<scalar_t*>(y.data_ptr());
  p.bias = bias.data_ptr<float>();
  p.mean = mean.data_ptr<float>();
  p.rstd = rstd.data_ptr<float>();
  p.eps = (float)eps;
  p.slope = (float)slope;
  p.vec_ok = ln_aligned({p.x, p.o0});
  ln_launch<scalar_t, LN_FWD>(p, g, bias.dim() == 2, act, x);
  return {y, mean, rstd};
}

template <typename scalar_t>
std::vector<torch::Tensor> ln_bwd_impl(const torch::Tensor& dy,
                                       const torch::Tensor& x,
                                       const torch::Tensor& mean,
                                       const torch::Tensor& rstd,
                                       const torch::Tensor& bias, double slope,
                                       bool act, const LnGeom& g) {
  auto fopts = x.options().dtype(torch::kFloat32);
  auto dx = torch::empty_like(x);
  auto dbias = torch::empty({g.T, g.D}, fopts);
  LnParams<scalar_t> p{};
  p.x = reinterpret_cast<const scalar_t*>(x.data_ptr());
  p.dy = reinterpret_cast<const scalar_t*>(dy.data_ptr());
  p.o0 = reinterpret_cast<scalar_t*>(dx.data_ptr());
  p.bias = bias.data_ptr<float>();
  p.mean = mean.data_ptr<float>();
  p.rstd = rstd.data_ptr<float>();
  p.slope = (float)slope;
  p.vec_ok = ln_aligned({p.x, p.dy, p.o0});
  ln_launch<scalar_t, LN_BWD>(p, g, bias.dim() == 2, act, x);
  ln_dbias_launch<scalar_t>(dy, x, mean, rstd, bias, dbias, g, slope, act,
                            p.vec_ok && g.D % 8 == 0);
  return {dx, dbias};
}

template <typename scalar_t>
std::vector<torch::Tensor> ln_dbwd_impl(const torch::Tensor& x,
                                        const torch::Tensor& dy,
                                        const torch::Tensor& gx,
                                        const torch::Tensor& gb,
                                        const torch::Tensor& mean,
                                        const torch::Tensor& rstd,
                                        const torch::Tensor& bias,
                                        double slope, bool act,
                                        const LnGeom& g) {
  auto d_dy = torch::empty_like(x);
  auto d_x = torch::empty_like(x);
  LnParams<scalar_t> p{};
  p.x = reinterpret_cast<const scalar_t*>(x.data_ptr());
  p.dy = reinterpret_cast<const scalar_t*>(dy.data_ptr());
  p.gx = reinterpret_cast<const scalar_t*>(gx.data_ptr());
  p.o0 = reinterpret_cast<scalar_t*>(d_dy.data_ptr());
  p.o1 = reinterpret_cast<scalar_t*>(d_x.data_ptr());
  p.bias = bias.data_ptr<float>();
  p.gb = gb.data_ptr<float>();
  p.mean = mean.data_ptr<float>();
  p.rstd = rstd.data_ptr<float>();
  p.slope = (float)slope;
  p.vec_ok = ln_aligned({p.x, p.dy, p.gx, p.o0, p.o1});
  ln_launch<scalar_t, LN_DBWD>(p, g, bias.dim() == 2, act, x);
  return {d_dy, d_x};
}

void ln_check_like(const torch::Tensor& a, const torch::Tensor& x,
                   const char* what) {
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() &&
                  a.scalar_type() == x.scalar_type() &&
                  a.numel() == x.numel(),
              "layernorm: ", what, " must match x");
}

void ln_check_stats(const torch::Tensor& m, const LnGeom& g, const char* what) {
  TORCH_CHECK(m.is_cuda() && m.is_contiguous() &&
                  m.scalar_type() == torch::kFloat32 && m.numel() == g.nimg,
              "layernorm: ", what, " must be fp32 [T, NS]");
}

}  // namespace

// x: [T, NS, ...] contiguous bf16/fp32 (an image is everything behind NS);
// bias: fp32 [D] or [T, D].  Returns {y, mean [T, NS], rstd [T, NS]}.
std::vector<torch::Tensor> ln_act_fwd(torch::Tensor x, torch::Tensor bias,
                                      double eps, double slope, bool act) {
  const LnGeom g = ln_geom(x);
  auto bc = bias.contiguous().to(torch::kFloat32);
  ln_check_bias(bc, g, "bias");
  if (x.scalar_type() == torch::kFloat32)
    return ln_fwd_impl<float>(x, bc, eps, slope, act, g);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16,
              "ln_act_fwd: unsupported dtype");
  return ln_fwd_impl<bf16>(x, bc, eps, slope, act, g);
}

// Returns {dx, dbias_t [T, D]} (the caller folds dbias_t over T for a
// shared bias).
std::vector<torch::Tensor> ln_act_bwd(torch::Tensor dy, torch::Tensor x,
                                      torch::Tensor mean, torch::Tensor rstd,
                                      torch::Tensor bias, double slope,
                                      bool act) {
  const LnGeom g = ln_geom(x);
  auto bc = bias.contiguous().to(torch::kFloat32);
  auto dyc = dy.contiguous();
  auto mc = mean.contiguous(), rc = rstd.contiguous();
  ln_check_bias(bc, g, "bias");
  ln_check_like(dyc, x, "dy");
  ln_check_stats(mc, g, "mean");
  ln_check_stats(rc, g, "rstd");
  if (x.scalar_type() == torch::kFloat32)
    return ln_bwd_impl<float>(dyc, x, mc, rc, bc, slope, act, g);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16,
              "ln_act_bwd: unsupported dtype");
  return ln_bwd_impl<bf16>(dyc, x, mc, rc, bc, slope, act, g);
}

// Backward of ln_act_bwd: cotangents gx (of dx) and gb [T, D] (of
// dbias_t).  Returns {d_dy, d_x}; the bias gets no gradient.
std::vector<torch::Tensor> ln_act_dbwd(torch::Tensor x, torch::Tensor dy,
                                       torch::Tensor gx, torch::Tensor gb,
                                       torch::Tensor mean, torch::Tensor rstd,
                                       torch::Tensor bias, double slope,
                                       bool act) {
  const LnGeom g = ln_geom(x);
  auto bc = bias.contiguous().to(torch::kFloat32);
  auto gbc = gb.contiguous().to(torch::kFloat32);
  auto dyc = dy.contiguous();
  auto gxc = gx.contiguous();
  auto mc = mean.contiguous(), rc = rstd.contiguous();
  ln_check_bias(bc, g, "bias");
  TORCH_CHECK(gbc.is_cuda() && gbc.dim() == 2 && gbc.size(0) == g.T &&
                  gbc.size(1) == g.D,
              "ln_act_dbwd: gb must be [T, D]");
  ln_check_like(dyc, x, "dy");
  ln_check_like(gxc, x, "gx");
  ln_check_stats(mc, g, "mean");
  ln_check_stats(rc, g, "rstd");
  if (x.scalar_type() == torch::kFloat32)
    return ln_dbwd_impl<float>(x, dyc, gxc, gbc, mc, rc, bc, slope, act, g);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16,
              "ln_act_dbwd: unsupported dtype");
  return ln_dbwd_impl<bf16>(x, dyc, gxc, gbc, mc, rc, bc, slope, act, g);
}
