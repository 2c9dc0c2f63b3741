// Analytic double-backward of fused BN(batch stats)+leaky-ReLU.
//
// Second-order MAML differentiates the inner-loop support backward
// (create_graph=True), so the backward of BN must itself be
// differentiable.  Instead of a torch-op composition (measured ~25% of
// step kernel-time as ATen reduce/elementwise swarm), these kernels
// evaluate the closed form.
//
// Notation per (t, c), means <.> over the M image positions:
//   r = rstd, xh = (x - mu) * r, pre = g*xh + b, mask = pre>0 ? 1 : slope
//   u' = u * mask                          (u = incoming dy of the fwd)
//   first backward:  dx = g*r*(u' - s1 - xh*s2), dgamma = M*s2, dbeta = M*s1
//     with s1 = <u'>, s2 = <u'*xh>
// Given gx = dL/d(dx), ggam = dL/d(dgamma_t), gbet = dL/d(dbeta_t):
//   G = <gx>, Gxh = <gx*xh>, Gu = <gx*u'>
//   d_u  = mask * [ g*r*(gx - G - xh*Gxh) + ggam*xh + gbet ]
//   d_x  = g*r^2 * [ -xh*(Gu - s1*G - s2*Gxh) - s2*(gx - G - xh*Gxh)
//                    - (u' - s1 - xh*s2)*Gxh ]
//          + ggam * r * (u' - s1 - xh*s2)
//   d_gamma_t = r * M * (Gu - s1*G - s2*Gxh)        (computed from sums
//   d_beta_t  = 0                                    by the wrapper)
// (the leaky-ReLU mask is treated as constant — a.e. exact, same as ATen.)

#include "common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;
using bf16 = __hip_bfloat16;

// ---------------------------------------------------------------------------
// pass 1: the five per-(t,c) sums  [T, 5, C] = {s1, s2, G, Gxh, Gu} * M
// ---------------------------------------------------------------------------
template <typename scalar_t, bool PER_TASK_AFFINE>
__global__ void bn_dbwd_sums_kernel(const scalar_t* __restrict__ x,
                                    const scalar_t* __restrict__ u,
                                    const scalar_t* __restrict__ gx,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ rstd,
                                    const float* __restrict__ gamma,
                                    const float* __restrict__ beta,
                                    float* __restrict__ partials,  // [T,NBLK,5,C]
                                    int T, long M, int C, float slope,
                                    bool act, int rows_per_block) {
  const int cpad = ((C + WAVE - 1) / WAVE) * WAVE;
  const int rows_in_block = blockDim.x / cpad;
  const int c = threadIdx.x % cpad;
  const int rgroup = threadIdx.x / cpad;
  const int t = blockIdx.x;
  const long row0 = (long)blockIdx.y * rows_per_block;
  if (c >= C) return;

  const long tc = (long)t * C + c;
  const float mu = mean[tc], r = rstd[tc];
  const float g = PER_TASK_AFFINE ? gamma[tc] : gamma[c];
  const float b = PER_TASK_AFFINE ? beta[tc] : beta[c];
  const long base = (long)t * M * C + c;
  float s1 = 0.f, s2 = 0.f, G = 0.f, Gxh = 0.f, Gu = 0.f;
  const long row_end = min(row0 + rows_per_block, M);
  for (long m = row0 + rgroup; m < row_end; m += rows_in_block) {
    const long i = base + m * C;
    const float xh = (to_f32(x[i]) - mu) * r;
    float up = to_f32(u[i]);
    if (act) up *= ((g * xh + b) > 0.f) ? 1.f : slope;
    const float gv = to_f32(gx[i]);
    s1 += up;
    s2 += up * xh;
    G += gv;
    Gxh += gv * xh;
    Gu += gv * up;
  }
  extern __shared__ float lds[];  // [5][blockDim.x]
  const int n = blockDim.x;
  lds[0 * n + threadIdx.x] = s1;
  lds[1 * n + threadIdx.x] = s2;
  lds[2 * n + threadIdx.x] = G;
  lds[3 * n + threadIdx.x] = Gxh;
  lds[4 * n + threadIdx.x] = Gu;
  __syncthreads();
  if (rgroup == 0) {
    for (int rr = 1; rr < rows_in_block; ++rr) {
      s1 += lds[0 * n + rr * cpad + c];
      s2 += lds[1 * n + rr * cpad + c];
      G += lds[2 * n + rr * cpad + c];
      Gxh += lds[3 * n + rr * cpad + c];
      Gu += lds[4 * n + rr * cpad + c];
    }
    // private per-block slice; reduced in fixed order by bn_reduce5_kernel
    float* pt = partials + (((long)t * gridDim.y + blockIdx.y) * 5) * C;
    pt[0 * C + c] = s1;
    pt[1 * C + c] = s2;
    pt[2 * C + c] = G;
    pt[3 * C + c] = Gxh;
    pt[4 * C + c] = Gu;
  }
}

// ordered reduction of partials[T, NBLK, 5, C] -> sums[T, 5, C]
// (bitwise run-to-run deterministic; no global atomics).  The loads of
// kAhead5 blocks are issued together and then added in ascending block
// order: one serial chain of additions per (t, c), as before — only the
// load latency overlaps.
// With dgamma_t != nullptr the thread also finishes
//   d_gamma_t = rstd * M * (Gu - s1*G - s2*Gxh)          (means over M)
// with the operations, and the order, of the tensor expression it replaces
// (s = sums * (1/M); rstd * M; s4 - s0*s2 - s1*s3; product), each rounded
// on its own: contraction is off for those lines.
constexpr int kAhead5 = 8;
__global__ void __launch_bounds__(256)
bn_reduce5_kernel(const float* __restrict__ partials, float* __restrict__ sums,
                  int T, int nblk, int C, const float* __restrict__ rstd,
                  float* __restrict__ dgamma_t, float Mf, float invM) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * C) return;
  const int t = i / C, c = i % C;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < nblk; b0 += kAhead5) {
    float v[kAhead5][5];
#pragma unroll
    for (int a = 0; a < kAhead5; ++a) {
      if (b0 + a < nblk) {
        const float* p = partials + (((long)t * nblk + b0 + a) * 5) * C;
#pragma unroll
        for (int k = 0; k < 5; ++k) v[a][k] = p[k * C + c];
      }
    }
#pragma unroll
    for (int a = 0; a < kAhead5; ++a) {
      if (b0 + a < nblk) {
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[k] += v[a][k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) sums[((long)t * 5 + k) * C + c] = acc[k];
  if (dgamma_t != nullptr) {
#pragma clang fp contract(off)
    const float s0 = acc[0] * invM, s1 = acc[1] * invM, s2 = acc[2] * invM,
                s3 = acc[3] * invM, s4 = acc[4] * invM;
    const float rm = rstd[i] * Mf;
    const float p02 = s0 * s2;
    const float d1 = s4 - p02;
    const float p13 = s1 * s3;
    const float d2 = d1 - p13;
    dgamma_t[i] = rm * d2;
  }
}

// ---------------------------------------------------------------------------
// pass 2: elementwise d_u and d_x
// ---------------------------------------------------------------------------
template <typename scalar_t, bool PER_TASK_AFFINE>
__global__ void bn_dbwd_apply_kernel(const scalar_t* __restrict__ x,
                                     const scalar_t* __restrict__ u,
                                     const scalar_t* __restrict__ gx,
                                     scalar_t* __restrict__ d_u,
                                     scalar_t* __restrict__ d_x,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     const float* __restrict__ gamma,
                                     const float* __restrict__ beta,
                                     const float* __restrict__ ggam,  // [T,C]
                                     const float* __restrict__ gbet,  // [T,C]
                                     const float* __restrict__ sums,  // [T,5,C]
                                     int T, long M, int C, float slope,
                                     bool act) {
  const long total = (long)T * M * C;
  const float invM = 1.f / (float)M;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    const int c = (int)(i % C);
    const int t = (int)(i / (M * (long)C));
    const long tc = (long)t * C + c;
    const float mu = mean[tc], r = rstd[tc];
    const float g = PER_TASK_AFFINE ? gamma[tc] : gamma[c];
    const float b = PER_TASK_AFFINE ? beta[tc] : beta[c];
    const float s1 = sums[((long)t * 5 + 0) * C + c] * invM;
    const float s2 = sums[((long)t * 5 + 1) * C + c] * invM;
    const float G = sums[((long)t * 5 + 2) * C + c] * invM;
    const float Gxh = sums[((long)t * 5 + 3) * C + c] * invM;
    const float Gu = sums[((long)t * 5 + 4) * C + c] * invM;
    const float gg = ggam[tc];
    const float gb = gbet[tc];

    const float xh = (to_f32(x[i]) - mu) * r;
    float mask = 1.f;
    if (act) mask = ((g * xh + b) > 0.f) ? 1.f : slope;
    const float up = to_f32(u[i]) * mask;
    const float gv = to_f32(gx[i]);

    const float ucent = up - s1 - xh * s2;
    const float gcent = gv - G - xh * Gxh;
    const float du = mask * (g * r * gcent + gg * xh + gb);
    const float dxv = g * r * r *
                          (-xh * (Gu - s1 * G - s2 * Gxh) - s2 * gcent -
                           ucent * Gxh) +
                      gg * r * ucent;
    d_u[i] = from_f32<scalar_t>(du);
    d_x[i] = from_f32<scalar_t>(dxv);
  }
}

// ---------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------
namespace {
constexpr int kRowsPerBlockD = 256;
constexpr int kThreadsD = 256;
}  // namespace

// ---------------------------------------------------------------------------
// pass 1, 8 channels per thread (16-byte loads for bf16), C % 8 == 0.
//
// The partials are bit-for-bit those of bn_dbwd_sums_kernel: partial
// (t, slice, c) covers rows [256*slice, 256*slice + 256) and is the serial
// sum over rgroup = 0..R-1 of the serial ascending sum over the rows
// m = 256*slice + rgroup + R*k, with R that kernel's row groups per block
// (4 for C <= 64).  Here a thread owns one (slice, rgroup) chain for 8
// channels and a block owns several slices; which addends enter which chain,
// and in what order, is unchanged.
//
// The per-element operations are pinned to the ones the compiler chose for
// the scalar kernel (its pairing of G with s2 leaves s2's product unfused,
// Gxh and Gu are fused): contraction is off and every fma is explicit, so
// the 8-wide layout cannot shift them.
// ---------------------------------------------------------------------------
template <typename scalar_t, bool PER_TASK_AFFINE>
__global__ void bn_dbwd_sums_vec_kernel(
    const scalar_t* __restrict__ x, const scalar_t* __restrict__ u,
    const scalar_t* __restrict__ gx, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta,
    float* __restrict__ partials,  // [T, NSLICE, 5, C]
    long M, int C, float slope, bool act, int R, int slices_per_block,
    int nslice) {
  const int c8n = C / 8;
  const int c8 = threadIdx.x % c8n;
  const int chain = threadIdx.x / c8n;  // (slice in block, rgroup)
  const int sl = chain / R, rg = chain % R;
  const int t = blockIdx.x;
  const int slice = blockIdx.y * slices_per_block + sl;
  const bool live = sl < slices_per_block && slice < nslice;
  const int c0 = c8 * 8;
  extern __shared__ float ls[];  // [chains][5][C]
  if (live) {
    float mu[8], r[8], g[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long tc = (long)t * C + c0 + j;
      mu[j] = mean[tc]; r[j] = rstd[tc];
      g[j] = PER_TASK_AFFINE ? gamma[tc] : gamma[c0 + j];
      b[j] = PER_TASK_AFFINE ? beta[tc] : beta[c0 + j];
    }
    float s1[8] = {0}, s2[8] = {0}, G[8] = {0}, Gxh[8] = {0}, Gu[8] = {0};
    const long base = (long)t * M * C + c0;
    const long row0 = (long)slice * kRowsPerBlockD;
    const long row_end = min(row0 + kRowsPerBlockD, M);
    for (long m = row0 + rg; m < row_end; m += R) {
      float xv[8], uv[8], gxv[8];
      load8(x + base + m * C, xv);
      load8(u + base + m * C, uv);
      load8(gx + base + m * C, gxv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma clang fp contract(off)
        const float xh = (xv[j] - mu[j]) * r[j];
        float up = uv[j];
        if (act) up = up * ((__builtin_fmaf(g[j], xh, b[j]) > 0.f) ? 1.f : slope);
        const float gv = gxv[j];
        const float upxh = up * xh;
        s1[j] = s1[j] + up;
        s2[j] = s2[j] + upxh;
        G[j] = G[j] + gv;
        Gxh[j] = __builtin_fmaf(gv, xh, Gxh[j]);
        Gu[j] = __builtin_fmaf(gv, up, Gu[j]);
      }
    }
    float* lc = ls + (long)chain * 5 * C + c0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      lc[0 * C + j] = s1[j];
      lc[1 * C + j] = s2[j];
      lc[2 * C + j] = G[j];
      lc[3 * C + j] = Gxh[j];
      lc[4 * C + j] = Gu[j];
    }
  }
  __syncthreads();
  if (live && rg == 0) {
    // rgroup 0 + rgroup 1 + ... in this order, as the scalar kernel adds
    float* pt = partials + (((long)t * nslice + slice) * 5) * C + c0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = ls[((long)chain * 5 + k) * C + c0 + j];
        for (int rr = 1; rr < R; ++rr)
          v += ls[((long)(chain + rr) * 5 + k) * C + c0 + j];
        pt[k * C + j] = v;
      }
    }
  }
}

namespace {

// The two passes on x, u, gx [T, M, C].  vec_sums: the 8-channel sums kernel
// where C allows it.  With d_gamma_t defined the reduce also finishes
// d_gamma_t [T, C].  returns {d_u, d_x, sums[T,5,C]}
std::vector<torch::Tensor> dbwd_run(const torch::Tensor& x,
                                    const torch::Tensor& u,
                                    const torch::Tensor& gx,
                                    const torch::Tensor& mean,
                                    const torch::Tensor& rstd,
                                    const torch::Tensor& gamma,
                                    const torch::Tensor& beta,
                                    const torch::Tensor& ggam,
                                    const torch::Tensor& gbet, double slope,
                                    bool act, bool vec_sums,
                                    torch::Tensor d_gamma_t) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous());
  const int T = (int)x.size(0);
  const long M = x.size(1);
  const int C = (int)x.size(2);
  TORCH_CHECK(u.numel() == x.numel() && gx.numel() == x.numel());
  auto fopts = x.options().dtype(torch::kFloat32);
  auto sums = torch::empty({T, 5, C}, fopts);  // bn_reduce5 writes it whole
  auto d_u = torch::empty_like(x);
  auto d_x = torch::empty_like(x);
  auto gc = gamma.contiguous().to(torch::kFloat32);
  auto bc = beta.contiguous().to(torch::kFloat32);
  auto ggc = ggam.contiguous().to(torch::kFloat32);
  auto gbc = gbet.contiguous().to(torch::kFloat32);
  auto uc = u.contiguous();
  auto gxc = gx.contiguous();
  const bool per_task = gamma.dim() == 2;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int cpad = ((C + WAVE - 1) / WAVE) * WAVE;
  const int threads = cpad * std::max<int>(1, kThreadsD / cpad);
  dim3 sums_grid(T, (unsigned)((M + kRowsPerBlockD - 1) / kRowsPerBlockD));
  const int lds_bytes = 5 * threads * (int)sizeof(float);
  const long total = (long)T * M * C;
  // vector sums: a block owns spb 256-row slices, one (slice, rgroup) chain
  // per thread; R = the scalar kernel's row groups per block
  const int R = threads / cpad;
  const int c8n = std::max(1, C / 8);
  const int spb = std::max(1, std::min(kThreadsD / c8n / R, 16));
  const int vblocks = ((int)sums_grid.y + spb - 1) / spb;
  const int vlds_bytes = spb * R * 5 * C * (int)sizeof(float);
  const bool vec = vec_sums && (C % 8 == 0) && C <= 512 && vblocks <= 65535;
  TORCH_CHECK(!vec || spb * R * c8n <= kThreadsD);
  const float Mf = (float)M;
  const float invM = 1.0f / Mf;
  const float* rstd_p = d_gamma_t.defined() ? rstd.data_ptr<float>() : nullptr;
  float* dgam_p = d_gamma_t.defined() ? d_gamma_t.data_ptr<float>() : nullptr;

#define LAUNCH_DB(ST, PT)                                                      \
  do {                                                                         \
    const int nblk = (int)sums_grid.y;                                         \
    auto partials = torch::empty({T, nblk, 5, C}, fopts);                      \
    if (vec)                                                                   \
      hipLaunchKernelGGL((bn_dbwd_sums_vec_kernel<ST, PT>),                    \
                         dim3(T, vblocks), dim3(kThreadsD), vlds_bytes,        \
                         stream.stream(),                                      \
                         reinterpret_cast<const ST*>(x.data_ptr()),            \
                         reinterpret_cast<const ST*>(uc.data_ptr()),           \
                         reinterpret_cast<const ST*>(gxc.data_ptr()),          \
                         mean.data_ptr<float>(), rstd.data_ptr<float>(),       \
                         gc.data_ptr<float>(), bc.data_ptr<float>(),           \
                         partials.data_ptr<float>(), M, C, (float)slope, act,  \
                         R, spb, nblk);                                        \
    else                                                                       \
    hipLaunchKernelGGL((bn_dbwd_sums_kernel<ST, PT>), sums_grid,               \
                       dim3(threads), lds_bytes, stream.stream(),              \
                       reinterpret_cast<const ST*>(x.data_ptr()),              \
                       reinterpret_cast<const ST*>(uc.data_ptr()),             \
                       reinterpret_cast<const ST*>(gxc.data_ptr()),            \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                       gc.data_ptr<float>(), bc.data_ptr<float>(),             \
                       partials.data_ptr<float>(), T, M, C, (float)slope, act, \
                       kRowsPerBlockD);                                        \
    hipLaunchKernelGGL(bn_reduce5_kernel, dim3((T * C + 255) / 256),           \
                       dim3(256), 0, stream.stream(),                          \
                       partials.data_ptr<float>(), sums.data_ptr<float>(),     \
                       T, nblk, C, rstd_p, dgam_p, Mf, invM);                  \
    hipLaunchKernelGGL((bn_dbwd_apply_kernel<ST, PT>),                         \
                       dim3(ew_grid(total, kThreadsD)), dim3(kThreadsD), 0,    \
                       stream.stream(),                                        \
                       reinterpret_cast<const ST*>(x.data_ptr()),              \
                       reinterpret_cast<const ST*>(uc.data_ptr()),             \
                       reinterpret_cast<const ST*>(gxc.data_ptr()),            \
                       reinterpret_cast<ST*>(d_u.data_ptr()),                  \
                       reinterpret_cast<ST*>(d_x.data_ptr()),                  \
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),         \
                       gc.data_ptr<float>(), bc.data_ptr<float>(),             \
                       ggc.data_ptr<float>(), gbc.data_ptr<float>(),           \
                       sums.data_ptr<float>(), T, M, C, (float)slope, act);    \
  } while (0)

  if (x.scalar_type() == torch::kFloat32) {
    if (per_task) LAUNCH_DB(float, true); else LAUNCH_DB(float, false);
  } else if (x.scalar_type() == torch::kBFloat16) {
    if (per_task) LAUNCH_DB(bf16, true); else LAUNCH_DB(bf16, false);
  } else {
    TORCH_CHECK(false, "bn_act_dbwd: unsupported dtype");
  }
#undef LAUNCH_DB
  return {d_u, d_x, sums};
}

}  // namespace

// returns {d_u, d_x, sums[T,5,C]} — d_gamma_t is finished by the wrapper:
//   d_gamma_t = rstd * (Gu_sum - s1m*G_sum... see hip_autograd (cheap [T,C]).
std::vector<torch::Tensor> bn_act_dbwd(torch::Tensor x, torch::Tensor u,
                                       torch::Tensor gx, torch::Tensor mean,
                                       torch::Tensor rstd, torch::Tensor gamma,
                                       torch::Tensor beta, torch::Tensor ggam,
                                       torch::Tensor gbet, double slope,
                                       bool act) {
  return dbwd_run(x, u, gx, mean, rstd, gamma, beta, ggam, gbet, slope, act,
                  /*vec_sums=*/false, torch::Tensor());
}

// The same two passes as one call for the autograd backward: absent
// ggam / gbet ([T,C] fp32) read as zero, the sums pass runs 8 channels per
// thread where C allows (bits unchanged), and the reduce finishes
// d_gamma_t = rstd * M * (Gu - s1*G - s2*Gxh) with the bits of the tensor
// formula it replaces.  returns {d_u, d_x, d_gamma_t [T,C], sums [T,5,C]}
std::vector<torch::Tensor> bn_act_dbwd_full(
    torch::Tensor x, torch::Tensor u, torch::Tensor gx, torch::Tensor mean,
    torch::Tensor rstd, torch::Tensor gamma, torch::Tensor beta,
    c10::optional<torch::Tensor> ggam, c10::optional<torch::Tensor> gbet,
    double slope, bool act) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3);
  const long T = x.size(0), C = x.size(2);
  TORCH_CHECK(mean.numel() == T * C && rstd.numel() == T * C);
  auto fopts = x.options().dtype(torch::kFloat32);
  const bool has_gg = ggam.has_value() && ggam->defined();
  const bool has_gb = gbet.has_value() && gbet->defined();
  TORCH_CHECK((!has_gg || ggam->numel() == T * C) &&
              (!has_gb || gbet->numel() == T * C));
  torch::Tensor zero;
  if (!has_gg || !has_gb) zero = torch::zeros({T, C}, fopts);
  auto d_gamma_t = torch::empty({T, C}, fopts);
  auto out = dbwd_run(x, u, gx, mean, rstd, gamma, beta,
                      has_gg ? *ggam : zero, has_gb ? *gbet : zero, slope, act,
                      /*vec_sums=*/true, d_gamma_t);
  return {out[0], out[1], d_gamma_t, out[2]};
}
