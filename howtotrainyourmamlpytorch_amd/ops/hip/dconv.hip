// Direct (non-GEMM) 3x3 convolution for SMALL input-channel counts — the
// network's first layer (C in {1,3}; reference images are grayscale
// Omniglot / RGB mini-imagenet).
//
// The im2col-MFMA path is mis-shaped here: K = 9*C is 9..27, so the
// 32-wide MFMA K granularity plus BK=64 staging wastes >4x the real MACs
// and the measured rate is 8-25 TF.  CDNA4's VECTOR ALU (157 TF fp32) is
// the right unit for K this small:
//
//   fwd:   one thread per output position computes ALL F channels with
//          the 9*C*F weights staged in LDS and read wave-uniform
//          (hardware broadcast — no bank traffic), x window in registers.
//   wgrad: lane = output channel f; each wave walks a contiguous range of
//          positions; dy reads are coalesced across lanes, the x window
//          is a wave-uniform (single-cacheline) load; each lane holds its
//          f's full dW[c][ky][kx] tile (<= 27 fp32) in registers.
//
// Both are FMA-throughput bound by construction instead of staging bound.

#include "common.h"
#include "conv_host.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

using bf16 = __hip_bfloat16;
typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;

// ---------------------------------------------------------------------------
// fwd: X [T,NB,H,W,C] bf16 -> Y [T,NB,Ho,Wo,F] bf16 (F = FT compile-time)
// ---------------------------------------------------------------------------
template <int FT>
__global__ __launch_bounds__(256)
void dconv_fwd_kernel(const bf16* __restrict__ X, const float* __restrict__ W,
                      const float* __restrict__ bias, bf16* __restrict__ Y,
                      int T, int NB, int H, int Wd, int C,
                      int Ho, int Wo, int pad) {
  const int t = blockIdx.y;
  __shared__ float wl[9 * 8 * FT];  // [kyx][c][f]
  const float* Wt = W + (long)t * FT * C * 9;
  for (int i = threadIdx.x; i < FT * C * 9; i += blockDim.x) {
    // i over [f][c][kyx] source order -> [kyx][c][f] LDS order
    const int kyx = i % 9;
    const int c = (i / 9) % C;
    const int f = i / (9 * C);
    wl[(kyx * C + c) * FT + f] = Wt[i];
  }
  __syncthreads();

  const long Mtot = (long)NB * Ho * Wo;
  const bf16* Xt = X + (long)t * NB * H * Wd * C;
  bf16* Yt = Y + (long)t * Mtot * FT;
  const float* bt = bias ? bias + (long)t * FT : nullptr;

  for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < Mtot;
       m += (long)blockDim.x * gridDim.x) {
    const int wo = (int)(m % Wo);
    const int ho = (int)((m / Wo) % Ho);
    const int n = (int)(m / ((long)Wo * Ho));
    float acc[FT];
#pragma unroll
    for (int f = 0; f < FT; ++f) acc[f] = bt ? bt[f] : 0.f;
    for (int ky = 0; ky < 3; ++ky) {
      const int h = ho + ky - pad;
      if (h < 0 || h >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int w = wo + kx - pad;
        if (w < 0 || w >= Wd) continue;
        const short* xrow = (const short*)Xt + (((long)n * H + h) * Wd + w) * C;
        for (int c = 0; c < C; ++c) {
          const float xv = __bfloat162float(
              __hip_bfloat16(__hip_bfloat16_raw{(unsigned short)xrow[c]}));
          const float* wp = &wl[((ky * 3 + kx) * C + c) * FT];
#pragma unroll
          for (int f = 0; f < FT; ++f) acc[f] = fmaf(xv, wp[f], acc[f]);
        }
      }
    }
#pragma unroll
    for (int f8 = 0; f8 < FT / 8; ++f8) {
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (short)__bfloat16_as_short(__float2bfloat16(acc[f8 * 8 + j]));
      *(bf16x8*)&((short*)Yt)[m * FT + f8 * 8] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// fwd v2 (default for the workloads' C in {1,3}): the same fp32 arithmetic
// on the fp32 matrix unit.  v_mfma_f32_16x16x4_f32 runs at the VALU's peak
// rate and is bit for bit a k-ordered fmaf chain on the accumulator, so
//   acc = bias[f]; acc = fmaf(float(x), w_fp32, acc) over ky, kx, c
// comes out as in dconv_fwd_kernel (an out-of-image tap contributes
// fmaf(0, w, acc) instead of being skipped: at most the sign of a zero).
// What changes is how the operands arrive:
//   * weights sit in REGISTERS for the kernel's lifetime, one per lane per
//     MFMA (A[f = lane&15][k = lane>>4]): no LDS at all.  The v1 kernel's
//     wave-uniform ds_read_b128 costs 4 LDS cycles per 4 weights whatever
//     the broadcast, 12 reads per 24 v_pk_fma_f32 — twice the FMA time on
//     the CU's one LDS port — and its x loads are 9C dependent latencies;
//   * x is one 2-byte load per lane per k-step (B[k = lane>>4][pos =
//     lane&15]), all 9C/4 of a tile issued together and one tile ahead of
//     the MFMAs that consume them;
//   * D[f][pos] leaves each lane 4 consecutive f of one position: 8-byte
//     stores, a tile's FT*32 bytes of Y contiguous.
// k = (ky*3+kx)*CT + c is padded to a multiple of 4 with w = x = 0.
// A wave owns 16-position tiles tile0, tile0+S, ... and advances its
// (img, ho, wo) by S tiles with adds and compares.
// ---------------------------------------------------------------------------
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;
typedef __attribute__((__vector_size__(4 * sizeof(short)))) short bf16x4;

template <int FT, int CT>
__global__ __launch_bounds__(256)
void dconv_fwd_v2_kernel(const bf16* __restrict__ X, const float* __restrict__ W,
                         const float* __restrict__ bias, bf16* __restrict__ Y,
                         int NB, int H, int Wd, int Ho, int Wo, int pad) {
  constexpr int K = 9 * CT;
  constexpr int KS = (K + 3) / 4;    // MFMA k-steps
  constexpr int NT = FT / 16;        // 16-channel tiles
  constexpr int kInvalid = -(1 << 30);
  const int t = blockIdx.y;
  // wave-uniform by construction: keeps the tile loop on the scalar unit
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lane = threadIdx.x % WAVE;
  const int li = lane & 15;          // A: channel in tile; B, D: position in tile
  const int g = lane >> 4;           // A, B: k in step; D: 4-channel group
  const int Mtot = NB * Ho * Wo;
  const int ntiles = (Mtot + 15) / 16;

  const float* Wt = W + (long)t * FT * CT * 9;
  const unsigned short* Xt =
      (const unsigned short*)X + (long)t * NB * H * Wd * CT;
  short* Yt = (short*)Y + (long)t * Mtot * FT;

  // per-lane k decode (once): weight registers, x tap offsets
  float wa[KS][NT];
  int koff[KS], kdy[KS], kdx[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 4 * s + g;
    const bool kv = k < K;
    const int tap = kv ? k / CT : 0;
    const int c = kv ? k - tap * CT : 0;
    const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      wa[s][nt] = kv ? Wt[((nt * 16 + li) * CT + c) * 9 + tap] : 0.f;
    koff[s] = (dy * Wd + dx) * CT + c;
    kdy[s] = kv ? dy : (1 << 20);    // k padding: no row is ever in range
    kdx[s] = dx;
  }
  f32x4 bv[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bv[nt][j] = bias ? bias[(long)t * FT + nt * 16 + g * 4 + j] : 0.f;

  // this lane's position m = tile*16 + li and its stride per iteration
  const int stride = gridDim.x * (blockDim.x / WAVE);   // tiles
  const int dm = stride * 16;
  const int dwo = dm % Wo;
  const int dho = (dm / Wo) % Ho;
  const int dimg = (dm / Wo) / Ho;
  int tile = blockIdx.x * (blockDim.x / WAVE) + wave;
  int m = tile * 16 + li;
  int wo = m % Wo, ho = (m / Wo) % Ho, img = (m / Wo) / Ho;

  // the 9C (padded) window values of position (img, ho, wo), raw bf16;
  // every load is independent of the others
  unsigned short xr[KS];
#define DFWD2_LOAD()                                                           \
  do {                                                                         \
    const bool mv = m < Mtot;                                                  \
    const int hb = mv ? ho - pad : kInvalid;                                   \
    const int wb = wo - pad;                                                   \
    const int base = mv ? ((img * H + hb) * Wd + wb) * CT : 0;                 \
    _Pragma("unroll")                                                          \
    for (int s = 0; s < KS; ++s) {                                             \
      const bool ok = (unsigned)(hb + kdy[s]) < (unsigned)H &&                 \
                      (unsigned)(wb + kdx[s]) < (unsigned)Wd;                  \
      xr[s] = ok ? Xt[base + koff[s]] : (unsigned short)0;                     \
    }                                                                          \
  } while (0)

  // Per iteration: convert the window loaded one iteration ago, issue the
  // next tile's loads, then the MFMAs and the stores — the loads are in
  // flight behind the MFMA run.  (Measured slower, 3.5 against 2.9 ms at the
  // flagship's target call: branch-free clamped loads all issued ahead of
  // the MFMAs and consumed before the stores, so that the in-order memory
  // counter never waits on stores just issued.)
  DFWD2_LOAD();
  for (; tile < ntiles; tile += stride) {
    float xb[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
      xb[s] = __uint_as_float((unsigned)xr[s] << 16);
    const int m_cur = m;
    // next tile's position (past the end: every load predicated off)
    m += dm;
    wo += dwo;
    if (wo >= Wo) { wo -= Wo; ho += 1; }
    ho += dho;
    if (ho >= Ho) { ho -= Ho; img += 1; }
    img += dimg;
    DFWD2_LOAD();

    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = bv[nt];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s][nt], xb[s],
                                                       acc[nt], 0, 0, 0);
    if (m_cur < Mtot) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        bf16x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] = (short)__bfloat16_as_short(__float2bfloat16(acc[nt][j]));
        *(bf16x4*)&Yt[(long)m_cur * FT + nt * 16 + g * 4] = v;
      }
    }
  }
#undef DFWD2_LOAD
}

// ---------------------------------------------------------------------------
// wgrad: dWacc [T, nsl, 9C, F] (+ dBacc [T, nsl, F]) — same accumulator
// layout as the GEMM wgrad so the shared finalize kernel applies.
// lane = f; wave walks contiguous positions; CT = compile-time C.
// ---------------------------------------------------------------------------
template <int CT, bool DET>
__global__ __launch_bounds__(256)
void dconv_wgrad_kernel(const bf16* __restrict__ dY, const bf16* __restrict__ X,
                        float* __restrict__ dWacc, float* __restrict__ dBacc,
                        int T, int NB, int H, int Wd, int Ho, int Wo, int F,
                        int pad, long chunk) {
  const int t = blockIdx.y;
  const long Mtot = (long)NB * Ho * Wo;
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int nwaves = blockDim.x / WAVE;
  // this wave's contiguous position range
  const long c0 = blockIdx.x * chunk + wave * (chunk / nwaves);
  const long c1 = min(c0 + chunk / nwaves, Mtot);

  const bf16* Xt = X + (long)t * NB * H * Wd * CT;
  const short* dYt = (const short*)dY + (long)t * Mtot * F;

  float acc[9 * CT];
#pragma unroll
  for (int i = 0; i < 9 * CT; ++i) acc[i] = 0.f;
  float db = 0.f;

  if (c0 < Mtot) {
    int wo = (int)(c0 % Wo);
    int ho = (int)((c0 / Wo) % Ho);
    int n = (int)(c0 / ((long)Wo * Ho));
    for (long m = c0; m < c1; ++m) {
      const float dyv =
          (lane < F)
              ? __bfloat162float(__hip_bfloat16(
                    __hip_bfloat16_raw{(unsigned short)dYt[m * F + lane]}))
              : 0.f;
      db += dyv;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int h = ho + ky - pad;
        if (h < 0 || h >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int w = wo + kx - pad;
          if (w < 0 || w >= Wd) continue;
          const short* xrow =
              (const short*)Xt + (((long)n * H + h) * Wd + w) * CT;
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            const float xv = __bfloat162float(__hip_bfloat16(
                __hip_bfloat16_raw{(unsigned short)xrow[c]}));
            acc[(ky * 3 + kx) * CT + c] = fmaf(dyv, xv, acc[(ky * 3 + kx) * CT + c]);
          }
        }
      }
      // incremental position decode
      if (++wo == Wo) {
        wo = 0;
        if (++ho == Ho) { ho = 0; ++n; }
      }
    }
  }

  // ordered in-block reduction across waves via LDS, then one
  // store (DET slice) or atomicAdd per [9C][F] element per block
  float* dWt = DET ? dWacc + ((long)t * gridDim.x + blockIdx.x) * 9 * CT * F
                   : dWacc + (long)t * 9 * CT * F;
  {
    __shared__ float red[256];
#pragma unroll
    for (int i = 0; i < 9 * CT; ++i) {
      red[threadIdx.x] = acc[i];
      __syncthreads();
      if (wave == 0 && lane < F) {
        float s = 0.f;
        for (int wv = 0; wv < nwaves; ++wv) s += red[wv * WAVE + lane];
        if (DET) {
          dWt[(long)i * F + lane] = s;
        } else {
          atomicAdd(&dWt[(long)i * F + lane], s);
        }
      }
      __syncthreads();
    }
  }
  if (dBacc != nullptr) {
    __shared__ float dbl[256];
    dbl[threadIdx.x] = db;
    __syncthreads();
    if (wave == 0 && lane < F) {
      float s = 0.f;
      for (int wv = 0; wv < nwaves; ++wv) s += dbl[wv * WAVE + lane];
      if (DET) {
        dBacc[((long)t * gridDim.x + blockIdx.x) * F + lane] = s;
      } else {
        atomicAdd(&dBacc[(long)t * F + lane], s);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
torch::Tensor dconv_fwd(torch::Tensor x, torch::Tensor w,
                        c10::optional<torch::Tensor> bias, long pad,
                        long Ho, long Wo) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 5 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16);
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int F = (int)w.size(1);
  TORCH_CHECK(C <= 8 && (F == 16 || F == 32 || F == 48 || F == 64),
              "dconv_fwd needs C<=8 and F in {16,32,48,64}");
  auto wc = w.contiguous().to(torch::kFloat32);
  auto y = torch::empty({T, NB, Ho, Wo, F}, x.options());
  const float* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous().to(torch::kFloat32);
    bptr = bc.data_ptr<float>();
  }
  const long Mtot = (long)NB * Ho * Wo;
  auto stream = at::cuda::getCurrentCUDAStream();
  // v2 (fp32 MFMA, weights in registers) for the workloads' C in {1, 3};
  // MAML355_DCONV_FWD_V2=0 restores dconv_fwd_kernel everywhere
  const char* v2_env = getenv("MAML355_DCONV_FWD_V2");
  const bool v2 = (C == 1 || C == 3) && !(v2_env && v2_env[0] == '0');
  if (v2) {
    TORCH_CHECK(Ho == H + 2 * pad - 2 && Wo == W + 2 * pad - 2 && Ho >= 1 &&
                    Wo >= 1 && pad >= 0,
                "dconv_fwd: Ho/Wo do not match a stride-1 3x3 conv");
    // positions and element offsets within a task are 32-bit in the kernel
    TORCH_CHECK(Mtot < (1L << 30) && (long)NB * H * W * C < (1L << 30),
                "dconv_fwd: task too large for 32-bit offsets");
    // 4 waves per block, ~8 tiles of 16 positions per wave: the per-wave
    // weight load (9C/4 * F/16 registers) is amortised, the grid stays wide
    const long ntiles = (Mtot + 15) / 16;
    const int blocks2 =
        (int)std::max<long>(1, std::min<long>((ntiles + 31) / 32, 2048));
#define LAUNCH_DFWD2(FT, CT)                                                   \
  hipLaunchKernelGGL((dconv_fwd_v2_kernel<FT, CT>), dim3(blocks2, T),          \
                     dim3(256), 0, stream.stream(),                            \
                     reinterpret_cast<const bf16*>(x.data_ptr()),              \
                     wc.data_ptr<float>(), bptr,                               \
                     reinterpret_cast<bf16*>(y.data_ptr()),                    \
                     NB, H, W, (int)Ho, (int)Wo, (int)pad)
#define LAUNCH_DFWD2_C(FT)                                                     \
  do { if (C == 1) LAUNCH_DFWD2(FT, 1); else LAUNCH_DFWD2(FT, 3); } while (0)
    switch (F) {
      case 16: LAUNCH_DFWD2_C(16); break;
      case 32: LAUNCH_DFWD2_C(32); break;
      case 48: LAUNCH_DFWD2_C(48); break;
      default: LAUNCH_DFWD2_C(64); break;
    }
#undef LAUNCH_DFWD2_C
#undef LAUNCH_DFWD2
    return y;
  }
  const int blocks = (int)std::min<long>((Mtot + 255) / 256, 4096);
#define LAUNCH_DFWD(FT)                                                       \
  hipLaunchKernelGGL((dconv_fwd_kernel<FT>), dim3(blocks, T), dim3(256), 0,    \
                     stream.stream(),                                          \
                     reinterpret_cast<const bf16*>(x.data_ptr()),              \
                     wc.data_ptr<float>(), bptr,                               \
                     reinterpret_cast<bf16*>(y.data_ptr()),                    \
                     T, NB, H, W, C, (int)Ho, (int)Wo, (int)pad)
  switch (F) {
    case 16: LAUNCH_DFWD(16); break;
    case 32: LAUNCH_DFWD(32); break;
    case 48: LAUNCH_DFWD(48); break;
    default: LAUNCH_DFWD(64); break;
  }
#undef LAUNCH_DFWD
  return y;
}

std::vector<torch::Tensor> dconv_wgrad(torch::Tensor dy, torch::Tensor x,
                                       long pad, bool with_bias) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda());
  auto dyc = dy.contiguous();
  auto xc = x.contiguous();
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int Ho = (int)dy.size(2), Wo = (int)dy.size(3), F = (int)dy.size(4);
  TORCH_CHECK(C <= 8 && F <= 64, "dconv_wgrad needs C<=8, F<=64");
  const bool det = deterministic_mode();
  const long Mtot = (long)NB * Ho * Wo;
  // chunk so total waves fill the chip (4 waves per block)
  long gridx = std::max<long>(1, 2048 / std::max(1, T));
  long chunk = (Mtot + gridx - 1) / gridx;
  chunk = std::max<long>(((chunk + 3) / 4) * 4, 4);
  gridx = (Mtot + chunk - 1) / chunk;
  const int nslices = det ? (int)gridx : 1;
  auto acc = torch::zeros({T, nslices, 9 * C, F},
                          x.options().dtype(torch::kFloat32));
  auto dbacc = torch::zeros({T, nslices, F},
                            x.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_DWG(CT, DET_)                                                   \
  hipLaunchKernelGGL((dconv_wgrad_kernel<CT, DET_>), dim3((unsigned)gridx, T), \
                     dim3(256), 0, stream.stream(),                            \
                     reinterpret_cast<const bf16*>(dyc.data_ptr()),            \
                     reinterpret_cast<const bf16*>(xc.data_ptr()),             \
                     acc.data_ptr<float>(),                                    \
                     with_bias ? dbacc.data_ptr<float>() : nullptr,            \
                     T, NB, H, W, Ho, Wo, F, (int)pad, chunk)
#define LAUNCH_DWG_DET(CT)                                                     \
  do { if (det) LAUNCH_DWG(CT, true); else LAUNCH_DWG(CT, false); } while (0)
  switch (C) {
    case 1: LAUNCH_DWG_DET(1); break;
    case 2: LAUNCH_DWG_DET(2); break;
    case 3: LAUNCH_DWG_DET(3); break;
    case 4: LAUNCH_DWG_DET(4); break;
    default: LAUNCH_DWG_DET(8); break;
  }
#undef LAUNCH_DWG
#undef LAUNCH_DWG_DET
  return finish_wgrad(acc, dbacc, T, F, C, nslices, stream.stream());
}
