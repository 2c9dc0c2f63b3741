// Transpose-free ("NT") wgrad for the task-batched 3x3 conv on gfx950.
//
//   dW[t][n=(tap,c)][f] = sum_k im2col(X[t])[k][n] * dY[t][k][f]
//
// wgrad v2 (tconv.hip) first copies dY to [f][k] and X to a channel-major
// padded image so both MFMA operands are k-contiguous in memory.  Here the
// transpose moves into the LDS read instead: both tiles are staged by
// `global_load_lds` exactly as they sit in memory (rows = positions k,
// 16-byte chunks = 8 channels) and ds_read_b64_tr_b16 hands the MFMA its
// k-contiguous fragments.  No dY^T, no XT, no per-line padding of k; conv
// zero padding and the K tail come from a constant zero page.  All address
// logic lives in wgrad_nt_addr.h and is checked on the CPU.  (Deterministic
// mode re-creates v2's line padding with zero rows, to keep v2's sums.)
//
// Block: 256 threads = 4 waves; a block owns 64*NSUB columns n and every
// f; wave w owns the 16-column sub-tiles (sb*4 + w) and iterates the
// m-tiles over F, as v2.  Split-K over blockIdx.y with fp32 atomics, or
// private slices under MAML355_DETERMINISTIC (summed in fixed order by
// wgrad_finalize_kernel).
//
// Bias gradient stays fused: where the block grid leaves a spare column
// (9C not a multiple of the block width) that column's B fragment is set to
// ones in registers, so its accumulator is sum_k dY; otherwise, and always
// in deterministic mode, the n0 == 0 block sums the A tile's columns from
// LDS, as v2 does.

#include "common.h"
#include "conv_host.h"
#include "wgrad_nt_addr.h"
#include "wgrad_plan.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

using bf16 = __hip_bfloat16;
typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;
typedef short bf16x4v __attribute__((ext_vector_type(4)));

static_assert(wgnt::kRows == wgplan::kStep,
              "wgrad_plan.h cuts K-chunks for this tile");

enum {
  NT_BIAS_NONE = wgplan::kBiasNone,
  NT_BIAS_ONES = wgplan::kBiasOnes,
  NT_BIAS_COLSUM = wgplan::kBiasColsum
};

// x [M, C] (C < 8) -> xp [M, 8], zero-filled: the first layer's channel pad
__global__ void nt_chpad8_kernel(const bf16* __restrict__ x,
                                 bf16* __restrict__ xp, long M, int C) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < M;
       i += grid_stride()) {
    bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    const short* s = (const short*)x + i * C;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < C) v[j] = s[j];
    *(bf16x8*)((short*)xp + i * 8) = v;
  }
}

DEVINL bf16x4v lds_read_tr(const short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4v*)p);
}

// MT = m-tiles over F (ceil(F / 16)), a template parameter so the fragment
// reads and MFMAs of a K-step are one branch-free block the scheduler can
// interleave.
template <int NSUB, int MT, bool DET>
__global__ __launch_bounds__(256, 4)
void tconv_wgrad_nt_kernel(const bf16* __restrict__ dY,
                           const bf16* __restrict__ X,
                           const bf16* __restrict__ zpage,
                           float* __restrict__ dWacc,  // [T, nsl, 9*Cout, F]
                           float* __restrict__ dBacc,  // [T, nsl, F] or null
                           wgnt::Geom g, int Cout, long Kr, int kchunk,
                           int bias_mode) {
  const int t = blockIdx.z;
  const int n0 = blockIdx.x * (64 * NSUB);
  const int F = g.F;
  const long kc0 = (long)blockIdx.y * kchunk;
  const long kc_end = min(kc0 + (long)kchunk, Kr);

  __shared__ __attribute__((aligned(16))) short lds_a[2][64 * 64];
  __shared__ __attribute__((aligned(16))) short lds_b[2][NSUB][64 * 64];

  const bf16* dYt = dY + (long)t * g.NB * g.Ho * g.Wo * F;
  const bf16* Xt = X + (long)t * g.NB * g.H * g.W * g.C;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lane = threadIdx.x % WAVE;
  const int fr = lane & 15;
  const int fk = lane >> 4;

  // ---- staging descriptors: slot s = q*256 + tid of every tile ----
  // rows (hence positions) are shared by the A tile and all B sub-tiles
  int s_ch[2];
  wgnt::Pos s_pos[2];
  long s_k[2];
  wgnt::Col s_col[2][NSUB];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int s = q * 256 + threadIdx.x;
    s_ch[q] = wgnt::slot_chunk(s);
    s_k[q] = kc0 + wgnt::slot_row(s);
    s_pos[q] = wgnt::pos_from_k(g, s_k[q]);
#pragma unroll
    for (int sb = 0; sb < NSUB; ++sb)
      s_col[q][sb] = wgnt::col_from_n(g, n0 + sb * 64 + s_ch[q] * 8);
  }

#define NT_LOAD(src_, dst_)                                                    \
  __builtin_amdgcn_global_load_lds(                                            \
      (const __attribute__((address_space(1))) void*)(src_),                   \
      (__attribute__((address_space(3))) void*)(dst_), 16, 0, 0)

#define NT_STAGE(buf_)                                                         \
  do {                                                                         \
    _Pragma("unroll")                                                          \
    for (int q = 0; q < 2; ++q) {                                              \
      const long ao = wgnt::a_src(g, s_pos[q], s_k[q], s_ch[q]);                         \
      const bf16* asrc = ao == wgnt::kZeroPage ? zpage : dYt + ao;             \
      NT_LOAD(asrc, &lds_a[buf_][(q * 256 + wave * 64) * 8]);                  \
      _Pragma("unroll")                                                        \
      for (int sb = 0; sb < NSUB; ++sb) {                                      \
        const long bo = wgnt::b_src(g, s_pos[q], s_k[q], s_col[q][sb]);        \
        const bf16* bsrc = bo == wgnt::kZeroPage ? zpage : Xt + bo;            \
        NT_LOAD(bsrc, &lds_b[buf_][sb][(q * 256 + wave * 64) * 8]);            \
      }                                                                        \
    }                                                                          \
  } while (0)

#define NT_ADVANCE()                                                           \
  do {                                                                         \
    _Pragma("unroll")                                                          \
    for (int q = 0; q < 2; ++q) {                                              \
      s_k[q] += wgnt::kRows;                                                   \
      wgnt::pos_advance(g, s_pos[q]);                                          \
    }                                                                          \
  } while (0)

  f32x4 acc[NSUB][MT];
#pragma unroll
  for (int sb = 0; sb < NSUB; ++sb)
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[sb][i] = {0.f, 0.f, 0.f, 0.f};

  // ones column (bias): global column g.N9, if this block holds it
  const int ones_col = (bias_mode == NT_BIAS_ONES) ? g.N9 : -1;
  // columns this block must compute (wave-uniform skip of empty sub-tiles)
  const int ncols = g.N9 + (bias_mode == NT_BIAS_ONES ? 1 : 0);
  bool sb_active[NSUB], sb_ones[NSUB];
#pragma unroll
  for (int sb = 0; sb < NSUB; ++sb) {
    const int nsub0 = n0 + (sb * 4 + wave) * 16;
    sb_active[sb] = nsub0 < ncols;
    sb_ones[sb] = nsub0 + fr == ones_col;
  }
  const bool do_colsum = (bias_mode == NT_BIAS_COLSUM) && (blockIdx.x == 0);
  float db_acc = 0.f;
  const int db_f = threadIdx.x & 63;
  const int db_q = threadIdx.x >> 6;

  NT_STAGE(0);
  __syncthreads();
  int buf = 0;
  for (long k0 = kc0; k0 < kc_end; k0 += wgnt::kRows) {
    NT_ADVANCE();
    if (k0 + wgnt::kRows < kc_end) NT_STAGE(buf ^ 1);
    const short* la = lds_a[buf];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 afrag[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const bf16x4v a0 = lds_read_tr(la + wgnt::tr_idx(lane, ks, 0, mt));
        const bf16x4v a1 = lds_read_tr(la + wgnt::tr_idx(lane, ks, 1, mt));
        afrag[mt] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      }
#pragma unroll
      for (int sb = 0; sb < NSUB; ++sb) {
        if (!sb_active[sb]) continue;  // wave-uniform
        const short* lb = lds_b[buf][sb];
        const bf16x4v b0 = lds_read_tr(lb + wgnt::tr_idx(lane, ks, 0, wave));
        const bf16x4v b1 = lds_read_tr(lb + wgnt::tr_idx(lane, ks, 1, wave));
        bf16x8 bfrag = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
        if (sb_ones[sb]) {
          const short one = 0x3F80;  // bf16 1.0
          bfrag = {one, one, one, one, one, one, one, one};
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[sb][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[mt], bfrag, acc[sb][mt], 0, 0, 0);
      }
    }
    if (do_colsum && db_f < F) {
#pragma unroll
      for (int kk = db_q * 16; kk < db_q * 16 + 16; ++kk) {
        db_acc += __bfloat162float(__hip_bfloat16(__hip_bfloat16_raw{
            (unsigned short)la[wgnt::lds_idx(kk, db_f)]}));
      }
    }
    __syncthreads();
    buf ^= 1;
  }
#undef NT_STAGE
#undef NT_ADVANCE
#undef NT_LOAD

  if (do_colsum) {
    __shared__ float db_lds[4][64];
    db_lds[db_q][db_f] = db_acc;
    __syncthreads();
    if (db_q == 0 && db_f < F) {
      const float v = db_lds[0][db_f] + db_lds[1][db_f] + db_lds[2][db_f] +
                      db_lds[3][db_f];
      if (DET) {
        dBacc[((long)t * gridDim.y + blockIdx.y) * F + db_f] = v;
      } else {
        atomicAdd(&dBacc[(long)t * F + db_f], v);
      }
    }
  }

  const long sl = DET ? (long)t * gridDim.y + blockIdx.y : (long)t;
  float* dWt = dWacc + sl * 9 * Cout * F;
  float* dBt = dBacc ? dBacc + sl * F : nullptr;
#pragma unroll
  for (int sb = 0; sb < NSUB; ++sb) {
    const int n = n0 + (sb * 4 + wave) * 16 + fr;
    const int orow = wgnt::out_row(g, n, Cout);
    float* dst = nullptr;  // f = 0 of this lane's column
    if (orow >= 0) dst = dWt + (long)orow * F;
    else if (n == ones_col) dst = dBt;
    if (dst == nullptr) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = mt * 16 + fk * 4 + j;
        if (f < F) {
          if (DET) {
            dst[f] = acc[sb][mt][j];
          } else {
            atomicAdd(&dst[f], acc[sb][mt][j]);
          }
        }
      }
    }
  }
}

// dy [T, NB, Ho, Wo, F] bf16 ; x [T, NB, H, W, C] bf16
// -> {dw [T, F, C, 3, 3] fp32, db [T, F] fp32}; same contract as
// tconv_wgrad_v2.  Needs F % 8 == 0, F <= 64 and C % 8 == 0 or C in {1, 3}.
std::vector<torch::Tensor> tconv_wgrad_v3(torch::Tensor dy, torch::Tensor x,
                                          long pad, bool with_bias) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda());
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
              x.scalar_type() == torch::kBFloat16);
  auto dyc = dy.contiguous();
  auto xc = x.contiguous();
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int Ho = (int)dy.size(2), Wo = (int)dy.size(3), F = (int)dy.size(4);
  TORCH_CHECK(F % 8 == 0 && F <= 64, "wgrad_v3 needs F % 8 == 0, F <= 64");
  TORCH_CHECK(C % 8 == 0 || C == 1 || C == 3,
              "wgrad_v3 needs C % 8 == 0 or C in {1, 3}");
  TORCH_CHECK(dy.size(0) == T && dy.size(1) == NB &&
              Ho == H + 2 * pad - 2 && Wo == W + 2 * pad - 2 &&
              Ho >= 1 && Wo >= 1 && pad >= 0 && pad <= 2,
              "wgrad_v3: dy/x shapes do not match a 3x3 stride-1 conv");
  const bool det = deterministic_mode();
  auto stream = at::cuda::getCurrentCUDAStream();

  // first layer: pad the channels to one 16-byte chunk
  int Cp = C;
  if (C % 8 != 0) {
    Cp = 8;
    const long M = (long)T * NB * H * W;
    auto xp = torch::empty({T, NB, H, W, 8}, x.options());
    hipLaunchKernelGGL(nt_chpad8_kernel,
                       dim3((unsigned)std::min<long>((M + 255) / 256, 65536)),
                       dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const bf16*>(xc.data_ptr()),
                       reinterpret_cast<bf16*>(xp.data_ptr()), M, C);
    xc = xp;
  }
  // Deterministic mode keeps, bit for bit, the sums of the v2 / v1 routing
  // it replaces (deterministic results do not move with the kernel
  // generation): the same reduction index — v2 pads every line to Wo8 from
  // 30 000 positions up, v1 below is flat —, the same K-chunks, the same
  // column-sum bias.  Zero rows add nothing, a column's accumulator does not
  // depend on its neighbours, and the k -> MFMA-lane map is theirs, so every
  // fp32 operation is the one v2 / v1 performs.  wgplan::v3 takes that
  // plan's line width and K-chunks from wgplan::v2 / v1 themselves.
  //
  // 128-column blocks stage dY half as often (once for the first layer's
  // 72 columns) but halve the grid and drop occupancy 4 -> 3 blocks/CU:
  // measured ahead (x1.06 - x1.46) from T * K of about 6e5 positions up,
  // behind (x0.57 - x0.90) below (profiles/README.md).  Env
  // MAML355_WGRAD_NSUB overrides for A/B.
  const char* v2_env = getenv("MAML355_WGRAD_V2");
  const wgplan::Plan p =
      wgplan::v3(T, NB, Ho, Wo, C, with_bias, det,
                 !(v2_env && v2_env[0] == '0'), wgrad_nsub_override());
  const wgnt::Geom g =
      wgnt::make_geom(NB, H, W, Cp, Ho, Wo, F, (int)pad, p.Wk);
  TORCH_CHECK(p.gridy <= 65535 && T <= 65535, "wgrad_v3: grid too large");
  auto fopt = x.options().dtype(torch::kFloat32);
  auto acc = torch::zeros({T, p.nslices, 9 * C, F}, fopt);
  auto dbacc = torch::zeros({T, p.nslices, F}, fopt);
  const bf16* zpage = conv_zero_page(x);
  dim3 grid((unsigned)p.gridx, (unsigned)p.gridy, T);
#define LAUNCH_NT(NS_, MT_, DET_)                                              \
  hipLaunchKernelGGL((tconv_wgrad_nt_kernel<NS_, MT_, DET_>), grid, dim3(256), \
                     0, stream.stream(),                                       \
                     reinterpret_cast<const bf16*>(dyc.data_ptr()),            \
                     reinterpret_cast<const bf16*>(xc.data_ptr()), zpage,      \
                     acc.data_ptr<float>(),                                    \
                     with_bias ? dbacc.data_ptr<float>() : nullptr, g, C,      \
                     p.Kr, p.kchunk, p.bias)
#define LAUNCH_NT_MT(NS_, DET_)                                                \
  switch ((F + 15) / 16) {                                                     \
    case 1: LAUNCH_NT(NS_, 1, DET_); break;                                    \
    case 2: LAUNCH_NT(NS_, 2, DET_); break;                                    \
    case 3: LAUNCH_NT(NS_, 3, DET_); break;                                    \
    default: LAUNCH_NT(NS_, 4, DET_); break;                                   \
  }
  if (p.nsub == 2) {
    if (det) LAUNCH_NT_MT(2, true) else LAUNCH_NT_MT(2, false)
  } else {
    if (det) LAUNCH_NT_MT(1, true) else LAUNCH_NT_MT(1, false)
  }
#undef LAUNCH_NT_MT
#undef LAUNCH_NT
  return finish_wgrad(acc, dbacc, T, F, C, p.nslices, stream.stream());
}
