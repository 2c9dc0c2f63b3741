// Wide-channel bf16 task-batched STRIDE-2 3x3 convolution trio (fwd / dgrad /
// wgrad) for 65..256 channels on v_mfma_f32_16x16x32_bf16 — the convs of the
// max_pooling=False backbone above 64 filters, where sconv.hip (stride 2, up
// to 64 channels) and wconv.hip (65..256 channels, stride 1) both stop:
//
//   fwd   : Y[t]  = im2col_s2(X[t]) @ Wp[t]      M=NB*Ho*Wo, N=F, K=9*C
//           gather iy = 2*oy + ky - p, ix = 2*ox + kx - p.  Odd H with p = 1
//           reads iy = H on the last output row, so all four edges are
//           predicated; loads outside the image yield zeros.
//   dgrad : dX[iy,ix,c] = sum dY[(iy+p-ky)/2, (ix+p-kx)/2, f] * W[f,c,ky,kx]
//           over the taps whose divisions are exact.  The pixels are split by
//           the parity of (iy+p, ix+p) into four dense implicit GEMMs over
//           their own tap subsets (4, 2, 2, 1 taps; K = taps * F) — ONE
//           launch, parity and column tile packed into blockIdx.y.  No
//           zero-dilated dY (about 4x the MFMA work, spent on zeros).  Every
//           pixel of dX belongs to exactly one class and is stored by it; the
//           pixels no output touches (trailing row / column at p = 0 with even
//           H / W) see only out-of-range taps and come out exactly zero.
//   wgrad : dW[t] = dY[t]^T @ im2col_s2(X[t])    split-K over the NB*Ho*Wo
//           OUTPUT positions, private slice per K-chunk + ordered finalize,
//           db fused.  The chunks are wgplan::wconv's, called with Ho, Wo.
//
// Numerics contract = wconv.hip: activations [T, NB, H, W, C] bf16, weights
// [T, F, C, 3, 3] fp32 rounded to bf16 once by the repack, bias [T, F] fp32,
// fp32 MFMA accumulation, bias added in fp32, one rounding to bf16 at the
// store of y / dx; dw and db fp32.  C % 8 == 0 and F % 8 == 0, so every
// 16-byte chunk (8 channels) is inside one tap and wholly valid or wholly
// absent.  No floating-point atomics and no data-dependent order anywhere:
// all three ops are bitwise run-to-run reproducible in every mode.
//
// Weights: both GEMM kernels read wconv_repack's [T, 9, Co, Ci] images as
// they stand, no repack of its own.  fwd reads wconv_repack(w, false)
// ([T, 9, F, C]) at tap ky*3+kx.  dgrad reads wconv_repack(w, true)
// ([T, 9, C, F], which stores W[f][c][ky][kx] at tap (2-ky)*3+(2-kx)): the
// parity kernels index taps directly, so they address that image at
// 8 - (ky*3+kx).
//
// Tiling = wconv.hip's (128 x 128 blocks, four waves with 4 x 4 accumulators,
// 32-channel K-steps inside one tap, k-contiguous LDS rows at the 80-byte
// conflict-free stride, register staging with the next step's loads issued
// ahead of the MFMAs); geometry = sconv.hip's.  What is new is their product:
// the stride-2 gather and the parity classes on the wide tile, and the
// stride-2 gather under the transposing-read wgrad.
//
// Resources (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage):
//
//   kernel                         VGPRs  AGPRs  SGPRs  LDS bytes  waves/SIMD
//   swconv_mm_kernel<false> (fwd)    136     64     71      20480           2
//   swconv_mm_kernel<true> (dgrad)   136     64     81      20480           2
//   swconv_wgrad_kernel              100     64     70      18944           3
//   swconv_wgrad_finalize_kernel      23      0     58          0           8
//
// Scratch 0 bytes and no VGPR or SGPR spills in every instantiation; the
// AGPRs are the 4 x 4 accumulators.

#include "common.h"
#include "wgrad_plan.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;
typedef short bf16x4v __attribute__((ext_vector_type(4)));

DEVINL short f2bf(float v) {
  return (short)__hip_bfloat16_raw(__float2bfloat16(v)).x;
}
DEVINL float bf2f(short v) {
  return __bfloat162float(__hip_bfloat16(__hip_bfloat16_raw{(unsigned short)v}));
}

}  // namespace

// ---------------------------------------------------------------------------
// fwd / dgrad kernel: D[t] rows = gather(S[t]) @ Wp[t].
//   S  [T, NB, Hs, Ws, Ci]  (fwd: X; dgrad: dY)
//   Wp [T, 9, Co, Ci]       (wconv_repack; fwd plain, dgrad flipped)
//   D  [T, NB, Hd, Wd, Co]  (fwd: Y; dgrad: dX)
//
// Every GEMM row m is an output pixel with a base source coordinate
// (r_h, r_w); every K-step is 32 channels of one tap, with a source offset
// (dh, dw) and a weight tap.
//   fwd  : base = 2 * o - p, offset = +(ky, kx), weight tap ky*3+kx.
//   dgrad: class (py, px) holds the pixels iy = h0 + 2 j with h0 = py ^ p
//          (so iy + p has parity py); base a = (h0 + p - py) / 2 + j; the
//          taps ky = py ? {1} : {0, 2} read oy = a - ky / 2.  cnt = number
//          of such pixels per image side; M = NB * cntH * cntW differs per
//          class, the launch covers the largest one, and a block past its
//          class's M returns before any barrier (block-uniform).
//
// Block = 256 threads = 4 waves, tile SW_M = 128 pixels x SW_N = 128 output
// channels, K-step SW_K = 32.  Grid (ceil(M/128), column tiles [x 4
// parities], T).  Wave (wm, wn) of the 2 x 2 arrangement owns pixels
// [64 wm, +64) and channels [64 wn, +64): 4 x 4 accumulators.  16-column
// tiles past Co are skipped (wave-uniform).
//
// LDS: A (gathered source) as [pixel][k], B (weights) as [channel][k], both
// k-contiguous, row stride SW_LD = 40 bf16 (32 + 8 of padding, 80 bytes):
// 2 x 10 KB.  A fragment is one ds_read_b128 per lane: row lane&15, k =
// 8 * (lane>>4) .. +7, the MFMA's operand layout as it stands.  80 bytes =
// 20 dwords and 20 r mod 64 for r = 0..15 are the sixteen distinct multiples
// of 4, so the 16 rows of a lane group cover all 64 banks once.
//
// The MFMA takes the WEIGHT fragment as its row operand, so the accumulator
// holds D[channel = 4 * (lane>>4) + j][pixel = lane&15]: a lane owns 4
// consecutive channels of one pixel and stores them as one 8-byte write.
//
// Staging: thread -> fixed 8-channel chunk (tid & 3) and rows tid>>2 and
// tid>>2 + 64 of both tiles; its two pixel decodes live in registers for the
// whole K loop.  Rows past M, channels past Ci, taps outside the source and
// columns past Co load nothing and stage zeros.
// ---------------------------------------------------------------------------
#define SW_M 128
#define SW_N 128
#define SW_K 32
#define SW_LD 40

template <bool DGRAD>
__global__ __launch_bounds__(256)
void swconv_mm_kernel(const short* __restrict__ S, const short* __restrict__ Wp,
                      const float* __restrict__ bias, short* __restrict__ D,
                      int NB, int Hs, int Ws, int Ci, int Hd, int Wd, int Co,
                      int pad, int ncol) {
  const int t = blockIdx.z;
  int cb = blockIdx.y;
  int py = 0, px = 0, h0 = 0, w0 = 0, ah = 0, aw = 0;
  int cntH = Hd, cntW = Wd, nkx = 3, ntaps = 9;
  if (DGRAD) {
    const int par = (int)blockIdx.y / ncol;
    cb = (int)blockIdx.y - par * ncol;
    py = par >> 1;
    px = par & 1;
    h0 = py ^ pad;
    w0 = px ^ pad;
    cntH = Hd > h0 ? (Hd - h0 + 1) / 2 : 0;
    cntW = Wd > w0 ? (Wd - w0 + 1) / 2 : 0;
    ah = (h0 + pad - py) / 2;
    aw = (w0 + pad - px) / 2;
    nkx = px ? 1 : 2;
    ntaps = (py ? 1 : 2) * nkx;
  }
  const long Mtot = (long)NB * cntH * cntW;
  const long m0 = (long)blockIdx.x * SW_M;
  if (m0 >= Mtot) return;  // block-uniform: the smaller parity classes
  const int co0 = cb * SW_N;

  __shared__ __attribute__((aligned(16))) short lds_a[SW_M * SW_LD];
  __shared__ __attribute__((aligned(16))) short lds_b[SW_N * SW_LD];

  const short* St = S + (long)t * NB * Hs * Ws * Ci;
  const short* Wt = Wp + (long)t * 9 * Co * Ci;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int fr = lane & 15;
  const int fk = lane >> 4;
  const int wm = wave >> 1;
  const int wn = wave & 1;

  // this thread's staging chunk and its two rows (registers, decoded once)
  const int sq = (tid & 3) * 8;
  const int sr = tid >> 2;
  int r_n[2], r_h[2], r_w[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long mg = m0 + sr + 64 * i;
    if (mg < Mtot) {
      const int jw = (int)(mg % cntW);
      const int jh = (int)((mg / cntW) % cntH);
      r_n[i] = (int)(mg / ((long)cntW * cntH));
      r_h[i] = DGRAD ? ah + jh : 2 * jh - pad;
      r_w[i] = DGRAD ? aw + jw : 2 * jw - pad;
    } else {
      r_n[i] = -1; r_h[i] = 0; r_w[i] = 0;
    }
  }

  bool live[4];  // this wave's 16-channel tiles that hold a channel < Co
#pragma unroll
  for (int j = 0; j < 4; ++j) live[j] = co0 + wn * 64 + j * 16 < Co;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int ksteps = (Ci + SW_K - 1) / SW_K;
  const int nsteps = ntaps * ksteps;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // global -> register half of the staging for K-step s; a step past the
  // last one stages zeros (and is never consumed)
  bf16x8 va[2], vb[2];
  auto load_step = [&](int s) {
    const int tap = s / ksteps;
    const int c = (s - tap * ksteps) * SW_K + sq;
    int dh, dw, wtap;
    if (DGRAD) {
      const int tky = tap / nkx, tkx = tap - tky * nkx;
      const int ky = py ? 1 : 2 * tky, kx = px ? 1 : 2 * tkx;
      dh = -tky;
      dw = -tkx;
      wtap = 8 - (ky * 3 + kx);  // the flipped image, see the header
    } else {
      dh = tap / 3;
      dw = tap % 3;
      wtap = tap;
    }
    const bool kok = s < nsteps && c < Ci;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      bf16x8 v = zero8;
      const int h = r_h[i] + dh, w = r_w[i] + dw;
      if (kok && r_n[i] >= 0 && h >= 0 && h < Hs && w >= 0 && w < Ws) {
        v = *(const bf16x8*)&St[(((long)r_n[i] * Hs + h) * Ws + w) * Ci + c];
      }
      va[i] = v;
      const int co = co0 + sr + 64 * i;
      bf16x8 u = zero8;
      if (kok && co < Co) {
        u = *(const bf16x8*)&Wt[((long)wtap * Co + co) * Ci + c];
      }
      vb[i] = u;
    }
  };

  load_step(0);
  for (int s = 0; s < nsteps; ++s) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *(bf16x8*)&lds_a[(sr + 64 * i) * SW_LD + sq] = va[i];
      *(bf16x8*)&lds_b[(sr + 64 * i) * SW_LD + sq] = vb[i];
    }
    __syncthreads();
    // prefetch: the next K-step's global loads fly under this step's MFMAs
    load_step(s + 1);

    bf16x8 af[4], bfr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[i] = *(const bf16x8*)&lds_a[(wm * 64 + i * 16 + fr) * SW_LD + fk * 8];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bfr[j] = *(const bf16x8*)&lds_b[(wn * 64 + j * 16 + fr) * SW_LD + fk * 8];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!live[j]) continue;  // wave-uniform
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            bfr[j], af[i], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();  // all waves done reading before the next staging
  }

  // epilogue: D row = channel 4 * fk + e, D column = pixel fr; bias added in
  // fp32, one rounding, 4 channels per 8-byte store.  dgrad scatters its
  // class's pixels to (h0 + 2 jh, w0 + 2 jw).
  short* Dt = D + (long)t * NB * Hd * Wd * Co;
  long pix[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long mg = m0 + wm * 64 + i * 16 + fr;
    pix[i] = -1;
    if (mg < Mtot) {
      if (DGRAD) {
        const int jw = (int)(mg % cntW);
        const long q = mg / cntW;
        const int jh = (int)(q % cntH);
        const long n = q / cntH;
        pix[i] = (n * Hd + h0 + 2 * jh) * Wd + w0 + 2 * jw;
      } else {
        pix[i] = mg;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = co0 + wn * 64 + j * 16 + fk * 4;
    if (co >= Co) continue;  // Co % 8 == 0: the four channels stand together
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias != nullptr) {
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = bias[(long)t * Co + co + e];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (pix[i] < 0) continue;
      bf16x4v o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(acc[i][j][e] + bv[e]);
      *(bf16x4v*)&Dt[pix[i] * Co + co] = o;
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad kernel: slice[t][chunk][n = (tap, c)][f] = sum over the chunk's
// OUTPUT positions k of dY[t,k,f] * im2col_s2(X)[t,k,n]; dbslice = sum_k dY.
//   dY [T, NB, Ho, Wo, F] ; X [T, NB, H, W, C]
// Structure = wconv_wgrad_kernel: 256 threads = 4 waves over a 128-tile of F
// and a 128-tile of the 9C columns, wave (wf, wn) owns a 64 x 64 quarter
// (4 x 4 accumulators).  Grid (F tiles * column tiles, K-chunks, T); every
// (t, chunk) block stores a PRIVATE slice with plain stores and
// swconv_wgrad_finalize_kernel sums the slices in chunk order.
//
// Both operands are staged AS STORED in 16-byte chunks: dY tile [k][f] and
// im2col tile [k][n], SWG_K = 32 positions per K-step, row stride SWG_LD =
// 144 bf16 (288 bytes = 8 dwords mod 64: the eight consecutive rows a
// 32-lane half reads start at banks 0, 8, .., 56 — conflict-free): 2 x 9 KB.
// The X row of output position (ho, wo) and column (tap, c) is the pixel
// (2 ho + ky - p, 2 wo + kx - p), under the four-edge predicate.  The
// transpose happens in the LDS read, ds_read_b64_tr_b16: lane group g =
// lane>>4 reads rows 4g..4g+3 and 16 + 4g..+3, the same permutation of the
// step's k on both operands, so the product is unchanged.
//
// The bias gradient is the ordered column sum of the staged dY tiles, from
// column-block 0 only.
// ---------------------------------------------------------------------------
#define SWG_F 128
#define SWG_N 128
#define SWG_K 32
#define SWG_LD 144
static_assert(SWG_K == wgplan::kStepWide && SWG_N == wgplan::kTileWide &&
                  SWG_F == wgplan::kTileWide,
              "wgrad_plan.h cuts K-chunks for these tiles");

__global__ __launch_bounds__(256)
void swconv_wgrad_kernel(const short* __restrict__ dY,
                         const short* __restrict__ X,
                         float* __restrict__ dWsl,  // [T, nsl, 9C, F]
                         float* __restrict__ dBsl,  // [T, nsl, F] or nullptr
                         int NB, int H, int W, int C, int Ho, int Wo, int F,
                         int pad, int kchunk, int fblk) {
  const int t = blockIdx.z;
  const int fb = blockIdx.x % fblk;
  const int nb = blockIdx.x / fblk;
  const int f0 = fb * SWG_F;
  const int n0 = nb * SWG_N;
  const int N9 = 9 * C;
  const long Ktot = (long)NB * Ho * Wo;
  const long kc0 = (long)blockIdx.y * kchunk;
  const long kc_end = min(kc0 + (long)kchunk, Ktot);

  __shared__ __attribute__((aligned(16))) short lds_a[SWG_K * SWG_LD];  // dY [k][f]
  __shared__ __attribute__((aligned(16))) short lds_b[SWG_K * SWG_LD];  // col [k][n]
  __shared__ float db_lds[SWG_F];

  const short* dYt = dY + (long)t * Ktot * F;
  const short* Xt = X + (long)t * NB * H * W * C;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int fr = lane & 15;
  const int fk = lane >> 4;
  const int wf = wave >> 1;
  const int wn = wave & 1;

  // this thread's column chunk of each tile, decoded once
  const int cc = (tid & 15) * 8;
  const int sr = tid >> 4;
  const int a_f = f0 + cc;
  const bool a_ok = a_f < F;
  const int b_n = n0 + cc;
  const bool b_ok = b_n < N9;
  const int b_tap = b_ok ? b_n / C : 0;
  const int b_c = b_ok ? b_n - b_tap * C : 0;
  const int b_dy = b_tap / 3 - pad;
  const int b_dx = b_tap % 3 - pad;

  bool live_f[4], live_n[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    live_f[i] = f0 + wf * 64 + i * 16 < F;
    live_n[i] = n0 + wn * 64 + i * 16 < N9;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // fused bias grad: thread -> column tid & 127, rows 16 * (tid>>7)..
  const bool do_bias = (dBsl != nullptr) && (nb == 0);
  float db_acc = 0.f;
  const int db_f = tid & 127;
  const int db_h = tid >> 7;

  // The two staging rows of this thread advance by SWG_K output positions
  // per K-step: decode (wo, ho, img) once, then step it with carries.
  // dho < Ho and one carry keep ho below 2 * Ho.
  const int s_dwo = SWG_K % Wo;
  const int s_dho = (SWG_K / Wo) % Ho;
  const int s_dimg = (SWG_K / Wo) / Ho;
  int p_k[2], p_wo[2], p_ho[2], p_img[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int k = (int)kc0 + sr + 16 * i;
    p_k[i] = k;
    p_wo[i] = k % Wo;
    p_ho[i] = (k / Wo) % Ho;
    p_img[i] = (k / Wo) / Ho;
  }
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // global -> register half of the staging for the next K-step; rows past
  // the chunk end load nothing and stage zeros
  bf16x8 vy[2], vx[2];
  auto load_step = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long k = p_k[i];
      bf16x8 y8 = zero8, x8 = zero8;
      if (k < kc_end) {
        if (a_ok) y8 = *(const bf16x8*)&dYt[k * F + a_f];
        const int h = 2 * p_ho[i] + b_dy, w = 2 * p_wo[i] + b_dx;
        if (b_ok && h >= 0 && h < H && w >= 0 && w < W) {
          x8 = *(const bf16x8*)&Xt[(((long)p_img[i] * H + h) * W + w) * C + b_c];
        }
      }
      vy[i] = y8;
      vx[i] = x8;
      // advance this row to the next K-step
      p_k[i] += SWG_K;
      p_wo[i] += s_dwo;
      const int cw = p_wo[i] >= Wo;
      p_wo[i] -= cw ? Wo : 0;
      p_ho[i] += s_dho + cw;
      const int ch = p_ho[i] >= Ho;
      p_ho[i] -= ch ? Ho : 0;
      p_img[i] += s_dimg + ch;
    }
  };

  // transposing read: this lane's address inside a 16-column block of a
  // tile, for the row block h (0: rows 4 fk.., 1: rows 16 + 4 fk..)
  const int tr_lane = (fk * 4 + ((lane >> 2) & 3)) * SWG_LD + (lane & 3) * 4;
  auto read_tr = [&](const short* tile, int cblk) {
    const short* p0 = tile + tr_lane + cblk * 16;
    const bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) bf16x4v*)p0);
    const bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) bf16x4v*)(p0 + 16 * SWG_LD));
    const bf16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return r;
  };

  load_step();
  for (long k0 = kc0; k0 < kc_end; k0 += SWG_K) {
    __syncthreads();  // previous K-step's reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *(bf16x8*)&lds_a[(sr + 16 * i) * SWG_LD + cc] = vy[i];
      *(bf16x8*)&lds_b[(sr + 16 * i) * SWG_LD + cc] = vx[i];
    }
    __syncthreads();
    // prefetch: the next K-step's global loads fly under this step's MFMAs
    load_step();

    bf16x8 af[4], bfr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = read_tr(lds_a, wf * 4 + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) bfr[j] = read_tr(lds_b, wn * 4 + j);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!live_n[j]) continue;  // wave-uniform
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!live_f[i]) continue;  // wave-uniform
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    }
    if (do_bias) {
#pragma unroll
      for (int kk = db_h * 16; kk < db_h * 16 + 16; ++kk) {
        db_acc += bf2f(lds_a[kk * SWG_LD + db_f]);
      }
    }
  }
  if (do_bias) {  // block-uniform
    if (db_h == 1) db_lds[db_f] = db_acc;
    __syncthreads();
    if (db_h == 0 && f0 + db_f < F) {
      dBsl[((long)t * gridDim.y + blockIdx.y) * F + f0 + db_f] =
          db_acc + db_lds[db_f];
    }
  }

  // C/D: row = f (4 * fk + e), column = n (fr).  Tiles are disjoint, so the
  // (t, chunk) slice is written exactly once; 4 consecutive f per store.
  float* dWt = dWsl + ((long)t * gridDim.y + blockIdx.y) * N9 * F;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn * 64 + j * 16 + fr;
    if (n >= N9) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = f0 + wf * 64 + i * 16 + fk * 4;
      if (f >= F) continue;  // F % 8 == 0: the four rows stand together
      *(f32x4*)&dWt[(long)n * F + f] = acc[i][j];
    }
  }
}

// slices [T, nsl, 9C, F] -> dW [T, F, C, 3, 3]; dbsl [T, nsl, F] -> db [T, F].
// Slices are summed in chunk order: the one, fixed reduction order.
__global__ void swconv_wgrad_finalize_kernel(const float* __restrict__ sl,
                                             const float* __restrict__ dbsl,
                                             float* __restrict__ dw,
                                             float* __restrict__ db,
                                             int T, int F, int C, int nsl) {
  const long total = (long)T * F * C * 9;
  const long ssz = (long)9 * C * F;
  const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long i = first; i < total; i += grid_stride()) {
    long r = i;
    const int kx = (int)(r % 3); r /= 3;
    const int ky = (int)(r % 3); r /= 3;
    const int c = (int)(r % C); r /= C;
    const int f = (int)(r % F); r /= F;
    const long t = r;
    const long e = ((long)(ky * 3 + kx) * C + c) * F + f;
    float v = 0.f;
    for (int s = 0; s < nsl; ++s) v += sl[(t * nsl + s) * ssz + e];
    dw[i] = v;
  }
  if (dbsl) {
    for (long i = first; i < (long)T * F; i += grid_stride()) {
      const long t = i / F;
      const int f = (int)(i % F);
      float v = 0.f;
      for (int s = 0; s < nsl; ++s) v += dbsl[(t * nsl + s) * F + f];
      db[i] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------
namespace {

bool sw_channels_ok(long a, long b) {
  return a >= 8 && b >= 8 && a % 8 == 0 && b % 8 == 0 && a <= 256 && b <= 256;
}

bool sw_aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

long sw_out_dim(long h, long pad) { return (h + 2 * pad - 3) / 2 + 1; }

}  // namespace

// x [T, NB, H, W, C] bf16 ; wp [T, 9, F, C] bf16 = wconv_repack(w, false) ;
// bias [T, F] fp32 / undef  ->  y [T, NB, Ho, Wo, F] bf16
torch::Tensor swconv_fwd(torch::Tensor x, torch::Tensor wp,
                         c10::optional<torch::Tensor> bias, long pad) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 5 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "swconv_fwd needs bf16");
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 4 && wp.is_contiguous() &&
              wp.scalar_type() == torch::kBFloat16 && wp.size(1) == 9 &&
              wp.device() == x.device());
  TORCH_CHECK(x.size(0) <= 65535, "swconv_fwd: at most 65535 tasks (grid.z)");
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int F = (int)wp.size(2);
  TORCH_CHECK(wp.size(0) == T && wp.size(3) == C, "wp does not match x");
  TORCH_CHECK(sw_channels_ok(C, F),
              "swconv_fwd: channels must be multiples of 8 in 8..256");
  TORCH_CHECK(pad == 0 || pad == 1, "swconv: pad must be 0 or 1");
  TORCH_CHECK(H + 2 * pad >= 3 && W + 2 * pad >= 3, "swconv: input too small");
  const long Ho = sw_out_dim(H, pad), Wo = sw_out_dim(W, pad);
  TORCH_CHECK(sw_aligned16(x) && sw_aligned16(wp), "swconv_fwd: 16-byte alignment");
  auto y = torch::empty({T, NB, Ho, Wo, F}, x.options());
  const long Mtot = (long)NB * Ho * Wo;
  if (T == 0 || Mtot == 0) return y;
  // pixels are decoded and the row grid is cut in 32 bits; every global
  // offset is carried as 64-bit
  TORCH_CHECK(Mtot < (1L << 30) && (long)NB * H * W < (1L << 30),
              "swconv_fwd: too many positions per task");
  TORCH_CHECK(sw_aligned16(y), "swconv_fwd: 16-byte alignment");
  const float* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == torch::kFloat32 &&
                bias->numel() == (long)T * F);
    bc = bias->contiguous();
    bptr = bc.data_ptr<float>();
  }
  const int ncol = (F + SW_N - 1) / SW_N;
  dim3 grid((unsigned)((Mtot + SW_M - 1) / SW_M), (unsigned)ncol, T);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((swconv_mm_kernel<false>), grid, dim3(256), 0,
                     stream.stream(),
                     reinterpret_cast<const short*>(x.data_ptr()),
                     reinterpret_cast<const short*>(wp.data_ptr()), bptr,
                     reinterpret_cast<short*>(y.data_ptr()), NB, H, W, C,
                     (int)Ho, (int)Wo, F, (int)pad, ncol);
  return y;
}

// dy [T, NB, Ho, Wo, F] bf16 ; wp [T, 9, C, F] bf16 = wconv_repack(w, true)
// -> dx [T, NB, H, W, C] bf16.  H, W are explicit: two input sizes map to
// the same Ho under stride 2.  dx is allocated uninitialised; the four
// parity classes together store every pixel.
torch::Tensor swconv_dgrad(torch::Tensor dy, torch::Tensor wp, long pad,
                           long H, long W) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 5 && dy.is_contiguous());
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16, "swconv_dgrad needs bf16");
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 4 && wp.is_contiguous() &&
              wp.scalar_type() == torch::kBFloat16 && wp.size(1) == 9 &&
              wp.device() == dy.device());
  TORCH_CHECK(dy.size(0) <= 65535, "swconv_dgrad: at most 65535 tasks (grid.z)");
  const int T = (int)dy.size(0), NB = (int)dy.size(1), Ho = (int)dy.size(2),
            Wo = (int)dy.size(3), F = (int)dy.size(4);
  const int C = (int)wp.size(2);
  TORCH_CHECK(wp.size(0) == T && wp.size(3) == F, "wp does not match dy");
  TORCH_CHECK(sw_channels_ok(C, F),
              "swconv_dgrad: channels must be multiples of 8 in 8..256");
  TORCH_CHECK(pad == 0 || pad == 1, "swconv: pad must be 0 or 1");
  TORCH_CHECK(H + 2 * pad >= 3 && W + 2 * pad >= 3 &&
              sw_out_dim(H, pad) == Ho && sw_out_dim(W, pad) == Wo,
              "swconv_dgrad: (H, W) inconsistent with dy");
  TORCH_CHECK(sw_aligned16(dy) && sw_aligned16(wp),
              "swconv_dgrad: 16-byte alignment");
  auto dx = torch::empty({T, NB, H, W, C}, dy.options());
  if (T == 0 || NB == 0) return dx;
  TORCH_CHECK((long)NB * H * W < (1L << 30) && (long)NB * Ho * Wo < (1L << 30),
              "swconv_dgrad: too many positions per task");
  TORCH_CHECK(sw_aligned16(dx), "swconv_dgrad: 16-byte alignment");
  // largest parity class: ceil(H/2) x ceil(W/2) pixels per image
  const long Msub = (long)NB * ((H + 1) / 2) * ((W + 1) / 2);
  const int ncol = (C + SW_N - 1) / SW_N;
  dim3 grid((unsigned)((Msub + SW_M - 1) / SW_M), (unsigned)(4 * ncol), T);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((swconv_mm_kernel<true>), grid, dim3(256), 0,
                     stream.stream(),
                     reinterpret_cast<const short*>(dy.data_ptr()),
                     reinterpret_cast<const short*>(wp.data_ptr()), nullptr,
                     reinterpret_cast<short*>(dx.data_ptr()), NB, Ho, Wo, F,
                     (int)H, (int)W, C, (int)pad, ncol);
  return dx;
}

// dy [T, NB, Ho, Wo, F] bf16 ; x [T, NB, H, W, C] bf16
// -> {dw [T, F, C, 3, 3] fp32, db [T, F] fp32 (zeros unless with_bias)}
std::vector<torch::Tensor> swconv_wgrad(torch::Tensor dy, torch::Tensor x,
                                        long pad, bool with_bias) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && dy.dim() == 5 && x.dim() == 5 &&
              dy.device() == x.device());
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
              x.scalar_type() == torch::kBFloat16, "swconv_wgrad needs bf16");
  auto dyc = dy.contiguous();
  auto xc = x.contiguous();
  TORCH_CHECK(x.size(0) <= 65535, "swconv_wgrad: at most 65535 tasks (grid.z)");
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int Ho = (int)dy.size(2), Wo = (int)dy.size(3), F = (int)dy.size(4);
  TORCH_CHECK(dy.size(0) == T && dy.size(1) == NB, "dy does not match x");
  TORCH_CHECK(sw_channels_ok(C, F),
              "swconv_wgrad: channels must be multiples of 8 in 8..256");
  TORCH_CHECK(pad == 0 || pad == 1, "swconv: pad must be 0 or 1");
  TORCH_CHECK(H + 2 * pad >= 3 && W + 2 * pad >= 3 &&
              sw_out_dim(H, pad) == Ho && sw_out_dim(W, pad) == Wo,
              "swconv_wgrad: dy size does not match x and the pad");
  TORCH_CHECK(sw_aligned16(dyc) && sw_aligned16(xc),
              "swconv_wgrad: 16-byte alignment");
  const int N9 = 9 * C;
  const long Ktot = (long)NB * Ho * Wo;
  // positions are stepped in 32 bits; every global offset is 64-bit
  TORCH_CHECK(Ktot < (1L << 30) && (long)NB * H * W < (1L << 30),
              "swconv_wgrad: too many positions per task");
  auto fopts = x.options().dtype(torch::kFloat32);
  auto dw = torch::empty({T, F, C, 3, 3}, fopts);
  auto db = torch::zeros({T, F}, fopts);
  if (T == 0 || Ktot == 0) return {dw.zero_(), db};
  // the wide plan is written in output positions: stride 2 changes Ho, Wo only
  const wgplan::Plan p = wgplan::wconv(T, NB, Ho, Wo, C, F);
  const int nsl = p.nslices;
  const int fblk = (F + SWG_F - 1) / SWG_F;
  TORCH_CHECK(nsl >= 1 && nsl <= 65535 &&
                  p.gridx == fblk * ((N9 + SWG_N - 1) / SWG_N),
              "swconv_wgrad: plan does not match the tiles");
  auto sl = torch::empty({T, nsl, N9, F}, fopts);
  auto dbsl = torch::empty({T, nsl, F}, fopts);
  TORCH_CHECK(sw_aligned16(sl), "swconv_wgrad: 16-byte alignment");
  dim3 grid((unsigned)p.gridx, (unsigned)nsl, T);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(swconv_wgrad_kernel, grid, dim3(256), 0, stream.stream(),
                     reinterpret_cast<const short*>(dyc.data_ptr()),
                     reinterpret_cast<const short*>(xc.data_ptr()),
                     sl.data_ptr<float>(),
                     with_bias ? dbsl.data_ptr<float>() : nullptr, NB, H, W, C,
                     Ho, Wo, F, (int)pad, p.kchunk, fblk);
  const long total = (long)T * F * C * 9;
  hipLaunchKernelGGL(swconv_wgrad_finalize_kernel, dim3(ew_grid(total)),
                     dim3(256), 0, stream.stream(), sl.data_ptr<float>(),
                     with_bias ? dbsl.data_ptr<float>() : nullptr,
                     dw.data_ptr<float>(), db.data_ptr<float>(), T, F, C, nsl);
  return {dw, db};
}
