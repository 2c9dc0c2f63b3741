// Wide-channel bf16 task-batched stride-1 3x3 convolution trio (fwd / dgrad /
// wgrad) for 65..256 channels on v_mfma_f32_16x16x32_bf16 — the backend that
// takes over where tconv.hip / wgrad_nt.hip stop (64 channels):
//
//   fwd   : Y[t]  = im2col(X[t])  @ Wp[t]       M=NB*Ho*Wo, N=Co, K=9*Ci
//   dgrad : dX[t] = im2col(dY[t]) @ Wp_flip[t]  (SAME kernel; weights
//           repacked flipped+transposed, im2col pad' = 2 - pad)
//   wgrad : dW[t] = dY[t]^T @ im2col(X[t])      split-K over positions,
//           private slice per K-chunk + ordered finalize, db fused
//
// Activations [T, NB, H, W, C] bf16, weights [T, F, C, 3, 3] fp32 rounded to
// bf16 by the repack, bias [T, F] fp32.  Numerics as tconv.hip: bf16
// operands, fp32 MFMA accumulation, bias added in fp32, one rounding to bf16
// at the store of y / dx; dw and db fp32.  C % 8 == 0 and F % 8 == 0, so every
// 16-byte chunk (8 channels) is inside one tap and either wholly valid or
// wholly absent.
//
// What is its own here is the output-column dimension: with up to 256 output
// channels a 64-column block would stage the im2col operand four times, so
// the blocks are 128 x 128 and each of the four waves owns a 64 x 64 quarter
// (4 x 4 accumulators, 64 VGPRs).  The pipelining is the plain one of
// fconv.hip: both tiles go through registers between two barriers, with
// bounds-checked loads that yield zeros outside the image, past the M / K
// tails and past the last column — no zero page, no padded input copy — and
// the global loads of K-step k+1 are issued before the MFMAs of step k.
// No floating-point atomics anywhere: every reduction order is fixed, so all
// three ops are bitwise run-to-run reproducible in every mode.

#include "common.h"
#include "wgrad_plan.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

namespace {

using bf16 = __hip_bfloat16;
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
// Weight repack: W [T, F, C, 3, 3] fp32 -> Wp [T, 9, Co, Ci] bf16, the
// reduction channel innermost so a B-tile row (one output column, 32
// channels of one tap) is four 16-byte loads:
//   fwd  : Wp[t][ky*3+kx][f][c]         = W[t][f][c][ky][kx]   (Co=F, Ci=C)
//   dgrad: Wp[t][(2-ky)*3+(2-kx)][c][f] = W[t][f][c][ky][kx]   (Co=C, Ci=F)
// ---------------------------------------------------------------------------
__global__ void wconv_repack_kernel(const float* __restrict__ w,
                                    short* __restrict__ wp,
                                    int T, int F, int C, bool flip) {
  const long total = (long)T * F * C * 9;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += grid_stride()) {
    long r = i;
    const int kx = (int)(r % 3); r /= 3;
    const int ky = (int)(r % 3); r /= 3;
    const int c = (int)(r % C); r /= C;
    const int f = (int)(r % F); r /= F;
    const long t = r;
    long o;
    if (!flip) {
      o = ((t * 9 + (long)(ky * 3 + kx)) * F + f) * C + c;
    } else {
      o = ((t * 9 + (long)((2 - ky) * 3 + (2 - kx))) * C + c) * F + f;
    }
    wp[o] = f2bf(w[i]);
  }
}

// ---------------------------------------------------------------------------
// fwd / dgrad kernel.
//   X  [T, NB, H, W, Ci] ; Wp [T, 9, Co, Ci] ; bias [T, Co] or nullptr
//   Y  [T, NB, Ho, Wo, Co]            pad = im2col pad (fwd p, dgrad 2-p)
//
// Block = 256 threads = 4 waves, tile MM_M = 128 positions x MM_N = 128
// output channels, K-step MM_K = 32 channels inside one (ky, kx) tap; the K
// loop runs 9 * ceil(Ci / 32) steps.  Grid (ceil(M/128), ceil(Co/128), T).
// Wave (wm, wn) of the 2 x 2 arrangement owns positions [64 wm, +64) and
// channels [64 wn, +64): 4 x 4 accumulators.  16-column tiles past Co are
// skipped (wave-uniform).
//
// LDS: A (im2col) as [position][k], B (weights) as [channel][k], both
// k-contiguous, row stride MM_LD = 40 bf16 (32 + 8 of PADDING, 80 bytes):
// 2 x 10 KB.  A fragment is one ds_read_b128 per lane: row lane&15, k =
// 8 * (lane>>4) .. +7, which is the MFMA's operand layout as it stands.
// Banks: 80 bytes = 20 dwords, and 20 r mod 64 for r = 0..15 are the sixteen
// distinct multiples of 4, so the 16 rows of a lane group cover all 64 banks
// once — conflict-free, where the unpadded 64-byte stride would put rows r
// and r + 4 on the same banks.  Per K-step 8 fragment reads feed 16 MFMAs.
//
// The MFMA is issued with the WEIGHT fragment as its row operand, so the
// accumulator holds D[channel = 4 * (lane>>4) + j][position = lane&15]: a
// lane owns 4 consecutive channels of one position and stores them as one
// 8-byte write.
//
// Staging: thread -> fixed 8-channel chunk (tid & 3) and rows tid>>2 and
// tid>>2 + 64 of both tiles; its two position decodes live in registers
// for the whole K loop.
// ---------------------------------------------------------------------------
#define MM_M 128
#define MM_N 128
#define MM_K 32
#define MM_LD 40

__global__ __launch_bounds__(256)
void wconv_mm_kernel(const short* __restrict__ X, const short* __restrict__ Wp,
                     const float* __restrict__ bias, short* __restrict__ Y,
                     int NB, int H, int W, int Ci, int Ho, int Wo, int Co,
                     int pad) {
  const int t = blockIdx.z;
  const long Mtot = (long)NB * Ho * Wo;
  const long m0 = (long)blockIdx.x * MM_M;
  const int co0 = blockIdx.y * MM_N;

  __shared__ __attribute__((aligned(16))) short lds_a[MM_M * MM_LD];
  __shared__ __attribute__((aligned(16))) short lds_b[MM_N * MM_LD];

  const short* Xt = X + (long)t * NB * H * W * Ci;
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
      r_w[i] = (int)(mg % Wo);
      r_h[i] = (int)((mg / Wo) % Ho);
      r_n[i] = (int)(mg / ((long)Wo * Ho));
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

  const int ksteps = (Ci + MM_K - 1) / MM_K;
  const int nsteps = 9 * ksteps;
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // global -> register half of the staging for K-step s; a step past the
  // last one, channels past Ci, rows past M, taps outside the image and
  // columns past Co load nothing and stage zeros
  bf16x8 va[2], vb[2];
  auto load_step = [&](int s) {
    const int tap = s / ksteps;
    const int c = (s - tap * ksteps) * MM_K + sq;
    const int dy = tap / 3 - pad, dx = tap % 3 - pad;
    const bool kok = s < nsteps && c < Ci;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      bf16x8 v = zero8;
      const int h = r_h[i] + dy, w = r_w[i] + dx;
      if (kok && r_n[i] >= 0 && h >= 0 && h < H && w >= 0 && w < W) {
        v = *(const bf16x8*)&Xt[(((long)r_n[i] * H + h) * W + w) * Ci + c];
      }
      va[i] = v;
      const int co = co0 + sr + 64 * i;
      bf16x8 u = zero8;
      if (kok && co < Co) {
        u = *(const bf16x8*)&Wt[((long)tap * Co + co) * Ci + c];
      }
      vb[i] = u;
    }
  };

  load_step(0);
  for (int s = 0; s < nsteps; ++s) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *(bf16x8*)&lds_a[(sr + 64 * i) * MM_LD + sq] = va[i];
      *(bf16x8*)&lds_b[(sr + 64 * i) * MM_LD + sq] = vb[i];
    }
    __syncthreads();
    // prefetch: the next K-step's global loads fly under this step's MFMAs
    load_step(s + 1);

    bf16x8 af[4], bfr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      af[i] = *(const bf16x8*)&lds_a[(wm * 64 + i * 16 + fr) * MM_LD + fk * 8];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bfr[j] = *(const bf16x8*)&lds_b[(wn * 64 + j * 16 + fr) * MM_LD + fk * 8];
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

  // epilogue: D row = channel 4 * fk + e, D column = position fr; bias added
  // in fp32, one rounding, 4 channels per 8-byte store
  short* Yt = Y + (long)t * Mtot * Co;
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
      const long mg = m0 + wm * 64 + i * 16 + fr;
      if (mg >= Mtot) continue;
      bf16x4v o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(acc[i][j][e] + bv[e]);
      *(bf16x4v*)&Yt[mg * Co + co] = o;
    }
  }
}

// ---------------------------------------------------------------------------
// wgrad kernel: slice[t][chunk][n = (tap, c)][f] = sum over the chunk's
// positions k of dY[t,k,f] * im2col(X)[t,k,n]; dbslice[t][chunk][f] = sum_k dY.
//   dY [T, NB, Ho, Wo, F] ; X [T, NB, H, W, C]
// Block = 256 threads = 4 waves over a WG_F = 128 tile of F and a WG_N = 128
// tile of the 9C columns; wave (wf, wn) owns a 64 x 64 quarter (4 x 4
// accumulators).  Grid (F tiles * column tiles, K-chunks, T); every
// (t, chunk) block stores a PRIVATE slice with plain stores and
// wconv_wgrad_finalize_kernel sums the slices in chunk order — one path in
// every mode.  16-wide tiles past F or past 9C are skipped (wave-uniform).
//
// Both operands sit position-major in memory and are staged AS STORED: dY
// tile [k][f] and im2col tile [k][n], WG_K = 32 positions per K-step, 16-byte
// writes, row stride WG_LD = 144 bf16 (128 + 16 of PADDING, 288 bytes): 2 x
// 9 KB.  The MFMA wants k-contiguous fragments, so the transpose happens in
// the LDS read: ds_read_b64_tr_b16 takes, per 16-lane group, a 4-row x
// 16-column block (lane 4q + p supplies the address of row q, columns
// 4p..4p+3) and hands lane i column i of it.  Lane group g = lane>>4 reads
// rows 4g..4g+3 and 16 + 4g..+3: its 8 reduction indices are a permutation
// of the step's k, the same on the dY and on the X side, so the product is
// unchanged.  Banks: a 32-lane half reads 8 CONSECUTIVE rows x 32 bytes;
// 288 bytes = 72 dwords = 8 mod 64, so row i of the eight starts at bank 8i
// and the half covers the 64 banks once — conflict-free, where the unpadded
// 256-byte stride would put all 8 rows on the same banks.
//
// Staging: thread -> fixed 8-column chunk (tid & 15) of both tiles — its
// (tap, channel) decode is done once — and rows tid>>4 and tid>>4 + 16,
// whose (wo, ho, image) advance by 32 positions per K-step with carries.
// The bias gradient is the ordered column sum of the staged dY tiles, from
// column-block 0 only.
// ---------------------------------------------------------------------------
#define WG_F 128
#define WG_N 128
#define WG_K 32
#define WG_LD 144
static_assert(WG_K == wgplan::kStepWide && WG_N == wgplan::kTileWide &&
                  WG_F == wgplan::kTileWide,
              "wgrad_plan.h cuts K-chunks for these tiles");

__global__ __launch_bounds__(256)
void wconv_wgrad_kernel(const short* __restrict__ dY,
                        const short* __restrict__ X,
                        float* __restrict__ dWsl,  // [T, nsl, 9C, F]
                        float* __restrict__ dBsl,  // [T, nsl, F] or nullptr
                        int NB, int H, int W, int C, int Ho, int Wo, int F,
                        int pad, int kchunk, int fblk) {
  const int t = blockIdx.z;
  const int fb = blockIdx.x % fblk;
  const int nb = blockIdx.x / fblk;
  const int f0 = fb * WG_F;
  const int n0 = nb * WG_N;
  const int N9 = 9 * C;
  const long Ktot = (long)NB * Ho * Wo;
  const long kc0 = (long)blockIdx.y * kchunk;
  const long kc_end = min(kc0 + (long)kchunk, Ktot);

  __shared__ __attribute__((aligned(16))) short lds_a[WG_K * WG_LD];  // dY [k][f]
  __shared__ __attribute__((aligned(16))) short lds_b[WG_K * WG_LD];  // col [k][n]
  __shared__ float db_lds[WG_F];

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

  // fused bias grad: the dY tile is the same in every column block, so only
  // column-block 0 sums it; thread -> column tid & 127, rows 16 * (tid>>7)..
  const bool do_bias = (dBsl != nullptr) && (nb == 0);
  float db_acc = 0.f;
  const int db_f = tid & 127;
  const int db_h = tid >> 7;

  // The two staging rows of this thread advance by WG_K positions per
  // K-step: decode (wo, ho, img) once, then step it with carries.  dho < Ho
  // and one carry keep ho below 2 * Ho.
  const int s_dwo = WG_K % Wo;
  const int s_dho = (WG_K / Wo) % Ho;
  const int s_dimg = (WG_K / Wo) / Ho;
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
        const int h = p_ho[i] + b_dy, w = p_wo[i] + b_dx;
        if (b_ok && h >= 0 && h < H && w >= 0 && w < W) {
          x8 = *(const bf16x8*)&Xt[(((long)p_img[i] * H + h) * W + w) * C + b_c];
        }
      }
      vy[i] = y8;
      vx[i] = x8;
      // advance this row to the next K-step
      p_k[i] += WG_K;
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
  const int tr_lane = (fk * 4 + ((lane >> 2) & 3)) * WG_LD + (lane & 3) * 4;
  auto read_tr = [&](const short* tile, int cblk) {
    const short* p0 = tile + tr_lane + cblk * 16;
    const bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) bf16x4v*)p0);
    const bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) bf16x4v*)(p0 + 16 * WG_LD));
    const bf16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return r;
  };

  load_step();
  for (long k0 = kc0; k0 < kc_end; k0 += WG_K) {
    __syncthreads();  // previous K-step's reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *(bf16x8*)&lds_a[(sr + 16 * i) * WG_LD + cc] = vy[i];
      *(bf16x8*)&lds_b[(sr + 16 * i) * WG_LD + cc] = vx[i];
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
        db_acc += bf2f(lds_a[kk * WG_LD + db_f]);
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
__global__ void wconv_wgrad_finalize_kernel(const float* __restrict__ sl,
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
static bool wconv_channels_ok(long a, long b) {
  return a >= 8 && b >= 8 && a % 8 == 0 && b % 8 == 0 && a <= 256 && b <= 256;
}

static bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

torch::Tensor wconv_repack(torch::Tensor w, bool flip) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 5 && w.size(3) == 3 && w.size(4) == 3);
  TORCH_CHECK(w.scalar_type() == torch::kFloat32, "wconv_repack needs fp32");
  auto wc = w.contiguous();
  const int T = (int)w.size(0), F = (int)w.size(1), C = (int)w.size(2);
  TORCH_CHECK(w.size(0) <= 65535, "wconv_repack: at most 65535 tasks");
  auto wp = torch::empty({T, 9, flip ? C : F, flip ? F : C},
                         w.options().dtype(torch::kBFloat16));
  const long total = (long)T * F * C * 9;
  if (total == 0) return wp;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(wconv_repack_kernel, dim3(ew_grid(total)), dim3(256), 0,
                     stream.stream(), wc.data_ptr<float>(),
                     reinterpret_cast<short*>(wp.data_ptr()), T, F, C, flip);
  return wp;
}

// x [T, NB, H, W, Ci] bf16 ; wp [T, 9, Co, Ci] bf16 ; bias [T, Co] fp32 / undef
torch::Tensor wconv_mm(torch::Tensor x, torch::Tensor wp,
                       c10::optional<torch::Tensor> bias, long pad,
                       long Ho, long Wo) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 5 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "wconv_mm needs bf16");
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 4 && wp.is_contiguous() &&
              wp.scalar_type() == torch::kBFloat16 && wp.size(1) == 9 &&
              wp.device() == x.device());
  TORCH_CHECK(x.size(0) <= 65535, "wconv_mm: at most 65535 tasks (grid.z)");
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), Ci = (int)x.size(4);
  const int Co = (int)wp.size(2);
  TORCH_CHECK(wp.size(0) == T && wp.size(3) == Ci, "wp does not match x");
  TORCH_CHECK(wconv_channels_ok(Ci, Co),
              "wconv_mm: channels must be multiples of 8 in 8..256");
  TORCH_CHECK(pad >= 0 && pad <= 2 && Ho == H + 2 * pad - 2 &&
              Wo == W + 2 * pad - 2 && Ho >= 1 && Wo >= 1,
              "wconv_mm: output size does not match the im2col pad");
  TORCH_CHECK(aligned16(x) && aligned16(wp), "wconv_mm: 16-byte alignment");
  auto y = torch::empty({T, NB, Ho, Wo, Co}, x.options());
  const long Mtot = (long)NB * Ho * Wo;
  if (T == 0 || Mtot == 0) return y;
  // positions are decoded and the row grid is cut in 32 bits; every global
  // offset is carried as 64-bit
  TORCH_CHECK(Mtot < (1L << 30) && (long)NB * H * W < (1L << 30),
              "wconv_mm: too many positions per task");
  TORCH_CHECK(aligned16(y), "wconv_mm: 16-byte alignment");
  const float* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == torch::kFloat32 &&
                bias->numel() == (long)T * Co);
    bc = bias->contiguous();
    bptr = bc.data_ptr<float>();
  }
  dim3 grid((unsigned)((Mtot + MM_M - 1) / MM_M),
            (unsigned)((Co + MM_N - 1) / MM_N), T);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(wconv_mm_kernel, grid, dim3(256), 0, stream.stream(),
                     reinterpret_cast<const short*>(x.data_ptr()),
                     reinterpret_cast<const short*>(wp.data_ptr()), bptr,
                     reinterpret_cast<short*>(y.data_ptr()), NB, H, W, Ci,
                     (int)Ho, (int)Wo, Co, (int)pad);
  return y;
}

// The split-K plan wconv_wgrad cuts for a shape: {kchunk, chunks}.
std::vector<long> wconv_wgrad_plan(long T, long NB, long Ho, long Wo, long C,
                                   long F) {
  const wgplan::Plan p =
      wgplan::wconv((int)T, (int)NB, (int)Ho, (int)Wo, (int)C, (int)F);
  return {p.kchunk, p.gridy};
}

// dy [T, NB, Ho, Wo, F] bf16 ; x [T, NB, H, W, C] bf16
// -> {dw [T, F, C, 3, 3] fp32, db [T, F] fp32 (zeros unless with_bias)}
std::vector<torch::Tensor> wconv_wgrad(torch::Tensor dy, torch::Tensor x,
                                       long pad, bool with_bias) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && dy.dim() == 5 && x.dim() == 5 &&
              dy.device() == x.device());
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
              x.scalar_type() == torch::kBFloat16, "wconv_wgrad needs bf16");
  auto dyc = dy.contiguous();
  auto xc = x.contiguous();
  TORCH_CHECK(x.size(0) <= 65535, "wconv_wgrad: at most 65535 tasks (grid.z)");
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int Ho = (int)dy.size(2), Wo = (int)dy.size(3), F = (int)dy.size(4);
  TORCH_CHECK(dy.size(0) == T && dy.size(1) == NB, "dy does not match x");
  TORCH_CHECK(wconv_channels_ok(C, F),
              "wconv_wgrad: channels must be multiples of 8 in 8..256");
  TORCH_CHECK(pad >= 0 && pad <= 2 && Ho == H + 2 * pad - 2 &&
              Wo == W + 2 * pad - 2 && Ho >= 1 && Wo >= 1,
              "wconv_wgrad: dy size does not match the pad");
  TORCH_CHECK(aligned16(dyc) && aligned16(xc), "wconv_wgrad: 16-byte alignment");
  const int N9 = 9 * C;
  const long Ktot = (long)NB * Ho * Wo;
  // positions are stepped in 32 bits; every global offset is 64-bit
  TORCH_CHECK(Ktot < (1L << 30) && (long)NB * H * W < (1L << 30),
              "wconv_wgrad: too many positions per task");
  auto fopts = x.options().dtype(torch::kFloat32);
  auto dw = torch::empty({T, F, C, 3, 3}, fopts);
  auto db = torch::zeros({T, F}, fopts);
  if (T == 0 || Ktot == 0) return {dw.zero_(), db};
  const wgplan::Plan p = wgplan::wconv(T, NB, Ho, Wo, C, F);
  const int nsl = p.nslices;
  const int fblk = (F + WG_F - 1) / WG_F;
  TORCH_CHECK(nsl >= 1 && nsl <= 65535 && p.gridx == fblk * ((N9 + WG_N - 1) / WG_N),
              "wconv_wgrad: plan does not match the tiles");
  auto sl = torch::empty({T, nsl, N9, F}, fopts);
  auto dbsl = torch::empty({T, nsl, F}, fopts);
  TORCH_CHECK(aligned16(sl), "wconv_wgrad: 16-byte alignment");
  dim3 grid((unsigned)p.gridx, (unsigned)nsl, T);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(wconv_wgrad_kernel, grid, dim3(256), 0, stream.stream(),
                     reinterpret_cast<const short*>(dyc.data_ptr()),
                     reinterpret_cast<const short*>(xc.data_ptr()),
                     sl.data_ptr<float>(),
                     with_bias ? dbsl.data_ptr<float>() : nullptr, NB, H, W, C,
                     Ho, Wo, F, (int)pad, p.kchunk, fblk);
  const long total = (long)T * F * C * 9;
  hipLaunchKernelGGL(wconv_wgrad_finalize_kernel, dim3(ew_grid(total)),
                     dim3(256), 0, stream.stream(), sl.data_ptr<float>(),
                     with_bias ? dbsl.data_ptr<float>() : nullptr,
                     dw.data_ptr<float>(), db.data_ptr<float>(), T, F, C, nsl);
  return {dw, db};
}
