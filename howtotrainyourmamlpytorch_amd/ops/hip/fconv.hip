// fp32 task-batched stride-1 3x3 convolution trio (fwd / dgrad / wgrad) as
// implicit GEMM on the exact fp32 matrix path of gfx950,
// v_mfma_f32_16x16x4_f32 — the fp32 twin of tconv.hip, same layouts and the
// same contract:
//
//   fwd   : Y[t]  = im2col(X[t])  @ Wp[t]       M=NB*Ho*Wo, N=Co, K=9*Ci
//   dgrad : dX[t] = im2col(dY[t]) @ Wp_flip[t]  (SAME kernel; weights
//           repacked flipped+transposed, im2col pad' = 2 - pad)
//   wgrad : dW[t] = dY[t]^T @ im2col(X[t])      split-K over positions,
//           private slice per K-chunk + ordered finalize, db fused
//
// Activations [T, NB, H, W, C] fp32, weights [T, F, C, 3, 3] fp32 used
// UNROUNDED, bias [T, F] fp32, all outputs fp32.  C and F are any value in
// 1..64: nothing needs channel alignment (C % 4 == 0 only selects 16-byte
// gathers over scalar ones).
//
// The instruction is a k-ordered fmaf chain (one rounding per product), at
// 1/16 of the bf16 MFMA rate, so per staged byte these kernels are ~8x
// more compute-heavy than tconv.hip's.  Hence the plain structure: every
// K-step stages both tiles synchronously through registers between two
// barriers, with bounds-checked im2col gathers that yield 0 outside the
// image — no async staging, no zero page, no pre-swizzled weight image.
// The one refinement is a register prefetch: the global loads of K-step
// k+1 are issued before the MFMAs of step k and written to LDS after them.
// No floating-point atomics anywhere: every reduction order is fixed, so
// all three ops are bitwise run-to-run reproducible in every mode.

#include "common.h"
#include "wgrad_plan.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

using namespace maml355;

typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;

// ---------------------------------------------------------------------------
// Weight repack: W [T, F, C, 3, 3] fp32 -> Wp [T, 9, Ci, Co] fp32 (a pure
// permutation, no rounding)
//   fwd  : Wp[t][ky*3+kx][c][f] = W[t][f][c][ky][kx]          (Ci=C, Co=F)
//   dgrad: Wp[t][ky*3+kx][f][c] = W[t][f][c][2-ky][2-kx]      (Ci=F, Co=C)
// ---------------------------------------------------------------------------
__global__ void fconv_repack_kernel(const float* __restrict__ w,
                                    float* __restrict__ wp,
                                    int T, int F, int C, bool dgrad) {
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
    if (!dgrad) {
      o = (((t * 9 + (long)(ky * 3 + kx)) * C + c) * F) + f;
    } else {
      o = (((t * 9 + (long)((2 - ky) * 3 + (2 - kx))) * F + f) * C) + c;
    }
    wp[o] = w[i];
  }
}

// ---------------------------------------------------------------------------
// fwd / dgrad kernel.
//   X  [T, NB, H, W, Ci] ; Wp [T, 9, Ci, Co] ; bias [T, Co] or nullptr
//   Y  [T, NB, Ho, Wo, Co]            pad = im2col pad (fwd p, dgrad 2-p)
//
// Block = 256 threads = 4 waves, tile FBM=128 rows x 64 cols, K-step
// FBK=32.  Wave w owns rows [32w, 32w+32) as two 16-row halves times up
// to four 16-col tiles: 8 independent accumulators (2 when Co <= 16), the
// MFMAs issued round-robin over them so no two neighbours share one (40-
// cycle dependent latency vs 32-cycle issue).
//
// Operand layout: both tiles are k-contiguous in LDS, A as [m][k] and B
// transposed as [col][k], row stride FLD = FBK + 4 floats.  The MFMA wants
// one float per lane, A[i = lane&15][k = lane>>4]; a lane group g = lane>>4
// reads the FOUR consecutive k  16*kb + 4*g + {0,1,2,3}  of its row with
// one ds_read_b128 and feeds element j to MFMA j of that 16-wide K block.
// MFMA j therefore contracts k in {16kb + 4g + j : g = 0..3} — a
// permutation of the block's k, identical on the A and the B side, so the
// product is unchanged and the result is still one fmaf chain.
// Banks: row stride 36 floats puts the 16 rows of a lane group on the 16
// distinct multiples of 4 (36r mod 64), i.e. one b128 read covers all 64
// banks exactly once per 16 lanes — conflict-free, where the unpadded
// stride 32 would put every second row on the same banks.
//
// Staging: thread -> fixed k-quad (tid & 7) and rows tid>>3 + 32*i, so its
// four row decodes live in registers for the whole K loop and each K-step
// decodes one k-quad; no LDS tables.
// ---------------------------------------------------------------------------
#define FBM 128
#define FBK 32
#define FLD (FBK + 4)

template <int NT>   // 16-column tiles: ceil(Co / 16), compile-time so the
                     // MFMA loop has no branches and its LDS reads batch
__global__ __launch_bounds__(256)
void fconv_mm_kernel(const float* __restrict__ X, const float* __restrict__ Wp,
                     const float* __restrict__ bias, float* __restrict__ Y,
                     int T, int NB, int H, int W, int Ci,
                     int Ho, int Wo, int Co, int pad) {
  const int t = blockIdx.y;
  const long Mtot = (long)NB * Ho * Wo;
  const long m0 = (long)blockIdx.x * FBM;
  const int K9 = 9 * Ci;
  const bool vec = (Ci % 4) == 0;

  __shared__ __attribute__((aligned(16))) float lds_a[FBM * FLD];
  __shared__ __attribute__((aligned(16))) float lds_bt[64 * FLD];

  const float* Xt = X + (long)t * NB * H * W * Ci;
  const float* Wt = Wp + (long)t * 9 * Ci * Co;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int fr = lane & 15;
  const int fk = lane >> 4;

  // this thread's four staging rows (registers, decoded once)
  const int kq = (tid & 7) * 4;
  int r_n[4], r_h[4], r_w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long mg = m0 + (tid >> 3) + 32 * i;
    if (mg < Mtot) {
      r_w[i] = (int)(mg % Wo);
      r_h[i] = (int)((mg / Wo) % Ho);
      r_n[i] = (int)(mg / ((long)Wo * Ho));
    } else {
      r_n[i] = -1; r_h[i] = 0; r_w[i] = 0;
    }
  }
  // B staging: column f fixed per thread, k rows tid>>6 + 4*i
  const int b_f = tid & 63;
  const int b_k = tid >> 6;

  f32x4 acc[2][NT];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[hh][i] = {0.f, 0.f, 0.f, 0.f};

  // global -> register half of the staging for the K-step at k0 (k >= K9
  // loads nothing and stages zeros)
  f32x4 va[4];
  float vb[8];
  auto load_step = [&](int k0) {
    // ---- A (im2col gather)
    if (vec) {
      // Ci % 4 == 0: the quad k..k+3 is 4 consecutive channels of one tap,
      // 16-byte aligned; K9 % 4 == 0, so the quad is valid as a whole
      const int k = k0 + kq;
      const int kyx = k / Ci;
      const int c0 = k - kyx * Ci;
      const int dy = kyx / 3 - pad, dx = kyx % 3 - pad;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int h = r_h[i] + dy, w = r_w[i] + dx;
        if (k < K9 && r_n[i] >= 0 && h >= 0 && h < H && w >= 0 && w < W) {
          v = *(const f32x4*)&Xt[(((long)r_n[i] * H + h) * W + w) * Ci + c0];
        }
        va[i] = v;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) va[i] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + kq + j;
        if (k < K9) {
          const int kyx = k / Ci;
          const int c = k - kyx * Ci;
          const int dy = kyx / 3 - pad, dx = kyx % 3 - pad;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int h = r_h[i] + dy, w = r_w[i] + dx;
            if (r_n[i] >= 0 && h >= 0 && h < H && w >= 0 && w < W) {
              va[i][j] = Xt[(((long)r_n[i] * H + h) * W + w) * Ci + c];
            }
          }
        }
      }
    }
    // ---- B^T: Wp rows k0..k0+31 are contiguous [k][Co]
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = k0 + b_k + 4 * i;
      vb[i] = (b_f < Co && k < K9) ? Wt[(long)k * Co + b_f] : 0.f;
    }
  };
  load_step(0);
  for (int k0 = 0; k0 < K9; k0 += FBK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(f32x4*)&lds_a[((tid >> 3) + 32 * i) * FLD + kq] = va[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      lds_bt[b_f * FLD + b_k + 4 * i] = vb[i];
    }
    __syncthreads();
    // prefetch: the next K-step's global loads fly under this step's MFMAs
    load_step(k0 + FBK);

#pragma unroll
    for (int kb = 0; kb < FBK / 16; ++kb) {
      const int kc = kb * 16 + fk * 4;
      const f32x4 a0 = *(const f32x4*)&lds_a[(wave * 32 + fr) * FLD + kc];
      const f32x4 a1 = *(const f32x4*)&lds_a[(wave * 32 + 16 + fr) * FLD + kc];
      f32x4 b[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        b[nt] = *(const f32x4*)&lds_bt[(nt * 16 + fr) * FLD + kc];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a0[j], b[nt][j], acc[0][nt], 0, 0, 0);
          acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a1[j], b[nt][j], acc[1][nt], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // all waves done reading before the next staging
  }

  // epilogue: C/D layout col = lane&15, row = (lane>>4)*4 + j; bias added
  float* Yt = Y + (long)t * Mtot * Co;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = nt * 16 + fr;
      if (col >= Co) continue;
      const float bv = bias ? bias[(long)t * Co + col] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long mg = m0 + wave * 32 + hh * 16 + fk * 4 + j;
        if (mg < Mtot) Yt[mg * Co + col] = acc[hh][nt][j] + bv;
      }
    }
}

// ---------------------------------------------------------------------------
// wgrad kernel: slice[t][chunk][n = 9C][f] = sum over the chunk's positions
// k of dY[t,k,f] * im2col(X)[t,k,n];  dbslice[t][chunk][f] = sum_k dY.
//   dY [T, NB, Ho, Wo, F] ; X [T, NB, H, W, C]
// Block = 256 threads = 4 waves over a 64-column block of 9C; wave w owns
// the 16-column sub-tile w and walks the <= 4 row tiles of F: 4 independent
// accumulators.  Grid (column blocks, K-chunks, T); every (t, chunk) block
// stores a PRIVATE slice with plain stores and fconv_wgrad_finalize_kernel
// sums the slices in chunk order — no atomics, one path in every mode.
//
// Both tiles are staged AS STORED, position-major: dY tile [k][f] and
// im2col tile [k][n], row stride WLD = 80 floats, 16-byte writes.  The
// reduction index is the LDS row here, so each MFMA operand is one
// ds_read_b32 (B is reused over the F tiles: 1.25 reads per MFMA).  Banks:
// a read touches rows 4ks + (lane>>4) at columns base + (lane&15); stride
// 80 = 64 + 16 shifts consecutive rows by 16 banks, so the 64 lanes cover
// the 64 banks once (stride 64 would be a 4-way conflict).
// Staging: thread -> fixed column quad (tid & 15) and rows tid>>4 + 16*i,
// one position decode per row and K-step in registers.  The global loads
// of K-step k+1 are issued before the MFMAs of step k and written to LDS
// after them (register prefetch), so their latency is not on the path.
// ---------------------------------------------------------------------------
#define WFN 64
#define WFK 32
static_assert(WFK == wgplan::kStepF32 && WFN == wgplan::kCols,
              "wgrad_plan.h cuts K-chunks for these tiles");
#define WLD 80

template <int MT>   // 16-row tiles of F: ceil(F / 16), compile-time (as NT)
__global__ __launch_bounds__(256)
void fconv_wgrad_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                        float* __restrict__ dWsl,  // [T, nsl, 9C, F]
                        float* __restrict__ dBsl,  // [T, nsl, F] or nullptr
                        int T, int NB, int H, int W, int C,
                        int Ho, int Wo, int F, int pad, int kchunk) {
  const int t = blockIdx.z;
  const int n0 = blockIdx.x * WFN;
  const int N9 = 9 * C;
  const long Ktot = (long)NB * Ho * Wo;
  const long kchunk0 = (long)blockIdx.y * kchunk;
  const long kchunk_end = min(kchunk0 + (long)kchunk, Ktot);
  const bool vecx = (C % 4) == 0;
  const bool vecf = (F % 4) == 0;

  __shared__ __attribute__((aligned(16))) float lds_a[WFK * WLD];  // dY  [k][f]
  __shared__ __attribute__((aligned(16))) float lds_b[WFK * WLD];  // col [k][n]
  __shared__ float db_lds[4][64];

  const float* dYt = dY + (long)t * Ktot * F;
  const float* Xt = X + (long)t * NB * H * W * C;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const int lane = tid % WAVE;
  const int fr = lane & 15;
  const int fk = lane >> 4;
  const bool wave_live = n0 + wave * 16 < N9;  // wave-uniform

  // this thread's column quad, decoded once: n -> (tap, c)
  const int q4 = (tid & 15) * 4;
  int q_dy[4], q_dx[4], q_c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + q4 + j;
    if (n < N9) {
      const int kyx = n / C;
      q_c[j] = n - kyx * C;
      q_dy[j] = kyx / 3 - pad;
      q_dx[j] = kyx % 3 - pad;
    } else {
      q_c[j] = -1; q_dy[j] = 0; q_dx[j] = 0;
    }
  }

  f32x4 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = {0.f, 0.f, 0.f, 0.f};
  // fused bias grad: the dY tile is the same in every column block, so
  // only block column 0 sums it
  const bool do_bias = (dBsl != nullptr) && (blockIdx.x == 0);
  float db_acc = 0.f;
  const int db_f = tid & 63;
  const int db_q = tid >> 6;  // rows 8*db_q .. 8*db_q+7 of the tile

  // global -> register half of the staging for the K-step at k0; rows past
  // the chunk end load nothing and stage zeros
  // The two staging rows of this thread advance by WFK positions per
  // K-step: decode (wo, ho, img) once, then step it with carries — a
  // per-step division by Wo and Ho costs more VALU time than the step's
  // MFMAs take.  dho < Ho and one carry keep ho below 2*Ho.
  const int s_dwo = WFK % Wo;
  const int s_dho = (WFK / Wo) % Ho;
  const int s_dimg = (WFK / Wo) / Ho;
  int p_k[2], p_wo[2], p_ho[2], p_img[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int k = (int)kchunk0 + (tid >> 4) + 16 * i;
    p_k[i] = k;
    p_wo[i] = k % Wo;
    p_ho[i] = (k / Wo) % Ho;
    p_img[i] = (k / Wo) / Ho;
  }
  f32x4 vy[2], vx[2];
  auto load_step = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long k = p_k[i];
      f32x4 y4 = {0.f, 0.f, 0.f, 0.f}, x4 = {0.f, 0.f, 0.f, 0.f};
      if (k < kchunk_end) {
        // dY row k, columns q4..q4+3
        const float* src = dYt + k * F + q4;
        if (vecf) {
          if (q4 < F) y4 = *(const f32x4*)src;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (q4 + j < F) y4[j] = src[j];
        }
        const int wo = p_wo[i], ho = p_ho[i];
        const long img = p_img[i];
        if (vecx) {
          // C % 4 == 0: the quad is 4 consecutive channels of one tap
          const int h = ho + q_dy[0], w = wo + q_dx[0];
          if (q_c[0] >= 0 && h >= 0 && h < H && w >= 0 && w < W) {
            x4 = *(const f32x4*)&Xt[((img * H + h) * W + w) * C + q_c[0]];
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int h = ho + q_dy[j], w = wo + q_dx[j];
            if (q_c[j] >= 0 && h >= 0 && h < H && w >= 0 && w < W) {
              x4[j] = Xt[((img * H + h) * W + w) * C + q_c[j]];
            }
          }
        }
      }
      vy[i] = y4;
      vx[i] = x4;
      // advance this row to the next K-step
      p_k[i] += WFK;
      p_wo[i] += s_dwo;
      const int cw = p_wo[i] >= Wo;
      p_wo[i] -= cw ? Wo : 0;
      p_ho[i] += s_dho + cw;
      const int ch = p_ho[i] >= Ho;
      p_ho[i] -= ch ? Ho : 0;
      p_img[i] += s_dimg + ch;
    }
  };
  load_step();
  for (long k0 = kchunk0; k0 < kchunk_end; k0 += WFK) {
    __syncthreads();  // previous K-step's reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int kk = (tid >> 4) + 16 * i;
      *(f32x4*)&lds_a[kk * WLD + q4] = vy[i];
      *(f32x4*)&lds_b[kk * WLD + q4] = vx[i];
    }
    __syncthreads();
    // prefetch: the next K-step's global loads fly under this step's MFMAs
    load_step();

    if (wave_live) {
#pragma unroll
      for (int ks = 0; ks < WFK / 4; ++ks) {
        const float b = lds_b[(ks * 4 + fk) * WLD + wave * 16 + fr];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const float a = lds_a[(ks * 4 + fk) * WLD + mt * 16 + fr];
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[mt], 0, 0, 0);
        }
      }
    }
    if (do_bias) {
#pragma unroll
      for (int kk = db_q * 8; kk < db_q * 8 + 8; ++kk) {
        db_acc += lds_a[kk * WLD + db_f];
      }
    }
  }
  if (do_bias) {
    db_lds[db_q][db_f] = db_acc;
    __syncthreads();
    if (db_q == 0 && db_f < F) {
      const float v = ((db_lds[0][db_f] + db_lds[1][db_f]) + db_lds[2][db_f]) +
                      db_lds[3][db_f];
      dBsl[((long)t * gridDim.y + blockIdx.y) * F + db_f] = v;
    }
  }

  // C/D: col = lane&15 (n within the wave's sub-tile), row = fk*4+j (f).
  // Column blocks are disjoint, so the (t, chunk) slice is written once.
  float* dWt = dWsl + ((long)t * gridDim.y + blockIdx.y) * N9 * F;
  const int n = n0 + wave * 16 + fr;
  if (wave_live && n < N9) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = mt * 16 + fk * 4 + j;
        if (f < F) dWt[(long)n * F + f] = acc[mt][j];
      }
    }
  }
}

// slices [T, nsl, 9C, F] -> dW [T, F, C, 3, 3]; dbsl [T, nsl, F] -> db [T, F].
// Slices are summed in chunk order: the one, fixed reduction order.
__global__ void fconv_wgrad_finalize_kernel(const float* __restrict__ sl,
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
torch::Tensor fconv_repack(torch::Tensor w, bool dgrad) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 5 && w.size(3) == 3 && w.size(4) == 3);
  TORCH_CHECK(w.scalar_type() == torch::kFloat32, "fconv_repack needs fp32");
  auto wc = w.contiguous();
  const int T = (int)w.size(0), F = (int)w.size(1), C = (int)w.size(2);
  auto wp = torch::empty({T, 9, dgrad ? F : C, dgrad ? C : F}, w.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  const long total = (long)T * F * C * 9;
  if (total == 0) return wp;
  hipLaunchKernelGGL(fconv_repack_kernel, dim3(ew_grid(total)), dim3(256),
                     0, stream.stream(), wc.data_ptr<float>(),
                     wp.data_ptr<float>(), T, F, C, dgrad);
  return wp;
}

// x [T, NB, H, W, Ci] fp32 ; wp [T, 9, Ci, Co] fp32 ; bias [T, Co] fp32 / undef
torch::Tensor fconv_mm(torch::Tensor x, torch::Tensor wp,
                       c10::optional<torch::Tensor> bias, long pad,
                       long Ho, long Wo) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 5 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kFloat32, "fconv_mm needs fp32");
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 4 && wp.is_contiguous() &&
              wp.scalar_type() == torch::kFloat32 && wp.size(1) == 9);
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), Ci = (int)x.size(4);
  const int Co = (int)wp.size(3);
  TORCH_CHECK(wp.size(0) == T && wp.size(2) == Ci, "wp does not match x");
  TORCH_CHECK(Ci >= 1 && Ci <= 64 && Co >= 1 && Co <= 64,
              "fconv_mm: channels must be in 1..64");
  TORCH_CHECK(T <= 65535, "fconv_mm: at most 65535 tasks (grid.y)");
  TORCH_CHECK(pad >= 0 && pad <= 2 && Ho == H + 2 * pad - 2 &&
              Wo == W + 2 * pad - 2 && Ho >= 1 && Wo >= 1,
              "fconv_mm: output size does not match the im2col pad");
  auto y = torch::empty({T, NB, Ho, Wo, Co}, x.options());
  const long Mtot = (long)NB * Ho * Wo;
  if (T == 0 || Mtot == 0) return y;
  const float* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    TORCH_CHECK(bias->scalar_type() == torch::kFloat32 && bias->numel() == (long)T * Co);
    bc = bias->contiguous();
    bptr = bc.data_ptr<float>();
  }
  dim3 grid((unsigned)((Mtot + FBM - 1) / FBM), T);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_FMM(NT_)                                                        \
  hipLaunchKernelGGL((fconv_mm_kernel<NT_>), grid, dim3(256), 0,               \
                     stream.stream(), x.data_ptr<float>(),                     \
                     wp.data_ptr<float>(), bptr, y.data_ptr<float>(), T, NB,   \
                     H, W, Ci, (int)Ho, (int)Wo, Co, (int)pad)
  switch ((Co + 15) / 16) {
    case 1: LAUNCH_FMM(1); break;
    case 2: LAUNCH_FMM(2); break;
    case 3: LAUNCH_FMM(3); break;
    default: LAUNCH_FMM(4); break;
  }
#undef LAUNCH_FMM
  return y;
}

// dy [T, NB, Ho, Wo, F] fp32 ; x [T, NB, H, W, C] fp32
// -> {dw [T, F, C, 3, 3] fp32, db [T, F] fp32 (zeros unless with_bias)}
std::vector<torch::Tensor> fconv_wgrad(torch::Tensor dy, torch::Tensor x,
                                       long pad, bool with_bias) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && dy.dim() == 5 && x.dim() == 5);
  TORCH_CHECK(dy.scalar_type() == torch::kFloat32 &&
              x.scalar_type() == torch::kFloat32, "fconv_wgrad needs fp32");
  auto dyc = dy.contiguous();
  auto xc = x.contiguous();
  const int T = (int)x.size(0), NB = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3), C = (int)x.size(4);
  const int Ho = (int)dy.size(2), Wo = (int)dy.size(3), F = (int)dy.size(4);
  TORCH_CHECK(dy.size(0) == T && dy.size(1) == NB, "dy does not match x");
  TORCH_CHECK(C >= 1 && C <= 64 && F >= 1 && F <= 64,
              "fconv_wgrad: channels must be in 1..64");
  TORCH_CHECK(T <= 65535, "fconv_wgrad: at most 65535 tasks (grid.z)");
  TORCH_CHECK(pad >= 0 && pad <= 2 && Ho == H + 2 * pad - 2 &&
              Wo == W + 2 * pad - 2 && Ho >= 1 && Wo >= 1,
              "fconv_wgrad: dy size does not match the pad");
  const int N9 = 9 * C;
  const long Ktot = (long)NB * Ho * Wo;
  TORCH_CHECK(Ktot < (1L << 30), "fconv_wgrad: too many positions per task");
  auto fopts = x.options();
  auto dw = torch::empty({T, F, C, 3, 3}, fopts);
  auto db = torch::zeros({T, F}, fopts);
  if (T == 0 || Ktot == 0) return {dw.zero_(), db};
  // K-chunks sized so the grid has ~3072 blocks: small support-pass
  // reductions would otherwise leave most of the chip idle, and a grid of
  // a few blocks per CU ends on a long partial round
  const wgplan::Plan p = wgplan::fconv(T, NB, Ho, Wo, C);
  const int nsl = p.nslices;
  auto sl = torch::empty({T, nsl, N9, F}, fopts);
  auto dbsl = torch::empty({T, nsl, F}, fopts);
  dim3 grid((unsigned)p.gridx, (unsigned)nsl, T);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_FWG(MT_)                                                        \
  hipLaunchKernelGGL((fconv_wgrad_kernel<MT_>), grid, dim3(256), 0,            \
                     stream.stream(), dyc.data_ptr<float>(),                   \
                     xc.data_ptr<float>(), sl.data_ptr<float>(),               \
                     with_bias ? dbsl.data_ptr<float>() : nullptr, T, NB, H,   \
                     W, C, Ho, Wo, F, (int)pad, p.kchunk)
  switch ((F + 15) / 16) {
    case 1: LAUNCH_FWG(1); break;
    case 2: LAUNCH_FWG(2); break;
    case 3: LAUNCH_FWG(3); break;
    default: LAUNCH_FWG(4); break;
  }
#undef LAUNCH_FWG
  const long total = (long)T * F * C * 9;
  hipLaunchKernelGGL(fconv_wgrad_finalize_kernel, dim3(ew_grid(total)),
                     dim3(256), 0, stream.stream(), sl.data_ptr<float>(),
                     with_bias ? dbsl.data_ptr<float>() : nullptr,
                     dw.data_ptr<float>(), db.data_ptr<float>(), T, F, C, nsl);
  return {dw, db};
}
