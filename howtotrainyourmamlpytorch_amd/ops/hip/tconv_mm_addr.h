// A-operand staging addresses of the fwd/dgrad GEMM (tconv_mm_v2_kernel in
// tconv.hip), shared between the kernel and a host-side checker
// (tests/host/tconv_mm_addr_check.cpp): everything here compiles as plain
// C++, so the index arithmetic is walked exhaustively under ASan/UBSan on
// the CPU before it ever drives a DMA.
//
// GEMM view (per task): Y[m][f] = sum_k im2col(X)[m][k] * Wp[k][f] with
//   m = (img*Ho + ho)*Wo + wo     output position, Mtot = NB*Ho*Wo rows
//   k = tap*Ci + c                tap = ky*3 + kx, Ci % 8 == 0, K9 = 9*Ci
//   im2col(X)[m][k] = X[img][ho+ky-pad][wo+kx-pad][c], zero outside the image
// The kernel reads X as it is stored, UNPADDED: a 16-byte staging slot is 8
// channels of one tap of one row, so one decision per slot and K-step picks
// either the element offset of those 8 channels or the zero page — for a
// border tap, a row past Mtot (M-tail) or a k past K9 (K-tail).
//
// A block stages 256 rows x 64 k per K-step as 2048 slots; thread `tid` of
// 512 issues slots s = q*512 + tid, q = 0..3.  `global_load_lds` writes slot
// s linearly (row s>>3, stored chunk s&7), so the LDS XOR swizzle is a
// permutation of which SOURCE chunk the slot fetches: (s&7) ^ (row&7).  The
// four slots of a thread are 64 rows apart, so they share that chunk and
// with it the whole k-state; only the row state is per slot.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TCMM_HD __host__ __device__ inline
#else
#define TCMM_HD inline
#endif

namespace maml355 {
namespace tcmm {

constexpr int kBM = 256;          // rows per block
constexpr int kBK = 64;           // k per K-step
constexpr int kThreads = 512;
constexpr int kSlotsPerThread = 4;

struct Geom {
  int NB, H, W, Ci;   // X [NB, H, W, Ci] per task, as stored
  int Ho, Wo, pad;    // Y [NB, Ho, Wo, Co] per task; im2col pad (dgrad: 2-p)
  long Mtot;          // NB * Ho * Wo
  int K9;             // 9 * Ci
};

TCMM_HD Geom make_geom(int NB, int H, int W, int Ci, int Ho, int Wo, int pad) {
  Geom g;
  g.NB = NB; g.H = H; g.W = W; g.Ci = Ci;
  g.Ho = Ho; g.Wo = Wo; g.pad = pad;
  g.Mtot = (long)NB * Ho * Wo;
  g.K9 = 9 * Ci;
  return g;
}

TCMM_HD int slot_row(int s) { return s >> 3; }
// first k (within the K-step) of the 8 channels slot s fetches
TCMM_HD int slot_k8(int s) { return ((s & 7) ^ ((s >> 3) & 7)) * 8; }

// k-state: k = (dy*3 + dx)*Ci + c, advanced by kBK per K-step with adds and
// compares only.  dy >= 3 is exactly k >= K9, the K-tail.
struct KState { int c, dy, dx; };

TCMM_HD KState k_init(const Geom& g, int k8) {
  KState s;
  const int tap = k8 / g.Ci;
  s.c = k8 - tap * g.Ci;
  s.dy = tap / 3;
  s.dx = tap - s.dy * 3;
  return s;
}

TCMM_HD void k_advance(const Geom& g, KState& s) {
  s.c += kBK;
  while (s.c >= g.Ci) {
    s.c -= g.Ci;
    if (++s.dx == 3) { s.dx = 0; ++s.dy; }
  }
}

// row state: rb = element offset of X[img][ho-pad][wo-pad][0], which lies
// before the image — for the first image of a task before the tensor, so it
// may be negative — and is only ever used with a tap that brings it back
// inside; hb/wb = ho-pad / wo-pad.  An M-tail row gets an hb no tap can
// bring into [0, H), so the border test sends it to the zero page as well.
struct Row { int rb, hb, wb; };

constexpr int kRowInvalid = -(1 << 30);

TCMM_HD Row row_init(const Geom& g, long mg) {
  Row r;
  if (mg < g.Mtot) {
    const int wo = (int)(mg % g.Wo);
    const int ho = (int)((mg / g.Wo) % g.Ho);
    const int img = (int)(mg / ((long)g.Wo * g.Ho));
    r.hb = ho - g.pad;
    r.wb = wo - g.pad;
    r.rb = ((img * g.H + r.hb) * g.W + r.wb) * g.Ci;
  } else {
    r.hb = kRowInvalid;
    r.wb = 0;
    r.rb = 0;
  }
  return r;
}

// The slot's source: true and the element offset of its 8 channels inside
// the task's X, or false for the zero page.
TCMM_HD bool slot_src(const Geom& g, const Row& r, const KState& k, int& off) {
  off = r.rb + (k.dy * g.W + k.dx) * g.Ci + k.c;
  return k.dy < 3 && (unsigned)(r.hb + k.dy) < (unsigned)g.H &&
         (unsigned)(r.wb + k.dx) < (unsigned)g.W;
}

}  // namespace tcmm
}  // namespace maml355
