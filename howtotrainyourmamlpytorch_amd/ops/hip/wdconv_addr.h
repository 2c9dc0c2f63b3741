// Address logic of the wide first-layer forward (wdconv_fwd_kernel in
// wdconv.hip), shared between the kernel and a host-side checker
// (tests/host/wdconv_addr_check.cpp): everything here compiles as plain C++,
// so the index arithmetic is walked under ASan/UBSan on the CPU.
//
// Per task the output is NL = NB*Ho lines of Wo positions.  A chunk is R
// consecutive lines (the last chunk of a task may be shorter) and may cross
// image boundaries.  Its input is staged in LDS as rows of the zero-PADDED
// images, of which output line ho reads rows S*ho .. S*ho + 2 (S = stride):
// an image contributes SR = S*(Ho-1) + 3 rows (stride 2 with even H + 2 pad
// leaves a trailing input row that no output touches: it is not a row here).
// Staged row 0 is padded row S*ho0 of image img0, the chunk's first line;
// staged row r is padded row (S*ho0 + r) % SR of image img0 + (S*ho0 + r) / SR.
// SR - S*Ho = 3 - S, so line l of the chunk starts at staged row
// S*l + (3 - S) * (images crossed).  A staged row holds the S*(Wo-1) + 3
// padded columns a line reads.  The halo (left/right columns, rows above and
// below an image, images past the task's last) is written as zeros: a window
// read needs no predicate.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WDC_HD __host__ __device__ inline
#else
#define WDC_HD inline
#endif

namespace maml355 {
namespace wdc {

constexpr int kThreads = 256;            // block size: 4 waves
constexpr int kWaves = 4;
constexpr int kTile = 16;                // positions per MFMA tile
constexpr int kStep = kWaves * kTile;    // positions a wave advances per tile
constexpr int kNLD = 16;                 // staging loads per thread per chunk
constexpr int kCap = kNLD * kThreads;    // elements (2 bytes) per LDS buffer
constexpr int kChunkMin = 256;           // positions per chunk: at least 16
constexpr int kChunkMax = 1024;          // tiles, at most 64
constexpr int kWantChunks = 512;         // chunks per launch worth cutting for

struct Geom {
  int NB, H, W, C, pad, S;
  int Ho, Wo, SR, RS;    // RS: elements per staged row
  int NL;                // NB * Ho output lines per task
  int R;                 // lines per chunk; 0: the shape does not fit
  int nchunks;           // per task
  int rows, nslots;      // staged rows per chunk, rows * RS
  unsigned mRS, mSR, mHo, mWo;  // multiply-high reciprocals (divisor > 1)
};

// ceil(2^32 / d), d >= 2: umulhi(n, magic(d)) == n / d whenever n * d <= 2^32
WDC_HD unsigned magic(int d) {
  return (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d);
}
WDC_HD int udiv2(int n, unsigned m) {  // divisor >= 2
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)__umulhi((unsigned)n, m);
#else
  return (int)(((unsigned long long)(unsigned)n * m) >> 32);
#endif
}
WDC_HD int udiv(int n, int d, unsigned m) {
  const int q = udiv2(n, m);
  return d == 1 ? n : q;
}

WDC_HD int out_dim(int h, int pad, int S) { return (h + 2 * pad - 3) / S + 1; }

// staged rows R lines can need: S*(R-1) + 3, plus 3 - S per image boundary
WDC_HD int staged_rows(int R, int Ho, int S) {
  return S * (R - 1) + 3 + (3 - S) * ((R - 1 + Ho - 1) / Ho);
}

// R is the most lines whose staged rows fit kCap, up to kChunkMax positions;
// where that leaves the launch fewer than kWantChunks chunks it comes down to
// as few as kChunkMin positions
WDC_HD Geom make_geom(int T, int NB, int H, int W, int C, int pad, int S) {
  Geom g;
  g.NB = NB; g.H = H; g.W = W; g.C = C; g.pad = pad; g.S = S;
  g.Ho = out_dim(H, pad, S); g.Wo = out_dim(W, pad, S);
  g.SR = S * (g.Ho - 1) + 3;
  g.RS = (S * (g.Wo - 1) + 3) * C;
  g.NL = NB * g.Ho;
  int R = kChunkMax / g.Wo;
  if (R < 1) R = 1;
  if (R > g.NL) R = g.NL;
  while (R >= 1 && (long)staged_rows(R, g.Ho, S) * g.RS > kCap) --R;
  const int Rmin = (kChunkMin + g.Wo - 1) / g.Wo;
  while (R > Rmin && (long)T * ((g.NL + R - 1) / R) < kWantChunks) --R;
  g.R = R < 1 ? 0 : R;
  g.nchunks = g.R ? (g.NL + g.R - 1) / g.R : 0;
  g.rows = g.R ? staged_rows(g.R, g.Ho, S) : 0;
  g.nslots = g.rows * g.RS;
  g.mRS = magic(g.RS); g.mSR = magic(g.SR);
  g.mHo = magic(g.Ho > 1 ? g.Ho : 2); g.mWo = magic(g.Wo > 1 ? g.Wo : 2);
  return g;
}

// Blocks per task (grid.x): about 1024 blocks per launch, and at least two
// chunks per block where a task has them, so the weight fragments are loaded
// once for both and the prefetch has a chunk to fetch.  Block b walks chunks
// b, b + grid_x, ..
WDC_HD int grid_x(const Geom& g, int T) {
  const int fill = (1024 + T - 1) / T;
  const int half = (g.nchunks + 1) / 2;
  const int gx = half < fill ? half : fill;
  return gx < 1 ? 1 : gx;
}

// first line of chunk ck
struct Chunk { int L0, img0, ho0; };
WDC_HD Chunk chunk_at(const Geom& g, int ck) {
  Chunk c;
  c.L0 = ck * g.R;
  c.img0 = udiv(c.L0, g.Ho, g.mHo);  // the launcher checks NL * Ho <= 2^32
  c.ho0 = c.L0 - c.img0 * g.Ho;
  return c;
}

// Staging: LDS element slot s of a chunk that starts at (img0, ho0) ->
// element offset into the task's x, or -1 for a zero (halo, an image past
// the task's last, a slot past the staged rows).  img0 >= NB gives all zeros.
// It comes in two halves.  slot_static is the part that is the same for every
// chunk, computed once per thread: staged row | image column element << 12,
// or kSlotNever for a slot that is always a zero (past the staged rows, the
// left/right halo).  slot_dyn places it in the chunk; kSlotNever pushes h out
// of range, so one compare decides (no per-slot predicate to keep around).
static_assert(kCap <= 4096, "slot_static packs rows and columns in 12 bits");
constexpr int kSlotNever = 1 << 30;
WDC_HD int slot_static(const Geom& g, int s) {
  const int row = udiv2(s, g.mRS);      // RS, SR >= 3
  const int cw = s - row * g.RS - g.pad * g.C;
  const bool ok = row < g.rows && (unsigned)cw < (unsigned)(g.W * g.C);
  return ok ? (row | (cw << 12)) : kSlotNever;
}
WDC_HD int slot_dyn(const Geom& g, int img0, int ho0, int st) {
  const int rel = g.S * ho0 + (st & 0xfff);
  const int irel = udiv2(rel, g.mSR);
  const int h = rel - irel * g.SR - g.pad + (st & kSlotNever);
  const int img = img0 + irel;
  const bool ok = img < g.NB && (unsigned)h < (unsigned)g.H;
  return ok ? ((img * g.H + h) * g.W) * g.C + ((st >> 12) & 0xfff) : -1;
}
WDC_HD int slot_src(const Geom& g, int img0, int ho0, int s) {
  return slot_dyn(g, img0, ho0, slot_static(g, s));
}

// Window reads: LDS element offset = pos_base(position) + k_off(k), with
// k = (ky*3 + kx)*C + c = ky*3C + r: the 3C values of one ky are one
// contiguous run of a staged row.  k >= 9C is the zero fill: offset 0, masked.
WDC_HD int k_off(const Geom& g, int k) {
  const int ky = (k >= 3 * g.C ? 1 : 0) + (k >= 6 * g.C ? 1 : 0);
  return k < 9 * g.C ? ky * g.RS + (k - ky * 3 * g.C) : 0;
}

// position q = l * Wo + wo of a chunk whose first line is ho0 of its image
WDC_HD int pos_base(const Geom& g, int ho0, int q) {
  const int l = udiv(q, g.Wo, g.mWo);
  const int wo = q - l * g.Wo;
  const int cross = udiv(ho0 + l, g.Ho, g.mHo);
  return (g.S * l + (3 - g.S) * cross) * g.RS + wo * g.S * g.C;
}

// Weight rows: MFMA tile nt (0..3) of a 64-channel group holds, in its row r,
// the channel below, so that the accumulators of tiles 2h and 2h+1 leave lane
// group gq = r>>2 the 8 CONSECUTIVE channels 32h + 8gq .. +7 of one position.
WDC_HD int tile_channel(int nt, int r) {
  return 32 * (nt >> 1) + 8 * (r >> 2) + 4 * (nt & 1) + (r & 3);
}

}  // namespace wdc
}  // namespace maml355
