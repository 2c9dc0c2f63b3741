// Address logic of the transpose-free wgrad (wgrad_nt.hip), shared between
// the kernel and a host-side checker (tests/host/wgrad_nt_addr_check.cpp):
// everything here compiles as plain C++ so the index arithmetic is walked
// exhaustively under ASan/UBSan on the CPU before it ever drives a DMA.
//
// GEMM view (per task): dW[n][f] = sum_k im2col(X)[k][n] * dY[k][f] with
//   k = (img*Ho + ho)*Wk + wo     output position; Wk = Wo (flat, no line
//                                 padding) or, to reproduce wgrad v2's
//                                 summation order bit for bit, Wk = Wo
//                                 rounded up to 8 with zero rows for wo >= Wo
//   n = tap*C + c                 tap = ky*3 + kx, C % 8 == 0
// Both tiles sit in LDS as they sit in memory — rows are positions k,
// 16-byte chunks are 8 consecutive channels — and the MFMA's k-contiguous
// fragments come out of ds_read_b64_tr_b16.  A tile is 64 rows x 8 chunks.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WGNT_HD __host__ __device__ inline
#else
#define WGNT_HD inline
#endif

namespace maml355 {
namespace wgnt {

constexpr int kRows = 64;    // positions per K-step (tile rows)
constexpr int kChunks = 8;   // 16-byte chunks per tile row (64 channels)

struct Geom {
  int NB, H, W, C;       // X [NB, H, W, C] per task (C already a multiple of 8)
  int Ho, Wo, F, pad;    // dY [NB, Ho, Wo, F] per task
  int Wk;                // line width of the reduction index, >= Wo
  long K;                // NB * Ho * Wk
  int N9;                // 9 * C
  int dwo, dho, dimg;    // kRows positions = dimg images + dho lines + dwo cols
};

WGNT_HD Geom make_geom(int NB, int H, int W, int C, int Ho, int Wo, int F,
                       int pad, int Wk) {
  Geom g;
  g.NB = NB; g.H = H; g.W = W; g.C = C;
  g.Ho = Ho; g.Wo = Wo; g.F = F; g.pad = pad;
  g.Wk = Wk;
  g.K = (long)NB * Ho * Wk;
  g.N9 = 9 * C;
  const int lines = kRows / Wk;
  g.dwo = kRows - lines * Wk;
  g.dimg = lines / Ho;
  g.dho = lines - g.dimg * Ho;
  return g;
}

// flat position -> (image, line, column)
struct Pos { int img, ho, wo; };

WGNT_HD Pos pos_from_k(const Geom& g, long k) {
  Pos p;
  const long line = k / g.Wk;
  p.wo = (int)(k - line * g.Wk);
  p.img = (int)(line / g.Ho);
  p.ho = (int)(line - (long)p.img * g.Ho);
  return p;
}

// advance by one K-step (kRows positions) with adds and compares only.
// Right whether a tile spans many lines and images (Wk = 5) or less than
// one line (Wk = 84): after the column carry ho <= Ho, plus dho <= Ho - 1,
// so one conditional subtract restores ho < Ho.
WGNT_HD void pos_advance(const Geom& g, Pos& p) {
  p.wo += g.dwo;
  if (p.wo >= g.Wk) { p.wo -= g.Wk; p.ho += 1; }
  p.ho += g.dho;
  if (p.ho >= g.Ho) { p.ho -= g.Ho; p.img += 1; }
  p.img += g.dimg;
}

// LDS image.  `global_load_lds` writes 16-byte slot s = issue*256 + thread
// linearly, so slot s is row s>>3, stored chunk s&7, and the swizzle is a
// permutation of which SOURCE chunk the slot fetches.  A transposed read's
// 32-lane half touches rows {r, r+1, r+2, r+3, r+8, ..., r+11} (r % 4 == 0)
// x 2 adjacent chunks = 16 slots; with 128-byte rows the bank window
// (64 dwords = 16 slots) sees slot index (row&1)*8 + chunk, so row bits 1
// and 3 are XOR-ed into chunk bits 1 and 2: all 16 slots distinct.
WGNT_HD int swz(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }
WGNT_HD int slot_row(int s) { return s >> 3; }
WGNT_HD int slot_chunk(int s) { return (s & 7) ^ swz(s >> 3); }  // source chunk
// short index of (row, channel col) inside a tile
WGNT_HD int lds_idx(int row, int col) {
  return row * 64 + ((((col >> 3) ^ swz(row)) << 3) | (col & 7));
}


// Transposed read (ds_read_b64_tr_b16, guide T10) of the 16x16x32 operand:
// k-slice ks (0/1) of the tile, 16-column block cblk, 4-row block h (0/1).
// Per 16-lane group fk the instruction takes the block rows
// 32ks + 8fk + 4h .. +3; lane 4q+p of the group supplies the address of
// row q, columns 4p .. 4p+3 and receives column (lane & 15), so the two
// reads h = 0, 1 give a lane its column's k = 32ks + 8fk .. +7.  Returns the
// short index the lane supplies; bits 1 and 3 of the row (the swizzle's
// inputs) depend on the lane alone, so ks and h are constant offsets.
WGNT_HD int tr_idx(int lane, int ks, int h, int cblk) {
  const int fk = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int row = (ks << 5) | (fk << 3) | (h << 2) | q;
  return row * 64 + (((cblk ^ (swz(row) >> 1)) << 4) | (p << 2));
}

// accumulator column n = tap*C + c -> row of the [9*Cout, F] accumulator,
// or -1 for the padded channels (first layer: C = 8, Cout in {1, 3}) and
// the columns past 9C
WGNT_HD int out_row(const Geom& g, int n, int Cout) {
  if (n >= g.N9) return -1;
  const int tap = n / g.C;
  const int c = n - tap * g.C;
  return c < Cout ? tap * Cout + c : -1;
}

constexpr long kZeroPage = -1;

// A tile: chunk `ch` of position (p, k) -> element offset into the task's
// dY, or kZeroPage (k past the end, a line-padding row, channels past F).
// With Wk == Wo this is k * F + ch * 8: the tile is a contiguous slab.
WGNT_HD long a_src(const Geom& g, const Pos& p, long k, int ch) {
  if (k >= g.K || p.wo >= g.Wo || ch * 8 >= g.F) return kZeroPage;
  return ((long)(p.img * g.Ho + p.ho) * g.Wo + p.wo) * g.F + ch * 8;
}

// B column block decode: global column n (multiple of 8) -> tap offsets and
// first channel; valid=false past 9C.
struct Col { int dy, dx, c0; bool valid; };

WGNT_HD Col col_from_n(const Geom& g, int n) {
  Col c;
  c.valid = n < g.N9;
  const int tap = c.valid ? n / g.C : 0;
  c.c0 = c.valid ? n - tap * g.C : 0;
  c.dy = tap / 3 - g.pad;
  c.dx = tap % 3 - g.pad;
  return c;
}

// B tile: 8 channels of X under tap (dy, dx) at position (p, k) -> element
// offset into the task's X, or kZeroPage where the tap falls outside the
// image (the conv's zero padding), k is past the end or the column is.
WGNT_HD long b_src(const Geom& g, const Pos& p, long k, const Col& c) {
  const int hi = p.ho + c.dy;
  const int wi = p.wo + c.dx;
  if (!c.valid || k >= g.K || p.wo >= g.Wo || (unsigned)hi >= (unsigned)g.H ||
      (unsigned)wi >= (unsigned)g.W)
    return kZeroPage;
  return ((long)(p.img * g.H + hi) * g.W + wi) * g.C + c.c0;
}

}  // namespace wgnt
}  // namespace maml355
