// CPU check of the transpose-free wgrad's address logic
// (howtotrainyourmamlpytorch_amd/ops/hip/wgrad_nt_addr.h).  No GPU: built
// with -fsanitize=address,undefined and run by tests/test_wgrad_nt_addr.py.
//
// Per shape it
//  1. walks every staging slot over every K-step of every K-chunk and checks
//     the incremental (img, ho, wo) state against the closed form, every
//     source offset against the tensor bounds (the 8 elements are really
//     read, so ASan sees an overrun), and the in-image / zero-page decision
//     against the definition of a zero-padded 3x3 convolution;
//  2. emulates the whole block — linear slot writes of the 16-byte chunks,
//     ds_read_b64_tr_b16 per 16-lane group, the 16x16x32 MFMA lane maps,
//     the ones column / column sums, the epilogue — on small integers and
//     compares dW and db exactly with the direct definition.
// `range` shapes (workload size) do step 1's offset checks only, with the
// task base added, where 32-bit arithmetic would overflow.

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wgrad_nt_addr.h"

using namespace maml355::wgnt;

static int g_fail = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__);      \
                         std::printf(__VA_ARGS__); std::printf("\n"); }        \
      ++g_fail;                                                                \
    }                                                                          \
  } while (0)

struct Shape { int T, NB, H, W, C, F, pad; };

static uint16_t bf16_of_int(int v) {  // small ints are exact in bf16
  float f = (float)v;
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return (uint16_t)(u >> 16);
}
static float f_of_bf16(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// ---- 1. address walk ------------------------------------------------------
static void walk(const Shape& s, bool range_only, bool pad8) {
  const int Cp = s.C % 8 ? 8 : s.C;
  const int Ho = s.H + 2 * s.pad - 2, Wo = s.W + 2 * s.pad - 2;
  const int Wk = pad8 ? (Wo + 7) / 8 * 8 : Wo;  // v2-compatible line padding
  const Geom g = make_geom(s.NB, s.H, s.W, Cp, Ho, Wo, s.F, s.pad, Wk);
  const long K = g.K;
  const long Kr = (K + kRows - 1) / kRows * kRows;
  const long dy_task = (long)s.NB * Ho * Wo * s.F;
  const long x_task = (long)s.NB * s.H * s.W * Cp;
  const long dy_total = dy_task * s.T, x_total = x_task * s.T;
  std::vector<uint16_t> dy, x;
  if (!range_only) { dy.assign(dy_task, 1); x.assign(x_task, 1); }
  const long chunks[3] = {kRows, 3 * kRows, Kr};
  const int nchunk = range_only ? 1 : 3;
  unsigned sink = 0;
  for (int ci = 0; ci < nchunk; ++ci) {
    const long kchunk = range_only ? 4096 : chunks[ci];
    for (long kc0 = 0; kc0 < Kr; kc0 += kchunk) {
      const long kc_end = kc0 + kchunk < Kr ? kc0 + kchunk : Kr;
      for (int slot = 0; slot < 512; ++slot) {
        const int row = slot_row(slot), ch = slot_chunk(slot);
        CHECK(row >= 0 && row < kRows && ch >= 0 && ch < kChunks, "slot %d", slot);
        long k = kc0 + row;
        Pos p = pos_from_k(g, k);
        for (long k0 = kc0; k0 < kc_end; k0 += kRows) {
          // closed form, written differently from pos_from_k
          const long img = k / ((long)Ho * Wk);
          const long rem = k - img * Ho * Wk;
          const int ho = (int)(rem / Wk), wo = (int)(rem % Wk);
          CHECK(p.img == img && p.ho == ho && p.wo == wo,
                "pos k=%ld got (%d,%d,%d) want (%ld,%d,%d)", k, p.img, p.ho,
                p.wo, img, ho, wo);
          // A
          const long ao = a_src(g, p, k, ch);
          const bool a_zero = k >= K || wo >= Wo || ch * 8 >= s.F;
          CHECK((ao == kZeroPage) == a_zero, "a zero k=%ld ch=%d", k, ch);
          if (ao != kZeroPage) {
            CHECK(ao == ((img * Ho + ho) * Wo + wo) * s.F + ch * 8, "a off");
            if (!pad8) CHECK(ao == k * s.F + ch * 8, "a tile not a slab");
            CHECK(ao >= 0 && ao + 8 <= dy_task, "a range %ld", ao);
            const long full = (long)(s.T - 1) * dy_task + ao;
            CHECK(full + 8 <= dy_total && full >= ao, "a full range");
            if (!range_only)
              for (int j = 0; j < 8; ++j) sink += dy[ao + j];
          }
          // B: every column block this chunk position serves
          for (int n = ch * 8; n < g.N9 + 128; n += 64) {
            const Col c = col_from_n(g, n);
            const long bo = b_src(g, p, k, c);
            bool inside = false;
            long want = -1;
            if (n < g.N9 && k < K && wo < Wo) {
              const int tap = n / Cp, c0 = n % Cp;
              const int ky = tap / 3, kx = tap % 3;
              // coordinates in the zero-padded image [H+2p, W+2p]
              const int hp = ho + ky, wp = wo + kx;
              inside = hp >= s.pad && hp < s.H + s.pad && wp >= s.pad &&
                       wp < s.W + s.pad;
              if (inside)
                want = (((long)img * s.H + (hp - s.pad)) * s.W + (wp - s.pad)) *
                           Cp + c0;
            }
            CHECK((bo != kZeroPage) == inside, "b zero k=%ld n=%d", k, n);
            if (bo != kZeroPage) {
              CHECK(bo == want, "b off k=%ld n=%d got %ld want %ld", k, n, bo, want);
              CHECK(bo >= 0 && bo + 8 <= x_task, "b range %ld", bo);
              const long full = (long)(s.T - 1) * x_task + bo;
              CHECK(full + 8 <= x_total && full >= bo, "b full range");
              if (!range_only && bo + 8 <= x_task)
                for (int j = 0; j < 8; ++j) sink += x[bo + j];
            }
          }
          k += kRows;
          pos_advance(g, p);
        }
      }
    }
  }
  if (range_only) {
    // the largest offsets do not fit 32 bits at workload size: make sure the
    // check above really saw them as 64-bit values
    CHECK(dy_total > 0 && x_total > 0, "totals");
  }
  std::printf("walk  T%d NB%d %dx%d C%d F%d pad%d Wk=%d K=%ld %s (sink %u)\n",
              s.T, s.NB, s.H, s.W, s.C, s.F, s.pad, Wk, K,
              range_only ? "range-only" : "full", sink & 1);
}

// ---- 2. block emulation ---------------------------------------------------
// ds_read_b64_tr_b16: lane i of a 16-lane group receives column i of the
// group's 4x16 block, row q in element q; row q, columns 4p..4p+3 sit at
// the address supplied by lane 4q+p of the group.
static void tr_read(const uint16_t* tile, int ks, int h, int cblk,
                    uint16_t out[64][4]) {
  for (int lane = 0; lane < 64; ++lane) {
    const int grp = lane & ~15, i = lane & 15;
    for (int q = 0; q < 4; ++q) {
      const int src_lane = grp + 4 * q + (i >> 2);
      const int idx = tr_idx(src_lane, ks, h, cblk);
      if (idx < 0 || idx + 4 > 64 * 64 || (idx & 3)) {
        CHECK(false, "tr_idx %d out of tile / misaligned", idx);
        out[lane][q] = 0;
        continue;
      }
      out[lane][q] = tile[idx + (i & 3)];
    }
  }
}

static void emulate(const Shape& s, int nsub, long kchunk_req, bool pad8) {
  const int Cp = s.C % 8 ? 8 : s.C;
  const int Ho = s.H + 2 * s.pad - 2, Wo = s.W + 2 * s.pad - 2;
  const int Wk = pad8 ? (Wo + 7) / 8 * 8 : Wo;
  const Geom g = make_geom(s.NB, s.H, s.W, Cp, Ho, Wo, s.F, s.pad, Wk);
  const long K = (long)s.NB * Ho * Wo;  // real positions
  const long Kr = (g.K + kRows - 1) / kRows * kRows;
  const int F = s.F, N9 = g.N9, wgn = 64 * nsub;
  const int gridx = (N9 + wgn - 1) / wgn;
  const bool ones = !pad8 && gridx * wgn > N9;  // deterministic: column sums
  const int ones_col = ones ? N9 : -1;
  const int ncols = N9 + (ones ? 1 : 0);
  const int mtiles = (F + 15) / 16;
  // one task; X holds the padded channels as zeros, as the pad kernel writes
  std::vector<uint16_t> dy(K * F), x((long)s.NB * s.H * s.W * Cp, 0);
  std::vector<int> dyi(K * F), xi((long)s.NB * s.H * s.W * s.C);
  uint32_t rng = 12345u + (uint32_t)(K * 31 + F);
  auto rnd = [&]() { rng = rng * 1664525u + 1013904223u; return (int)((rng >> 24) % 5) - 2; };
  for (long i = 0; i < K * F; ++i) { dyi[i] = rnd(); dy[i] = bf16_of_int(dyi[i]); }
  for (long m = 0; m < (long)s.NB * s.H * s.W; ++m)
    for (int c = 0; c < s.C; ++c) {
      const int v = rnd();
      xi[m * s.C + c] = v;
      x[m * Cp + c] = bf16_of_int(v);
    }
  const uint16_t zpage[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<double> dw((long)9 * s.C * F, 0.0), db(F, 0.0);

  const long kchunk = kchunk_req;
  for (int bx = 0; bx < gridx; ++bx)
    for (long kc0 = 0; kc0 < Kr; kc0 += kchunk) {
      const long kc_end = kc0 + kchunk < Kr ? kc0 + kchunk : Kr;
      const int n0 = bx * wgn;
      std::vector<float> acc((size_t)4 * nsub * 4 * 64 * 4, 0.f);  // [wave][sb][mt][lane][j]
      std::vector<double> colsum(F, 0.0);
      Pos pos[512];
      long kk[512];
      for (int slot = 0; slot < 512; ++slot) {
        kk[slot] = kc0 + slot_row(slot);
        pos[slot] = pos_from_k(g, kk[slot]);
      }
      for (long k0 = kc0; k0 < kc_end; k0 += kRows) {
        std::vector<uint16_t> la(64 * 64, 0xFFFF);
        std::vector<std::vector<uint16_t>> lb(nsub, std::vector<uint16_t>(64 * 64, 0xFFFF));
        for (int slot = 0; slot < 512; ++slot) {  // linear 16-byte slot writes
          const int ch = slot_chunk(slot);
          const long ao = a_src(g, pos[slot], kk[slot], ch);
          const uint16_t* as = ao == kZeroPage ? zpage : &dy[ao];
          for (int j = 0; j < 8; ++j) la[slot * 8 + j] = as[j];
          for (int sb = 0; sb < nsub; ++sb) {
            const Col c = col_from_n(g, n0 + sb * 64 + ch * 8);
            const long bo = b_src(g, pos[slot], kk[slot], c);
            const uint16_t* bs = bo == kZeroPage ? zpage : &x[bo];
            for (int j = 0; j < 8; ++j) lb[sb][slot * 8 + j] = bs[j];
          }
          kk[slot] += kRows;
          pos_advance(g, pos[slot]);
        }
        for (int wave = 0; wave < 4; ++wave)
          for (int ks = 0; ks < 2; ++ks)
            for (int sb = 0; sb < nsub; ++sb) {
              const int nsub0 = n0 + (sb * 4 + wave) * 16;
              if (nsub0 >= ncols) continue;
              uint16_t b0[64][4], b1[64][4], bfrag[64][8];
              tr_read(lb[sb].data(), ks, 0, wave, b0);
              tr_read(lb[sb].data(), ks, 1, wave, b1);
              for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 4; ++j) {
                  bfrag[l][j] = b0[l][j];
                  bfrag[l][4 + j] = b1[l][j];
                  if (nsub0 + (l & 15) == ones_col)
                    bfrag[l][j] = bfrag[l][4 + j] = 0x3F80;
                }
              for (int mt = 0; mt < mtiles; ++mt) {
                uint16_t a0[64][4], a1[64][4], afrag[64][8];
                tr_read(la.data(), ks, 0, mt, a0);
                tr_read(la.data(), ks, 1, mt, a1);
                for (int l = 0; l < 64; ++l)
                  for (int j = 0; j < 4; ++j) {
                    afrag[l][j] = a0[l][j];
                    afrag[l][4 + j] = a1[l][j];
                  }
                // v_mfma_f32_16x16x32_bf16: lane 16*kg + r holds row r
                // (A) / column r (B), k = 8kg..8kg+7; D[4kg+j][r] in lane
                float* d = &acc[((((size_t)wave * nsub + sb) * 4 + mt) * 64) * 4];
                for (int l = 0; l < 64; ++l)
                  for (int j = 0; j < 4; ++j) {
                    const int m = (l >> 4) * 4 + j, n = l & 15;
                    float v = 0.f;
                    for (int kg = 0; kg < 4; ++kg)
                      for (int e = 0; e < 8; ++e)
                        v += f_of_bf16(afrag[kg * 16 + m][e]) *
                             f_of_bf16(bfrag[kg * 16 + n][e]);
                    d[l * 4 + j] += v;
                  }
              }
            }
        if (!ones && bx == 0)
          for (int f = 0; f < F; ++f)
            for (int r = 0; r < 64; ++r)
              colsum[f] += f_of_bf16(la[lds_idx(r, f)]);
      }
      // epilogue
      for (int wave = 0; wave < 4; ++wave)
        for (int sb = 0; sb < nsub; ++sb)
          for (int l = 0; l < 64; ++l) {
            const int n = n0 + (sb * 4 + wave) * 16 + (l & 15);
            const int orow = out_row(g, n, s.C);
            for (int mt = 0; mt < mtiles; ++mt)
              for (int j = 0; j < 4; ++j) {
                const int f = mt * 16 + (l >> 4) * 4 + j;
                if (f >= F) continue;
                const float v = acc[((((size_t)wave * nsub + sb) * 4 + mt) * 64 + l) * 4 + j];
                if (orow >= 0) dw[(long)orow * F + f] += v;
                else if (n == ones_col) db[f] += v;
              }
          }
      if (!ones && bx == 0)
        for (int f = 0; f < F; ++f) db[f] += colsum[f];
    }

  // direct definition
  long bad = 0;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx)
      for (int c = 0; c < s.C; ++c)
        for (int f = 0; f < F; ++f) {
          long ref = 0;
          for (int n = 0; n < s.NB; ++n)
            for (int ho = 0; ho < Ho; ++ho)
              for (int wo = 0; wo < Wo; ++wo) {
                const int hi = ho + ky - s.pad, wi = wo + kx - s.pad;
                if (hi < 0 || hi >= s.H || wi < 0 || wi >= s.W) continue;
                ref += (long)dyi[(((long)n * Ho + ho) * Wo + wo) * F + f] *
                       xi[(((long)n * s.H + hi) * s.W + wi) * s.C + c];
              }
          const double got = dw[((long)(ky * 3 + kx) * s.C + c) * F + f];
          if (got != (double)ref) ++bad;
        }
  for (int f = 0; f < F; ++f) {
    long ref = 0;
    for (long k = 0; k < K; ++k) ref += dyi[k * F + f];
    if (db[f] != (double)ref) ++bad;
  }
  CHECK(bad == 0, "emulation: %ld wrong dW/db entries", bad);
  std::printf("emul  T%d NB%d %dx%d C%d F%d pad%d Wk%d nsub%d kchunk%ld %s: %s\n",
              s.T, s.NB, s.H, s.W, s.C, s.F, s.pad, Wk, nsub, kchunk,
              ones ? "ones-col" : "colsum", bad ? "MISMATCH" : "ok");
}

// bank check of the transposed reads: per 32-lane half the 32 8-byte
// accesses must fall on 64 distinct dword banks ((byte/4) % 64)
static void banks() {
  for (int ks = 0; ks < 2; ++ks)
    for (int h = 0; h < 2; ++h)
      for (int cblk = 0; cblk < 4; ++cblk)
        for (int half = 0; half < 2; ++half) {
          int hit[64] = {0};
          for (int l = half * 32; l < half * 32 + 32; ++l) {
            const int byte = tr_idx(l, ks, h, cblk) * 2;
            CHECK(byte % 8 == 0, "tr address not 8-byte aligned");
            ++hit[(byte / 4) % 64];
            ++hit[(byte / 4 + 1) % 64];
          }
          for (int b = 0; b < 64; ++b)
            CHECK(hit[b] == 1, "bank %d hit %d times (ks%d h%d c%d half%d)", b,
                  hit[b], ks, h, cblk, half);
        }
  std::printf("banks ok\n");
}

int main() {
  const Shape full[] = {
      {2, 3, 11, 9, 48, 48, 1},  {2, 3, 12, 11, 64, 64, 0},
      {2, 3, 7, 7, 8, 16, 1},    {2, 3, 7, 7, 8, 8, 1},
      {2, 5, 14, 14, 3, 48, 1},  {2, 5, 14, 14, 1, 64, 1},
      {1, 2, 3, 3, 16, 32, 0},   {2, 3, 5, 5, 16, 16, 1},
      {1, 2, 6, 84, 48, 48, 1},  {3, 7, 21, 21, 48, 48, 1},
      {2, 3, 14, 14, 48, 48, 1}, {2, 3, 14, 14, 8, 16, 1},
      {2, 2, 8, 8, 48, 48, 1},
  };
  const Shape range[] = {
      {128, 75, 84, 84, 3, 48, 1}, {128, 75, 42, 42, 48, 48, 1},
      {128, 75, 21, 21, 48, 48, 1}, {128, 75, 10, 10, 48, 48, 1},
  };
  banks();
  for (const Shape& s : full) { walk(s, false, false); walk(s, false, true); }
  for (const Shape& s : range) { walk(s, true, false); walk(s, true, true); }
  // emulation on the cheaper shapes, both block widths where 9C > 64
  const Shape emu[] = {
      {1, 3, 11, 9, 48, 48, 1}, {1, 3, 12, 11, 64, 64, 0},
      {1, 3, 7, 7, 8, 16, 1},   {1, 3, 7, 7, 8, 8, 1},
      {1, 5, 14, 14, 3, 48, 1}, {1, 5, 14, 14, 1, 64, 1},
      {1, 2, 3, 3, 16, 32, 0},  {1, 3, 5, 5, 16, 16, 1},
      {1, 2, 6, 84, 48, 48, 1},
  };
  for (const Shape& s : emu) {
    emulate(s, 1, 128, false);
    emulate(s, 2, 1 << 20, false);
    emulate(s, 1, 192, true);
    emulate(s, 2, 1 << 20, true);
  }
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
