// CPU check of the fwd/dgrad GEMM's A-staging address logic
// (howtotrainyourmamlpytorch_amd/ops/hip/tconv_mm_addr.h).  No GPU: built
// with -fsanitize=address,undefined and run by tests/test_tconv_mm_addr.py.
//
// Per shape, for the forward (pad p) and the dgrad (pad 2-p on dY) call, it
// walks every block tile, every one of the 2048 staging slots and every
// K-step the way the kernel does — k-state shared by a thread's four slots,
// advanced incrementally — and checks that
//  * the slot takes the zero page exactly when the direct definition of the
//    zero-padded im2col element says border, M-tail or K-tail;
//  * otherwise its offset is the direct definition's and [off, off+8) lies
//    inside the task's NB*H*W*Ci elements.  The 8 elements are really read
//    from a tensor of exactly T tasks, for the first and the last task, so
//    ASan sees an address before or past it;
//  * the LDS image the linear 16-byte slot writes produce, read back through
//    the kernel's swizzle, is the im2col tile.
// `range` shapes (workload size, T = 128) do the offset and bound checks
// arithmetically, with the task base added in 64 bits.

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tconv_mm_addr.h"

using namespace maml355::tcmm;

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

// the kernel's ds_read side (tconv.hip swz64): short index of (row, col)
static int swz64(int row, int col) { return (row * 64 + col) ^ ((row & 7) << 3); }

// X value that encodes its own position, so a read of the wrong pixel shows
static uint16_t xval(long task_elem) { return (uint16_t)(1 + task_elem % 65521); }

// one call: X [T, NB, H, W, Ci] -> Y [T, NB, Ho, Wo, *] with im2col pad `pad`
static void walk(const char* what, int T, int NB, int H, int W, int Ci, int pad,
                 bool range_only) {
  const int Ho = H + 2 * pad - 2, Wo = W + 2 * pad - 2;
  const Geom g = make_geom(NB, H, W, Ci, Ho, Wo, pad);
  const long task = (long)NB * H * W * Ci;
  const long total = task * T;
  const int K9 = 9 * Ci;
  const int ksteps = (K9 + kBK - 1) / kBK;
  const long ntile = (g.Mtot + kBM - 1) / kBM;
  CHECK(g.Mtot == (long)NB * Ho * Wo && g.K9 == K9, "geom");

  std::vector<uint16_t> x;
  if (!range_only) {
    x.resize(total);
    for (int t = 0; t < T; ++t)
      for (long e = 0; e < task; ++e) x[t * task + e] = xval(e);
  }
  const uint16_t zpage[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long nzero = 0, nsrc = 0;
  std::vector<uint16_t> lds(kBM * kBK);

  for (long tile = 0; tile < ntile; ++tile) {
    // workload sizes: first, second, an inner and the last two tiles
    if (range_only && tile > 1 && tile < ntile - 2 && tile != ntile / 2) continue;
    const long m0 = tile * kBM;
    // per-thread state exactly as the kernel keeps it
    std::vector<KState> ks_state(kThreads);
    std::vector<Row> rows(kThreads * kSlotsPerThread);
    for (int tid = 0; tid < kThreads; ++tid) {
      ks_state[tid] = k_init(g, slot_k8(tid));
      for (int q = 0; q < kSlotsPerThread; ++q) {
        const int s = q * kThreads + tid;
        CHECK(slot_k8(s) == slot_k8(tid), "slot %d does not share tid's k8", s);
        rows[q * kThreads + tid] = row_init(g, m0 + slot_row(s));
      }
    }
    for (int ks = 0; ks < ksteps; ++ks) {
      for (int tid = 0; tid < kThreads; ++tid)
        for (int q = 0; q < kSlotsPerThread; ++q) {
          const int s = q * kThreads + tid;
          int off = 0;
          const bool in =
              slot_src(g, rows[q * kThreads + tid], ks_state[tid], off);
          // direct definition of the zero-padded im2col element
          const long m = m0 + slot_row(s);
          const int k = ks * kBK + slot_k8(s);
          bool want_in = false;
          long want = 0;
          if (m < g.Mtot && k < K9) {
            const int wo = (int)(m % Wo), ho = (int)(m / Wo % Ho);
            const long img = m / ((long)Wo * Ho);
            const int tap = k / Ci, c = k % Ci;
            // coordinates in the zero-bordered image [H+2p, W+2p]
            const int hp = ho + tap / 3, wp = wo + tap % 3;
            want_in = hp >= pad && hp < H + pad && wp >= pad && wp < W + pad;
            if (want_in)
              want = ((img * H + (hp - pad)) * W + (wp - pad)) * Ci + c;
          }
          CHECK(in == want_in, "%s zero-page decision m=%ld k=%d: got %d want %d",
                what, m, k, (int)in, (int)want_in);
          const uint16_t* src = zpage;
          if (in) {
            ++nsrc;
            CHECK(off == want, "%s off m=%ld k=%d got %d want %ld", what, m, k,
                  off, want);
            CHECK(off >= 0 && (long)off + 8 <= task, "%s range m=%ld k=%d off %d",
                  what, m, k, off);
            const long last = (long)(T - 1) * task + off;
            CHECK(last >= 0 && last + 8 <= total, "%s last-task range", what);
            if (!range_only) {
              // really read, first and last task: Xt + off as the kernel forms it
              const uint16_t* first_p = x.data() + off;
              const uint16_t* last_p = x.data() + (long)(T - 1) * task + off;
              for (int j = 0; j < 8; ++j) {
                CHECK(first_p[j] == xval(want + j), "%s value", what);
                CHECK(last_p[j] == xval(want + j), "%s value (last task)", what);
              }
              src = first_p;
            }
          } else {
            ++nzero;
          }
          if (!range_only)
            for (int j = 0; j < 8; ++j) lds[(long)s * 8 + j] = src[j];
        }
      if (!range_only) {
        // the tile as the MFMA fragments read it
        for (int row = 0; row < kBM; ++row)
          for (int col = 0; col < kBK; ++col) {
            const long m = m0 + row;
            const int k = ks * kBK + col;
            uint16_t want = 0;
            if (m < g.Mtot && k < K9) {
              const int wo = (int)(m % Wo), ho = (int)(m / Wo % Ho);
              const long img = m / ((long)Wo * Ho);
              const int tap = k / Ci, c = k % Ci;
              const int h = ho + tap / 3 - pad, w = wo + tap % 3 - pad;
              if (h >= 0 && h < H && w >= 0 && w < W)
                want = xval(((img * H + h) * W + w) * Ci + c);
            }
            CHECK(lds[swz64(row, col)] == want, "%s lds image row %d col %d",
                  what, row, col);
          }
      }
      for (int tid = 0; tid < kThreads; ++tid) k_advance(g, ks_state[tid]);
    }
  }
  std::printf("walk %-5s T%d NB%d %dx%d Ci%d pad%d -> %dx%d, %ld tiles x %d "
              "ksteps: %ld tensor slots, %ld zero-page slots%s\n",
              what, T, NB, H, W, Ci, pad, Ho, Wo, ntile, ksteps, nsrc, nzero,
              range_only ? " (range-only)" : "");
}

static void both(const Shape& s, bool range_only) {
  const int Ho = s.H + 2 * s.pad - 2, Wo = s.W + 2 * s.pad - 2;
  walk("fwd", s.T, s.NB, s.H, s.W, s.C, s.pad, range_only);
  // dgrad: the same kernel on dY [NB, Ho, Wo, F] with pad 2-p gives [H, W]
  walk("dgrad", s.T, s.NB, Ho, Wo, s.F, 2 - s.pad, range_only);
}

int main() {
  const Shape full[] = {
      {2, 3, 11, 9, 48, 48, 1},  {2, 3, 12, 11, 64, 64, 0},
      {2, 3, 7, 7, 8, 8, 1},     {1, 2, 3, 3, 16, 32, 0},
      {1, 1, 1, 1, 8, 8, 1},     {3, 7, 21, 21, 48, 48, 1},
      {2, 3, 10, 10, 16, 48, 1},
      // the restored padded-copy path: the kernel on a bordered copy, pad 0
      {2, 3, 13, 11, 48, 48, 0},
  };
  // conv layers 1-3 of the two bench workloads, target pass, 128 tasks
  const Shape range[] = {
      {128, 75, 42, 42, 48, 48, 1}, {128, 75, 21, 21, 48, 48, 1},
      {128, 75, 10, 10, 48, 48, 1}, {128, 100, 14, 14, 64, 64, 1},
      {128, 100, 7, 7, 64, 64, 1},  {128, 100, 3, 3, 64, 64, 1},
  };
  for (const Shape& s : full) both(s, false);
  for (const Shape& s : range) both(s, true);
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
