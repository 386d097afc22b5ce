// Host-side AddressSanitizer + UndefinedBehaviorSanitizer check of the launch planners
// (SURVEY.md §5.2 "host-side ASan for the C++ extension").  GPU ASan is not available on
// this pool, so the device code is covered by the guard-buffer bounds tests
// (tests/test_kernels_gpu.py::test_out_params_respect_bounds); this harness covers the
// torch-free host code that plans a launch, compiled from the same .hip files as the library:
//   conv3_fwd_plan    (with conv3d_ds_plan, conv3_res_plan, conv3_fwd_grid): kernel, tile
//                     configuration, grid, split-K and statistics rows of the 3x3 conv
//   conv3_wgrad_plan  (with conv3d_wgrad_ds_plan, conv3_wgrad_c32_plan): kernel, tiles, splits
//   convt_wgrad_plan, convt_bwd_fused_ok / convt_bwd_fused_splits: kernel, splits and the
//                     32-bit buffer-descriptor span bounds of the transposed-conv gradients
//   bn_bwd_reduce_blocks, reduce_rows_chunks, reduce_rows_scatter_tmp, head_supported
// and the host side of csrc/data_math.h, the input pipeline's recipe (the text the kernels and
// the CPU twins both run): mirror index, D4 maps, scene choice, and the warp's fixed-point
// coordinates at the extremes its validity predicate admits (no signed overflow: UBSan)
// and of csrc/bn_math.h, the BatchNorm / gradient-tail recipe: the slab permutation is a
// bijection, stats4 at its edge inputs, the three summation orders at the regime borders
// over the geometry range the U-Net uses (2-D 8^2..1024^2, 3-D 8^3..128^3, batch 1..256), the
// U-Net's channel pairs in both directions, BN groups 1 / 2 / 4, with and without the
// prologues and the BN-backward epilogue, at 8, 248 and 256 CUs, asserting the invariants the
// kernels rely on.  Not covered: the launchers' own template dispatch, the tensor checks and
// allocations of csrc/bindings.cpp, and the grids of the kernels without a planner of their
// own (head, BatchNorm apply, convT forward / data gradient, input pipeline).
// No GPU is touched (no HIP API calls).
//
//   host_sanitize          the sweeps
//   host_sanitize --table  one line per case of the fixed list below:
//                          op | shape | num_cus | path | grid | splits/ksplit | tile
//                          (tests/golden/launch_plans.txt; docs/TESTING.md "Launch plans")
//
// Build + run (scripts/host_sanitize.sh):
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address \
//         -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=all ...
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <climits>

#include <vector>

#include "../csrc/bn_math.h"
#include "../csrc/data_math.h"
#include "../csrc/ops.h"

using namespace ddlpc;

// the planners read tuning knobs; bindings.cpp (torch-linked) is not part of this harness,
// so knobs resolve to the sweep's override, their DDLPC_<NAME> environment value or the default
// (--table: always the default, so the committed table never depends on the caller's environment)
static int g_wide_knob = -1;   // CONVT_WGRAD_WIDE for the convT sweep (-1: unset)
static bool g_knob_defaults = false;
int ddlpc::knob(const char* name, int def) {
  if (g_knob_defaults) return def;
  if (std::strcmp(name, "CONVT_WGRAD_WIDE") == 0 && g_wide_knob >= 0) return g_wide_knob;
  char env[128];
  std::snprintf(env, sizeof(env), "DDLPC_%s", name);
  const char* e = std::getenv(env);
  return e ? std::atoi(e) : def;
}

static long long g_checks = 0;
#define EXPECT(c, ...)                                                              \
  do {                                                                              \
    ++g_checks;                                                                     \
    if (!(c)) {                                                                     \
      std::fprintf(stderr, "FAIL %s:%d: %s  ", __FILE__, __LINE__, #c);             \
      std::fprintf(stderr, __VA_ARGS__);                                            \
      std::fprintf(stderr, "\n");                                                   \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

static const int kCUs = 256;
static const int kLds = 160 * 1024;
static const int kCuCounts[] = {8, 248, 256};   // the schedule tests' count, a reserved count, the chip
static float g_dummy = 0.f;                     // non-null stand-in for a pointer the planners only test
static bf16_t g_dummy16[1];

// one operator call, as the bindings fill their argument structs from it
enum : unsigned { PRO = 1, PRO2 = 2, BIAS = 4, BNB = 8, IMG = 16, DYPRO = 32, DYOUT = 64, BN = 128 };
struct Case {
  const char* op;                 // conv3_fwd | conv3_wgrad | convt_wgrad | convt_bwd_fused
  int N, D, H, W;                 // D = 0: 2-D
  int C1, C2, Cout, co1;          // convT: C1 = Cin
  unsigned flags;
  int groups;
};

static ConvFwdArgs fwd_args(const Case& c) {
  ConvFwdArgs a{};
  a.dims = c.D ? 3 : 2; a.N = c.N; a.D = c.D ? c.D : 1; a.H = c.H; a.W = c.W;
  a.C1 = c.C1; a.C2 = c.C2; a.Cin = c.C1 + c.C2;
  a.CinW = (a.Cin + 7) / 8 * 8;
  a.Cout = c.Cout; a.Co1 = c.co1 > 0 ? c.co1 : c.Cout;
  a.taps = a.dims == 2 ? 9 : 27;
  a.X1 = g_dummy16;
  a.X2 = c.C2 ? g_dummy16 : nullptr;
  if (c.flags & PRO) a.pscale = a.pshift = &g_dummy;
  if (c.flags & PRO2) a.pscale2 = a.pshift2 = &g_dummy;
  if (c.flags & BIAS) a.bias = &g_dummy;
  if (c.flags & BNB) { a.bnb_y = g_dummy16; a.bnb_s4 = &g_dummy; }
  if (c.groups > 1) {
    a.groups = c.groups;
    if (c.flags & PRO) a.gstride = 4LL * c.C1;
    if (c.flags & BNB) a.gstride = 4LL * c.Cout;
  }
  a.npix = (long long)a.N * a.D * a.H * a.W;
  return a;
}

static ConvWgradArgs wgrad_args(const Case& c) {
  ConvWgradArgs a{};
  a.dims = c.D ? 3 : 2; a.N = c.N; a.D = c.D ? c.D : 1; a.H = c.H; a.W = c.W;
  a.C1 = c.C1; a.C2 = c.C2; a.Cin = c.C1 + c.C2; a.Cout = c.Cout;
  a.taps = a.dims == 2 ? 9 : 27;
  a.dY = a.X1 = g_dummy16;
  a.X2 = c.C2 ? g_dummy16 : nullptr;
  if (c.flags & PRO) a.pscale = a.pshift = &g_dummy;
  if (c.flags & PRO2) a.pscale2 = a.pshift2 = &g_dummy;
  if (c.groups > 1 && (c.flags & PRO)) { a.groups = c.groups; a.gimg = c.N / c.groups; a.gstride = 4LL * c.C1; }
  if (c.flags & DYPRO) { a.dyy = g_dummy16; a.dys4 = a.dycoef = &g_dummy; }
  if (c.flags & DYOUT) a.dyout = g_dummy16;
  return a;
}

static GemmArgs convt_args(const Case& c) {
  GemmArgs a{};
  const int dims = c.D ? 3 : 2, D = c.D ? c.D : 1;
  a.mode = GEMM_CONVT_WGRAD;
  a.M = c.C1;
  a.N = (dims == 2 ? 4 : 8) * c.Cout;
  a.K = c.N * D * c.H * c.W;
  a.dims = dims; a.Nimg = c.N; a.D = D; a.H = c.H; a.W = c.W;
  a.Cin = c.C1; a.Cout = c.Cout;
  if (c.flags & BN) a.bn4 = &g_dummy;
  return a;
}

static bool fused_ok(const Case& c, int cus) {
  const int64_t x[4] = {c.N, c.H, c.W, c.C1}, d[4] = {c.N, 2 * c.H, 2 * c.W, c.Cout};
  return !c.D && convt_bwd_fused_ok(x, 4, d, 4, cus);
}

// ------------------------------------------------------------------ invariants per planner
static void check_fwd_plan(const Case& c, int cus) {
  ConvFwdArgs a = fwd_args(c);
  const ConvFwdPlan p = conv3_fwd_plan(a, cus, true);
  if (p.error != nullptr) {
    EXPECT(p.error[0] != 0 && p.path[0] == 0, "rejected plan with a path");
    return;
  }
  EXPECT(p.path[0] != 0, "accepted plan without a path");
  EXPECT(p.grid > 0 && p.stat_rows > 0, "grid=%d rows=%d", p.grid, p.stat_rows);
  if (p.kernel == CONV_FWD_DS) {
    EXPECT(p.stat_rows == p.grid && p.smem > 0 && p.smem <= kLds, "ds rows=%d grid=%d", p.stat_rows, p.grid);
    return;
  }
  EXPECT((long long)a.tilesD * a.TD >= a.D && (long long)a.tilesH * a.TH >= a.H &&
         (long long)a.tilesW * a.TW >= a.W, "tiles do not cover the image (%s)", p.path);
  EXPECT(a.nTilesM == a.N * a.tilesD * a.tilesH * a.tilesW, "nTilesM (%s)", p.path);
  EXPECT(a.ksplit >= 1 && (a.groups <= 1 || a.ksplit == 1), "ksplit=%d groups=%d", a.ksplit, a.groups);
  if (a.groups > 1) EXPECT(p.grid % a.groups == 0, "grid %d not group-major over %d", p.grid, a.groups);
  if (p.kernel == CONV_FWD_RES) {
    EXPECT(p.smem > 0 && p.smem <= kLds && (a.groups > 1 || p.grid <= 2 * cus), "res smem=%d grid=%d", p.smem, p.grid);
    EXPECT(p.stat_rows == p.grid && p.grid % a.nTilesN == 0, "res rows=%d grid=%d", p.stat_rows, p.grid);
    return;
  }
  const int cfg = p.variant;
  EXPECT((a.dims == 3 ? a.TD + 2 : 1) * (a.TH + 2) * (a.TW + 2) <= conv3_fwd_cfg_halo(a.dims, cfg),
         "halo of cfg %d", cfg);
  EXPECT(a.TD * a.TH * a.TW == conv3_fwd_cfg_bm(cfg), "tile of cfg %d", cfg);
  const int nchunks = (a.Cin + 31) / 32;
  if (a.ksplit > 1)
    EXPECT(nchunks % a.ksplit == 0 && nchunks / a.ksplit >= 2, "ksplit=%d of %d chunks", a.ksplit, nchunks);
  EXPECT(p.grid == conv3_fwd_grid(a) && (a.groups > 1 || p.grid <= a.persist_blocks), "stream grid=%d", p.grid);
  EXPECT(p.stat_rows == (a.ksplit > 1 ? p.fin_grid : p.grid), "rows=%d grid=%d fin=%d ks=%d", p.stat_rows,
         p.grid, p.fin_grid, a.ksplit);
  EXPECT(p.fin_grid >= 1 && p.fin_grid <= 2048, "fin_grid=%d", p.fin_grid);
  EXPECT(a.Co1 == a.Cout || a.Co1 % 16 == 0, "split at %d", a.Co1);
}

static void check_wgrad_plan(const Case& c, int cus) {
  ConvWgradArgs a = wgrad_args(c);
  const bool emit = (c.flags & DYOUT) != 0;
  const ConvWgradPlan p = conv3_wgrad_plan(a, cus, (c.flags & IMG) ? 3 : 0, emit);
  if (p.error != nullptr) {
    EXPECT(p.error[0] != 0 && p.path[0] == 0, "rejected plan with a path");
    return;
  }
  EXPECT(p.path[0] != 0, "accepted plan without a path");
  EXPECT(a.splits >= 1, "splits=%d", a.splits);
  const bool own = p.kernel == WGRAD_DS || p.kernel == WGRAD_C32;   // the ds / c32 planner set splits
  if (own) EXPECT(p.grid == a.splits && p.grid >= 1 && p.grid <= cus, "%s grid=%d", p.path, p.grid);
  else EXPECT(a.splits <= std::max(1, a.nTiles / 8), "splits=%d nTiles=%d", a.splits, a.nTiles);
  EXPECT(a.groups <= 1 || p.kernel == WGRAD_V3, "groups on %s", p.path);
  EXPECT(!emit || p.kernel == WGRAD_C32, "dy_out on %s", p.path);
  EXPECT(a.dyy == nullptr || p.kernel == WGRAD_C32 || p.kernel == WGRAD_V2 || p.kernel == WGRAD_IMG,
         "dY prologue on %s", p.path);
  if (p.kernel == WGRAD_V1)
    EXPECT((a.TD + (a.dims == 3 ? 2 : 0)) * (a.TH + 2) * (a.TW + 2) <= conv3_wgrad_halo_cap(a.dims), "v1 halo");
  if (p.kernel == WGRAD_V2 || p.kernel == WGRAD_V3 || p.kernel == WGRAD_IMG)
    EXPECT(a.TD == 1 && a.TW == 16 && a.TH >= 1, "tile %dx%dx%d on %s", a.TD, a.TH, a.TW, p.path);
  if (!own) {
    EXPECT((long long)a.tilesD * a.TD >= a.D && (long long)a.tilesH * a.TH >= a.H &&
           (long long)a.tilesW * a.TW >= a.W, "tiles do not cover the image (%s)", p.path);
    EXPECT(a.coTiles * p.bco >= a.Cout && a.ciChunks * 32 * a.ciw >= a.Cin, "channel tiles (%s)", p.path);
  }
}

// the rows a split of the variant a.wg2 names can span, in bytes (x, dOut)
static void convt_spans(const GemmArgs& a, int splits, long long& x_bytes, long long& dout_bytes) {
  const long long per = ((long long)a.K + splits - 1) / splits + 64;
  const long long span = a.dims == 2 ? 4 * per + 8LL * a.W : 8 * per + 16LL * a.H * a.W;
  x_bytes = per * a.Cin * 2;
  dout_bytes = span * a.Cout * 2;
}

static void check_convt_plan(const Case& c, int cus) {
  const long long lim = 1LL << 31;
  for (int kw = -1; kw <= 1; ++kw) {
    g_wide_knob = kw;
    GemmArgs a = convt_args(c);
    const char* path = convt_wgrad_plan(a, cus);
    EXPECT(path != nullptr && path[0] != 0, "no path");
    EXPECT(a.splits >= 1 && a.wg2 >= 0 && a.wg2 <= 2, "splits=%d wg2=%d", a.splits, a.wg2);
    EXPECT(std::strcmp(path, a.wg2 == 2 ? "convt_wgrad:wg2w" : a.wg2 ? "convt_wgrad:wg2" : "convt_wgrad:wg1") == 0,
           "path %s for wg2=%d", path, a.wg2);
    long long xb, db;
    convt_spans(a, a.splits, xb, db);
    if (a.wg2) EXPECT(db < lim, "dOut span %lld bytes", db);
    if (a.wg2 == 2) EXPECT(xb < lim && convt_wgrad2w_ok(a), "wide: x span %lld bytes", xb);
    if (kw == 0) EXPECT(a.wg2 != 2, "knob 0 chose the wide kernel");
    if (kw == 1) {
      // the wide kernel wherever its constraints hold: one workgroup per CU over its tiles
      GemmArgs w = convt_args(c);
      w.wg2 = 2;
      const int tiles = convt_wgrad2_tiles(w);
      const int ws = std::min(std::max(1, cus / tiles), std::max(1, w.K / 256));
      convt_spans(w, ws, xb, db);
      const bool want = c.C1 % 8 == 0 && c.Cout % 8 == 0 && c.C1 <= 512 && convt_wgrad2w_ok(w) && xb < lim && db < lim;
      EXPECT((a.wg2 == 2) == want, "knob 1: wg2=%d, expected wide=%d", a.wg2, (int)want);
    }
  }
  g_wide_knob = -1;
  if (fused_ok(c, cus)) {
    const long long K = (long long)c.N * c.H * c.W;
    const int s = convt_bwd_fused_splits(K, cus);
    const long long per = (K + s - 1) / s + 64;
    EXPECT(s >= 1 && (4 * per + 8LL * c.W) * 64 * 2 < lim, "fused: splits=%d", s);
    EXPECT(c.C1 == 64 && c.Cout == 64, "fused on %d -> %d channels", c.C1, c.Cout);
  }
}

// ------------------------------------------------------------------ sweeps
static const int kChans[][3] = {  // C1, C2, Cout (U-Net widths, both directions, concat layers)
    {8, 0, 32},    {32, 0, 32},   {32, 0, 64},   {64, 0, 64},   {64, 0, 128},
    {128, 0, 128}, {128, 0, 256}, {256, 0, 256}, {256, 256, 256}, {256, 128, 128},
    {128, 64, 64}, {64, 32, 32},  {32, 0, 8},    {64, 0, 32},   {128, 0, 64},
    {256, 0, 128}, {512, 0, 256}, {384, 0, 128}, {96, 0, 32},   {192, 0, 64},
    {32, 0, 96},   {32, 32, 32},  {16, 0, 64},   {32, 16, 32}};
static const int kSizes2[] = {8, 16, 24, 32, 40, 64, 72, 128, 200, 256, 512, 1024};
static const int kSizes3[] = {8, 12, 16, 24, 32, 64, 72, 128};
static const int kBatches[] = {1, 2, 8, 32, 128, 256};

template <typename F>
static void for_geometries(F&& f) {
  for (int dims = 2; dims <= 3; ++dims)
    for (int n : kBatches) {
      if (dims == 2) for (int hw : kSizes2) f(n, 0, hw, hw);
      else for (int s : kSizes3) { f(n, s, s, s); if (s >= 16) f(n, s / 4, s, s / 2); }
    }
}

static void sweep_conv_fwd() {
  for (auto& ch : kChans)
    for (int hw : kSizes2)
      for (int n : kBatches)
        for (int pro = 0; pro < 2; ++pro) {
          ConvFwdArgs a = fwd_args({"conv3_fwd", n, 0, hw, hw, ch[0], ch[1], ch[2], 0, pro ? PRO : 0u, 0});
          int grid = 0, smem = 0;
          const int v = conv3_res_plan(a, kCUs, grid, smem);
          if (v < 0) continue;
          EXPECT(grid > 0 && grid <= 2 * kCUs, "grid=%d C=%d/%d/%d hw=%d n=%d", grid, ch[0], ch[1], ch[2], hw, n);
          EXPECT(smem > 0 && smem <= kLds, "smem=%d", smem);
          EXPECT(grid % a.nTilesN == 0, "grid %d not a multiple of nTilesN %d", grid, a.nTilesN);
          EXPECT((long long)a.tilesH * a.TH >= a.H && (long long)a.tilesW * a.TW >= a.W,
                 "tiles do not cover the image");
          EXPECT(a.nTilesM == a.N * a.tilesH * a.tilesW, "nTilesM");
        }
  for (int cfg = 0; cfg <= 9; ++cfg) {
    EXPECT(conv3_fwd_cfg_bm(cfg) > 0 && conv3_fwd_cfg_bn(cfg) > 0, "cfg %d", cfg);
    EXPECT(conv3_fwd_cfg_halo(cfg <= 5 ? 2 : 3, cfg) > 0, "halo cfg %d", cfg);
  }
  // the whole plan: prologue / bias / BN-backward epilogue / split outputs / BN groups
  const unsigned modes[] = {0u, PRO | BIAS, BNB};
  for (int cus : kCuCounts)
    for (auto& ch : kChans)
      for_geometries([&](int n, int d, int h, int w) {
        for (unsigned m : modes)
          for (int groups : {1, 2, 4}) {
            if (n % groups != 0 || ((m & BNB) && d)) continue;
            const unsigned pro2 = (ch[1] && (m & PRO) && groups == 1) ? PRO2 : 0u;
            check_fwd_plan({"conv3_fwd", n, d, h, w, ch[0], ch[1], ch[2], 0, m | pro2, groups}, cus);
            if (!(m & BNB) && ch[2] >= 32)   // split outputs: on a 16-channel boundary, and off one
              for (int co1 : {ch[2] / 2, 8})
                check_fwd_plan({"conv3_fwd", n, d, h, w, ch[0], ch[1], ch[2], co1, m | pro2, groups}, cus);
          }
      });
}

static void sweep_wgrad() {
  const int c2s[] = {0, 32, 64, 128, 256};
  const int sizes[] = {16, 24, 32, 64, 128, 256, 512, 1024};
  for (int bco : {32, 64})
    for (int c2 : c2s)
      for (int hw : sizes) {
        const int pt = conv3_wgrad2_pt(bco, c2, hw, hw);
        EXPECT(pt == 64 || pt == 96 || pt == 128 || pt == 256, "pt=%d", pt);
        EXPECT(pt % 16 == 0, "pixel tile must be whole 16-wide rows");
      }
  EXPECT(conv3_wgrad_halo_cap(2) > 0 && conv3_wgrad_halo_cap(3) > 0, "halo caps");
  const unsigned modes[] = {0u, PRO, DYPRO, DYPRO | DYOUT, IMG, IMG | DYPRO};
  for (int cus : kCuCounts)
    for (auto& ch : kChans)
      for_geometries([&](int n, int d, int h, int w) {
        for (unsigned m : modes)
          for (int groups : {1, 2, 4}) {
            if (n % groups != 0 || (groups > 1 && (!(m & PRO) || ch[1]))) continue;
            const unsigned pro2 = (ch[1] && (m & PRO)) ? PRO2 : 0u;
            check_wgrad_plan({"conv3_wgrad", n, d, h, w, ch[0], ch[1], ch[2], 0, m | pro2, groups}, cus);
          }
      });
}

static void sweep_convt() {
  const int chans[][2] = {{512, 256}, {256, 128}, {128, 64}, {64, 32}, {256, 256}, {128, 128},
                          {64, 64},   {1024, 64}, {40, 24},  {96, 64}};
  for (int cus : kCuCounts)
    for (auto& ch : chans)
      for (unsigned bn : {0u, (unsigned)BN})
        for (int n : kBatches) {
          for (int hw : {4, 8, 16, 32, 64, 128, 256, 512}) check_convt_plan({"convt_wgrad", n, 0, hw, hw, ch[0], 0, ch[1], 0, bn, 0}, cus);
          for (int s : {4, 8, 16, 32, 64}) check_convt_plan({"convt_wgrad", n, s, s, s, ch[0], 0, ch[1], 0, bn, 0}, cus);
        }
  // shapes the fused backward must refuse
  const int64_t x[4] = {2, 6, 10, 64}, d_ok[4] = {2, 12, 20, 64}, d_bad[4] = {2, 12, 10, 64}, x128[4] = {2, 6, 10, 128};
  EXPECT(convt_bwd_fused_ok(x, 4, d_ok, 4, 8), "fused: the exact tests' shape");
  EXPECT(!convt_bwd_fused_ok(x, 4, d_bad, 4, 8) && !convt_bwd_fused_ok(x128, 4, d_ok, 4, 8) &&
         !convt_bwd_fused_ok(x, 3, d_ok, 4, 8), "fused: mismatched shapes");
}

static void sweep_reductions() {
  for (long long items = 1; items < (1LL << 34); items = items * 3 + 1) {
    const int nb = bn_bwd_reduce_blocks(items);
    EXPECT(nb >= 1 && nb <= 2048, "nb=%d items=%lld", nb, items);
  }
  for (int r = 1; r < (1 << 20); r = r * 2 + 1) {
    const int ch = reduce_rows_chunks(r);
    EXPECT(ch >= 1 && ch <= r, "chunks=%d rows=%d", ch, r);
    const long long t = reduce_rows_scatter_tmp(r, 7);
    EXPECT(t == 0 || t == 7LL * ch, "scatter scratch %lld for %d rows", t, r);
    EXPECT(r <= 1024 || t > 0, "two-pass scatter of %d rows without scratch", r);
  }
  EXPECT(head_supported(32, 6), "flagship head (32 -> 6 classes)");
  EXPECT(!head_supported(7, 6), "head rejects C %% 8 != 0");
}

// ------------------------------------------------------------------ data_math.h
// the mirror by walking |i| steps between the two edges (i is first reduced by whole periods)
static long long walk_mirror(long long i, long long n) {
  if (n == 1) return 0;
  long long steps = (i < 0 ? -i : i) % (2 * (n - 1)), pos = 0, dir = 1;
  for (; steps > 0; --steps) {
    if (pos + dir < 0 || pos + dir >= n) dir = -dir;
    pos += dir;
  }
  return pos;
}

template <typename I>
static void check_reflect(I i, I n) {
  const I r = reflect_index(i, n);
  EXPECT(r == (I)walk_mirror(i, n) && reflect_fast(i, n) == r, "reflect(%lld, %lld) = %lld", (long long)i,
         (long long)n, (long long)r);
}

// the largest scene side, 2^30 - 1: an index of at most one period folds at most once
static void check_big_reflect(int i) {
  const long long n = (1 << 30) - 1, m = i < 0 ? -(long long)i : i;
  EXPECT(m < 2 * (n - 1) && reflect_fast(i, (int)n) == (m < n ? m : 2 * (n - 1) - m), "reflect(%d, 2^30 - 1)", i);
}

static void sweep_data_math() {
  for (int n = 1; n <= 9; ++n) {
    for (int i = -40; i <= 40; ++i) { check_reflect<int>(i, n); check_reflect<int64_t>(i, n); }
    for (int d = -3; d <= 3; ++d)
      for (int sign : {-1, 1}) {
        check_reflect<int>(sign * ((1 << 30) + d), n);
        check_reflect<int64_t>(sign * ((1LL << 30) + d), n);
        check_big_reflect(sign * ((1 << 30) + d));
      }
  }
  for (int code = 0; code < 8; ++code)
    for (int tile : {1, 2, 33})
      for (int oy = 0; oy < tile; ++oy)
        for (int ox = 0; ox < tile; ++ox) {
          const Index2<int> f = d4_forward(code, tile, oy, ox);
          const Index2<int> g = d4_inverse(code, tile, f.a, f.b);
          EXPECT(f.a >= 0 && f.a < tile && f.b >= 0 && f.b < tile && g.a == oy && g.b == ox,
                 "d4 code %d tile %d (%d, %d) -> (%d, %d) -> (%d, %d)", code, tile, oy, ox, f.a, f.b, g.a, g.b);
          const Index2<int64_t> f64 = d4_forward<int64_t>(code, tile, oy, ox);
          EXPECT(f64.a == f.a && f64.b == f.b, "d4 int64 code %d", code);
        }
  // pick_scene at every boundary of the cumulative table: the draw r0 with (r0 * total) >> 32 == t
  const int64_t cum[] = {0, 1, 2, 7, 12, 1000, 1LL << 31, (1LL << 32) - 1};
  const int n = (int)(sizeof(cum) / sizeof(cum[0])) - 1;
  for (int k = 0; k <= n; ++k)
    for (int64_t t : {cum[k], cum[k] - 1}) {
      if (t < 0 || t >= cum[n]) continue;
      const uint32_t r0 = (uint32_t)((((unsigned __int128)t << 32) + cum[n] - 1) / cum[n]);
      EXPECT((int64_t)scale_draw(r0, (uint64_t)cum[n]) == t, "draw for t=%lld", (long long)t);
      const int lo = pick_scene(cum, n, r0);
      EXPECT(lo >= 0 && lo < n && cum[lo] <= t && t < cum[lo + 1], "pick_scene t=%lld -> %d", (long long)t, lo);
    }
  EXPECT(pick_scene(cum, n, 0u) == 0 && pick_scene(cum, n, 0xffffffffu) == n - 1, "pick_scene ends");
  // the crop origin draw and the footprint centre on the largest scene
  const long long big = (1LL << 30) - 1;
  for (long long span : {1LL, 32768LL, big, big + 5})
    for (uint32_t r : {0u, 1u, 0x80000000u, 0xffffffffu}) {
      const uint64_t cnt = origin_count(big, span), o = scale_draw(r, cnt);
      EXPECT(cnt == (uint64_t)(big > span ? big - span : 0) + 1 && o < cnt,
             "origin draw r=%u span=%lld -> %llu of %llu", r, span, (unsigned long long)o, (unsigned long long)cnt);
      const long long c = footprint_centre(r, big, span);
      EXPECT(c == (2 * (long long)o + span - 1) * 32768 && c > -kCentre && c < kCentre, "centre %lld", c);
    }
  EXPECT(footprint(32768, INT_MAX) == (1LL << 30) && footprint(1, 65536) == 1, "footprint");
  EXPECT(matrix_entry(INT_MAX, 65536) == INT_MAX && matrix_entry(INT_MAX, -65536) == -(long long)INT_MAX,
         "matrix entry");
  (void)footprint_centre(0xffffffffu, -1, LLONG_MAX);      // wild table entries wrap, unsigned
  (void)footprint_centre(0xffffffffu, LLONG_MIN, 1);
  // the warp coordinate at the extremes warp_row_valid admits: far inside int64, taps inside int
  const int tile = 32768;
  EXPECT(warp_row_valid(kCoef, -kCoef, kCentre - 1, 1 - kCentre) && !warp_row_valid(kCoef + 1, 0, 0, 0) &&
         !warp_row_valid(0, -kCoef - 1, 0, 0) && !warp_row_valid(0, 0, kCentre, 0) && !warp_row_valid(0, 0, 0, -kCentre),
         "warp_row_valid bounds");
  for (long long cy : {kCentre - 1, 1 - kCentre})
    for (long long cx : {kCentre - 1, 1 - kCentre})
      for (int A : {(int)kCoef, -(int)kCoef})
        for (int Bm : {(int)kCoef, -(int)kCoef})
          for (int a : {0, tile - 1})
            for (int b : {0, tile - 1}) {
              const Index2<long long> p = warp_coord(cy, cx, A, Bm, tile, a, b);
              for (long long q : {p.a, p.b}) {
                EXPECT(q > -(kCentre + (1LL << 36)) && q < kCentre + (1LL << 36), "warp coordinate %lld", q);
                EXPECT((q >> 16) >= INT_MIN && (q >> 16) + 1 <= INT_MAX && warp_tap(q) == (q >> 16) &&
                       warp_nearest(q) == ((q + 32768) >> 16), "tap of %lld", q);
                const float w = warp_weight(q);
                EXPECT(w >= 0.f && w < 1.f && (long long)(w * 65536.0f) == (q & 65535), "weight of %lld", q);
                check_big_reflect(warp_tap(q));
                check_big_reflect(warp_tap(q) + 1);
              }
            }
}

// ------------------------------------------------------------------ the plan table
// Part 1: every conv3_fwd / conv3_wgrad / convt_wgrad / convt_bwd_fused shape of CASES_8 and
// CASES_0 in tests/test_kernels_exact_gpu.py (its "dgrad" cases in conv3_fwd's own terms: the
// gradient's channels in, the forward conv's input channels out), printed at 256 and at 8 CUs.
static const Case kExactCases[] = {
    // conv3_fwd forward, resident-weight kernel
    {"conv3_fwd", 2, 0, 50, 40, 32, 0, 32, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 0, 50, 40, 8, 0, 32, 0, BIAS | IMG, 0},
    {"conv3_fwd", 2, 0, 50, 40, 64, 32, 32, 0, PRO | PRO2 | BIAS, 0},
    {"conv3_fwd", 2, 0, 40, 24, 32, 0, 64, 0, PRO | BIAS, 0},
    {"conv3_fwd", 3, 0, 20, 18, 64, 0, 64, 0, BIAS, 0},
    {"conv3_fwd", 4, 0, 20, 18, 32, 0, 64, 0, PRO, 2},
    {"conv3_fwd", 2, 3, 20, 40, 8, 0, 32, 0, BIAS | IMG, 0},
    // streaming kernel, 2-D
    {"conv3_fwd", 2, 0, 20, 18, 32, 0, 32, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 0, 12, 40, 64, 0, 64, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 0, 23, 40, 128, 0, 128, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 0, 12, 20, 128, 0, 128, 0, BIAS, 0},
    {"conv3_fwd", 2, 0, 8, 8, 256, 0, 256, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 0, 30, 30, 128, 0, 128, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 0, 30, 30, 128, 32, 128, 0, BIAS, 0},
    {"conv3_fwd", 2, 0, 62, 32, 128, 0, 128, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 0, 62, 32, 128, 64, 256, 128, 0, 0},
    // conv3_fwd as the data gradient
    {"conv3_fwd", 2, 0, 40, 24, 32, 0, 96, 64, 0, 0},
    {"conv3_fwd", 2, 0, 50, 40, 32, 0, 48, 16, 0, 0},
    {"conv3_fwd", 2, 0, 50, 40, 32, 0, 160, 128, 0, 0},
    {"conv3_fwd", 2, 0, 40, 24, 32, 0, 128, 64, 0, 0},
    {"conv3_fwd", 2, 0, 50, 40, 32, 0, 32, 0, BNB, 0},
    {"conv3_fwd", 2, 0, 40, 24, 64, 0, 64, 0, BNB, 0},
    {"conv3_fwd", 4, 0, 20, 18, 64, 0, 64, 0, BNB, 2},
    {"conv3_fwd", 2, 0, 20, 18, 32, 0, 32, 0, BNB, 0},
    {"conv3_fwd", 2, 0, 12, 40, 64, 0, 64, 0, BNB, 0},
    {"conv3_fwd", 2, 0, 8, 8, 256, 0, 256, 0, BNB, 0},
    {"conv3_fwd", 2, 0, 30, 30, 128, 0, 128, 0, BNB, 0},
    {"conv3_fwd", 2, 0, 23, 40, 128, 0, 128, 0, BNB, 0},
    {"conv3_fwd", 2, 0, 12, 20, 128, 0, 128, 0, BNB, 0},
    {"conv3_fwd", 2, 0, 12, 40, 32, 0, 64, 32, 0, 0},
    // 3-D forward
    {"conv3_fwd", 2, 5, 20, 18, 32, 0, 64, 32, PRO, 0},
    {"conv3_fwd", 2, 3, 20, 18, 32, 0, 32, 0, BIAS, 0},
    {"conv3_fwd", 2, 5, 8, 8, 64, 0, 32, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 5, 8, 8, 64, 0, 64, 0, BIAS, 0},
    {"conv3_fwd", 2, 7, 16, 8, 64, 0, 128, 0, BIAS, 0},
    {"conv3_fwd", 2, 5, 8, 8, 64, 0, 128, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 11, 8, 16, 64, 0, 32, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 7, 8, 16, 64, 0, 64, 0, BIAS, 0},
    {"conv3_fwd", 2, 7, 4, 16, 64, 0, 128, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 7, 8, 16, 64, 0, 96, 64, 0, 0},
    // CASES_0 (split-K at the whole chip)
    {"conv3_fwd", 2, 0, 20, 18, 128, 0, 32, 0, PRO | BIAS, 0},
    {"conv3_fwd", 2, 0, 20, 18, 128, 0, 64, 0, BIAS, 0},
    {"conv3_fwd", 2, 0, 20, 18, 128, 0, 64, 0, BNB, 0},
    {"conv3_fwd", 2, 5, 8, 8, 128, 0, 32, 0, BIAS, 0},
    {"conv3_fwd", 2, 5, 8, 8, 128, 0, 64, 0, BIAS, 0},
    {"conv3_fwd", 2, 5, 8, 8, 128, 0, 128, 0, BIAS, 0},
    // conv3_wgrad
    {"conv3_wgrad", 2, 0, 10, 6, 32, 0, 32, 0, PRO, 0},
    {"conv3_wgrad", 2, 0, 20, 18, 16, 0, 64, 0, PRO, 0},
    {"conv3_wgrad", 2, 0, 20, 18, 32, 16, 32, 0, PRO | PRO2, 0},
    {"conv3_wgrad", 2, 0, 20, 18, 8, 0, 32, 0, DYPRO, 0},
    {"conv3_wgrad", 2, 0, 20, 18, 8, 0, 32, 0, IMG, 0},
    {"conv3_wgrad", 3, 0, 40, 24, 8, 0, 64, 0, IMG, 0},
    {"conv3_wgrad", 2, 0, 20, 18, 8, 0, 32, 0, IMG | DYPRO, 0},
    {"conv3_wgrad", 2, 0, 20, 18, 32, 0, 32, 0, PRO, 0},
    {"conv3_wgrad", 4, 0, 20, 18, 32, 0, 32, 0, PRO, 2},
    {"conv3_wgrad", 2, 0, 20, 18, 64, 32, 64, 0, PRO | PRO2, 0},
    {"conv3_wgrad", 2, 0, 72, 58, 64, 0, 64, 0, PRO, 0},
    {"conv3_wgrad", 2, 0, 36, 30, 32, 0, 128, 0, PRO, 0},
    {"conv3_wgrad", 2, 0, 72, 100, 64, 32, 32, 0, PRO | PRO2, 0},
    {"conv3_wgrad", 2, 0, 72, 100, 32, 32, 32, 0, 0, 0},
    {"conv3_wgrad", 2, 0, 72, 100, 64, 32, 32, 0, DYPRO | DYOUT, 0},
    {"conv3_wgrad", 2, 5, 72, 58, 32, 0, 32, 0, PRO, 0},
    {"conv3_wgrad", 2, 5, 20, 18, 8, 0, 32, 0, IMG, 0},
    {"conv3_wgrad", 2, 5, 12, 20, 32, 0, 64, 0, PRO, 0},
    {"conv3_wgrad", 2, 5, 12, 20, 32, 0, 32, 0, 0, 0},
    {"conv3_wgrad", 2, 3, 36, 30, 32, 0, 128, 0, 0, 0},
    {"conv3_wgrad", 2, 3, 12, 20, 16, 0, 32, 0, 0, 0},
    {"conv3_wgrad", 2, 3, 10, 6, 32, 0, 32, 0, 0, 0},
    // transposed-conv weight gradient and fused backward
    {"convt_wgrad", 2, 0, 12, 20, 64, 0, 64, 0, BN, 0},
    {"convt_wgrad", 3, 0, 6, 10, 128, 0, 64, 0, 0, 0},
    {"convt_wgrad", 2, 0, 6, 10, 1024, 0, 64, 0, 0, 0},
    {"convt_wgrad", 2, 2, 6, 10, 64, 0, 64, 0, 0, 0},
    {"convt_bwd_fused", 3, 0, 12, 20, 64, 0, 64, 0, BN, 0},
    {"convt_bwd_fused", 2, 0, 6, 10, 64, 0, 64, 0, 0, 0},
    {"convt_bwd_fused", 2, 0, 6, 10, 64, 0, 64, 0, BN, 0},
    {"convt_bwd_fused", 2, 0, 6, 10, 128, 0, 64, 0, BN, 0},
};

// Part 2: rows at 8 CUs that take each chip-filling decision both ways (the comparison in
// the comment, its two sides on neighbouring lines)
static const Case kFillCases[] = {
    // conv3_fwd 128 -> 128: 256-pixel tiles (cfg 4) need >= 8 items; else 64-pixel tiles, split-K
    {"conv3_fwd", 1, 0, 16, 16, 128, 0, 128, 0, 0, 0},
    {"conv3_fwd", 2, 0, 32, 32, 128, 0, 128, 0, 0, 0},
    // 512-pixel tiles (cfg 5): >= 8 items without padding; 40 rows pad a 512-pixel tile by 60%
    {"conv3_fwd", 4, 0, 32, 32, 128, 0, 128, 0, 0, 0},
    {"conv3_fwd", 4, 0, 40, 32, 128, 0, 128, 0, 0, 0},
    // 128-pixel tiles (cfg 2) need >= 16 items (else cfg 3); tiles far larger than the image
    // fall back along cfg 4 -> 2 -> 3 (8 x 8 images)
    {"conv3_fwd", 1, 0, 24, 40, 128, 0, 128, 0, 0, 0},
    {"conv3_fwd", 2, 0, 24, 40, 128, 0, 128, 0, 0, 0},
    {"conv3_fwd", 8, 0, 8, 8, 128, 0, 128, 0, 0, 0},
    // split-K only while items * ks <= 16: four chunk groups, then two
    {"conv3_fwd", 1, 0, 8, 8, 256, 0, 128, 0, 0, 0},
    {"conv3_fwd", 6, 0, 8, 8, 256, 0, 128, 0, 0, 0},
    // resident kernel: >= 8 32x16 tiles (32 -> 32 channels), else streaming
    {"conv3_fwd", 1, 0, 32, 32, 32, 0, 32, 0, PRO, 0},
    {"conv3_fwd", 4, 0, 32, 32, 32, 0, 32, 0, PRO, 0},
    // 3-D 32 -> 32: the depth-streaming kernel needs >= 8 (chunk, column) items
    {"conv3_fwd", 1, 4, 32, 32, 32, 0, 32, 0, 0, 0},
    {"conv3_fwd", 2, 4, 32, 32, 32, 0, 32, 0, 0, 0},
    // 3-D 64 -> 64: the 8-wave tiles (cfg 7) need >= 8 items and <= 15% padding
    {"conv3_fwd", 1, 4, 16, 16, 64, 0, 64, 0, 0, 0},
    {"conv3_fwd", 1, 8, 16, 16, 64, 0, 64, 0, 0, 0},
    {"conv3_fwd", 2, 5, 16, 16, 64, 0, 64, 0, 0, 0},
    // conv3_wgrad: 128 output channels per workgroup from 32 x 32 images up
    {"conv3_wgrad", 2, 0, 16, 16, 128, 0, 128, 0, 0, 0},
    {"conv3_wgrad", 2, 0, 32, 32, 128, 0, 128, 0, 0, 0},
    // two input chunks per workgroup from 64 x 64 images up
    {"conv3_wgrad", 2, 0, 32, 32, 64, 0, 64, 0, 0, 0},
    {"conv3_wgrad", 2, 0, 64, 64, 64, 0, 64, 0, 0, 0},
    // the 32-output-channel concat kernel needs >= 64 16x16 tiles
    {"conv3_wgrad", 1, 0, 64, 64, 64, 32, 32, 0, 0, 0},
    {"conv3_wgrad", 1, 0, 128, 128, 64, 32, 32, 0, 0, 0},
    // 3-D depth-streaming weight gradient: >= 64 x 64 planes
    {"conv3_wgrad", 1, 4, 32, 32, 32, 0, 32, 0, 0, 0},
    {"conv3_wgrad", 1, 4, 64, 64, 32, 0, 32, 0, 0, 0},
    // convT weight gradient: the 256-column tiles from 16384 pixels with the deferred BN
    {"convt_wgrad", 8, 0, 32, 32, 256, 0, 256, 0, BN, 0},
    {"convt_wgrad", 16, 0, 32, 32, 256, 0, 256, 0, BN, 0},
    {"convt_wgrad", 16, 0, 32, 32, 256, 0, 256, 0, 0, 0},
    {"convt_bwd_fused", 2, 0, 32, 32, 64, 0, 64, 0, BN, 0},
};

// ------------------------------------------------------------------ bn_math.h
static void check_perm(int mode, int A, int T, int B) {
  const long long N = (long long)A * T * B;
  std::vector<char> hit((size_t)N, 0);
  for (long long j = 0; j < N; ++j) {
    const long long d = slab_perm(mode, j, T, B);
    EXPECT(d >= 0 && d < N && !hit[(size_t)d], "slab_perm(%d, %lld, %d, %d) = %lld", mode, j, T, B, d);
    hit[(size_t)d] = 1;
    // the element (a, t, b) of the slab is the element (a, b, t) of the parameter
    EXPECT(d == ((j / ((long long)B * T)) * B + j % B) * T + (j / B) % T, "slab_perm layout");
  }
  EXPECT(slab_perm(2, N - 1, T, B) == N - 1, "mode 2 is the identity");
}

static void sweep_bn_math() {
  for (auto& ch : kChans)                                   // conv: (Cout, taps, Cin), 2-D and 3-D
    for (int taps : {9, 27}) check_perm(0, ch[2], taps, ch[0] + ch[1]);
  for (auto& ch : {std::pair<int, int>{512, 256}, {256, 128}, {128, 64}, {64, 32}, {40, 24}})
    for (int subs : {4, 8}) check_perm(1, ch.first, subs, ch.second);   // convT: (Cin, subs, Cout)
  check_perm(0, 3, 1, 5);
  check_perm(1, 1, 7, 1);

  const float eps = 1e-5f, inv0 = (float)(1.0 / std::sqrt((double)eps));
  // one pixel: var = 0, the running variance keeps the biased one (no division by count - 1 = 0)
  BnStats4 s = bn_stats4(3.0, 9.0, 1.0, 2.f, 0.5f, eps);
  EXPECT(s.mean == 3.f && s.var == 0.0 && s.invstd == inv0 && bn_unbiased_var(s.var, 1.0) == 0.f, "stats4, count = 1");
  // a raw variance below zero (s2 / count < mean^2) clamps to 0
  s = bn_stats4(7.0, 4.0, 10.0, 1.f, 0.f, eps);
  EXPECT(s.var == 0.0 && s.invstd == inv0 && s.scale == inv0 && s.shift == fmaf(-0.7f, inv0, 0.f), "stats4, clamp");
  // a constant channel y = 3: var = 0 exactly, shift = beta - 3 scale in one rounding
  s = bn_stats4(3.0 * 441, 9.0 * 441, 441.0, -1.f, 0.25f, eps);
  EXPECT(s.mean == 3.f && s.var == 0.0 && s.scale == -inv0 && s.shift == fmaf(-3.f, -inv0, 0.25f), "stats4, constant");
  EXPECT(bn_unbiased_var(2.0, 5.0) == 2.5f, "unbiased variance");
  EXPECT(bn_momentum_update(7.f, 3.f, 1.f) == 3.f && bn_momentum_update(4.f, 8.f, 0.25f) == 5.f, "momentum update");

  // the three summation orders at the regime borders, on rows whose fp64 sum depends on the order
  for (long long R : {1LL, (long long)kSlabChunkRows, kSlabChunkRows + 1LL, (long long)kWideMaxRows, kWideMaxRows + 1LL}) {
    const long long ld = 3;
    std::vector<float> in((size_t)(R * ld));
    for (long long r = 0; r < R; ++r)
      for (long long j = 0; j < ld; ++j) in[(size_t)(r * ld + j)] = (r % 3 == 0 ? 1e30f : r % 3 == 1 ? -1e30f : 1.f) * (float)(j + 1);
    for (long long j = 0; j < ld; ++j) {
      double want = 0.0;
      if (R <= kSlabChunkRows) {
        for (long long r = 0; r < R; ++r) want += (double)in[(size_t)(r * ld + j)];
      } else if (R <= kWideMaxRows) {
        double w[kWideWaves] = {};
        for (long long r = 0; r < R; ++r) w[r % kWideWaves] += (double)in[(size_t)(r * ld + j)];
        for (double v : w) want += v;
      } else {
        std::vector<double> chunk((size_t)((R + kSlabChunkRows - 1) / kSlabChunkRows), 0.0);
        for (long long r = 0; r < R; ++r) chunk[(size_t)(r / kSlabChunkRows)] += (double)in[(size_t)(r * ld + j)];
        for (double v : chunk) want += v;
      }
      EXPECT(slab_column_sum(in.data(), R, ld, j) == want, "slab_column_sum R=%lld j=%lld", R, j);
    }
    EXPECT((R > kWideMaxRows) == (reduce_rows_scatter_tmp((int)R, 7) > 0), "scratch only above the wide form, R=%lld", R);
  }
}

static void print_row(const Case& c, int cus) {
  char shape[160];
  int n = std::snprintf(shape, sizeof(shape), "N=%d", c.N);
  auto add = [&](const char* k, int v) { if (v) n += std::snprintf(shape + n, sizeof(shape) - n, " %s=%d", k, v); };
  const bool convt = std::strncmp(c.op, "convt", 5) == 0;
  add("D", c.D); add("H", c.H); add("W", c.W);
  add(convt ? "Cin" : "C1", c.C1); add("C2", c.C2); add("Cout", c.Cout); add("co1", c.co1);
  add("pro", c.flags & PRO ? 1 : 0); add("pro2", c.flags & PRO2 ? 1 : 0); add("bias", c.flags & BIAS ? 1 : 0);
  add("bnb", c.flags & BNB ? 1 : 0); add("img", c.flags & IMG ? 1 : 0); add("dypro", c.flags & DYPRO ? 1 : 0);
  add("dyout", c.flags & DYOUT ? 1 : 0); add("bn", c.flags & BN ? 1 : 0); add("groups", c.groups);
  std::printf("%s | %s | %d | ", c.op, shape, cus);
  if (std::strcmp(c.op, "conv3_fwd") == 0) {
    ConvFwdArgs a = fwd_args(c);
    const ConvFwdPlan p = conv3_fwd_plan(a, cus, true);
    if (p.error) { std::printf("error: %s | - | - | -\n", p.error); return; }
    std::printf("%s | grid=%d rows=%d | ks=%d | ", p.path, p.grid, p.stat_rows, p.kernel == CONV_FWD_DS ? 1 : a.ksplit);
    if (p.kernel == CONV_FWD_DS) std::printf("-\n");
    else std::printf("%dx%dx%d\n", a.TD, a.TH, a.TW);
  } else if (std::strcmp(c.op, "conv3_wgrad") == 0) {
    ConvWgradArgs a = wgrad_args(c);
    const ConvWgradPlan p = conv3_wgrad_plan(a, cus, (c.flags & IMG) ? 3 : 0, (c.flags & DYOUT) != 0);
    if (p.error) { std::printf("error: %s | - | - | -\n", p.error); return; }
    const bool own = p.kernel == WGRAD_DS || p.kernel == WGRAD_C32;
    const int grid = own ? p.grid : a.coTiles * (p.kernel == WGRAD_IMG ? 1 : a.ciChunks) * a.planes * a.splits;
    std::printf("%s | grid=%d | splits=%d | ", p.path, grid, a.splits);
    if (own) std::printf("16x16\n");
    else std::printf("%dx%dx%d\n", a.TD, a.TH, a.TW);
  } else if (std::strcmp(c.op, "convt_wgrad") == 0) {
    GemmArgs a = convt_args(c);
    const char* path = convt_wgrad_plan(a, cus);
    const int tiles = a.wg2 ? convt_wgrad2_tiles(a) : ((a.M + 63) / 64) * ((a.N + 63) / 64);
    std::printf("%s | grid=%d | splits=%d | -\n", path, tiles * a.splits, a.splits);
  } else {
    if (fused_ok(c, cus)) {
      const int s = convt_bwd_fused_splits((long long)c.N * c.H * c.W, cus);
      std::printf("convt_bwd_fused:fused | grid=%d rows=%d | splits=%d | -\n", s, (c.flags & BN) ? s : 0, s);
    } else {
      std::printf("convt_bwd_fused:separate | - | - | -\n");
    }
  }
}

static void print_table() {
  std::printf("# op | shape | num_cus | path | grid | splits/ksplit | tile   (tools/host_sanitize.cpp --table)\n");
  for (int cus : {256, 8})
    for (const Case& c : kExactCases) print_row(c, cus);
  for (const Case& c : kFillCases) print_row(c, 8);
  // the same shape on the whole chip: too few items for one depth-streaming workgroup per two CUs
  print_row({"conv3_wgrad", 1, 4, 64, 64, 32, 0, 32, 0, 0, 0}, 256);
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--table") == 0) {
    g_knob_defaults = true;
    print_table();
    return 0;
  }
  sweep_conv_fwd();
  sweep_wgrad();
  sweep_convt();
  sweep_reductions();
  sweep_data_math();
  sweep_bn_math();
  std::printf("host_sanitize: %lld planner checks passed (ASan + UBSan)\n", g_checks);
  return 0;
}
