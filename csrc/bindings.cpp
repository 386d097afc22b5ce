// PyTorch operator registration for the gfx950 kernel library: TORCH_LIBRARY(ddlpc, ...)
// declares every operator as torch.ops.ddlpc.<name>; TORCH_LIBRARY_IMPL(ddlpc, CUDA) below
// registers the HIP kernels, and csrc/cpu_ref.cpp registers the C++ reference kernels under
// the CPU key (the dispatcher picks by tensor device).
//
// Tensor conventions: activations are channel-last tensors whose SHAPE is [N, (D,) H, W, C]
// (contiguous), bf16.  Parameters are fp32 in standard PyTorch layouts; packed bf16 weight
// copies are produced by weight_pack.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "data_checks.h"
#include "tail_checks.h"
#include "ops.h"
#include "optim_math.h"

namespace ddlpc {

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

#define CHECK_DEV(t) TORCH_CHECK((t).is_cuda(), #t " must be a GPU tensor")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHECK_BF16(t) TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16")
#define CHECK_F32(t) TORCH_CHECK((t).scalar_type() == at::kFloat, #t " must be fp32")

const bf16_t* bptr(const at::Tensor& t) { return reinterpret_cast<const bf16_t*>(t.data_ptr()); }
bf16_t* bptr_mut(at::Tensor& t) { return reinterpret_cast<bf16_t*>(t.data_ptr()); }
bool has(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }
const float* fptr_opt(const c10::optional<at::Tensor>& t) {
  return has(t) ? t->data_ptr<float>() : nullptr;
}

struct Geo {
  int dims, N, D, H, W, C;
};
Geo geo_of(const at::Tensor& x) {
  TORCH_CHECK(x.dim() == 4 || x.dim() == 5, "expected [N,(D,)H,W,C] channel-last tensor");
  Geo g;
  g.dims = (int)x.dim() - 2;
  g.N = (int)x.size(0);
  g.D = g.dims == 3 ? (int)x.size(1) : 1;
  g.H = (int)x.size(g.dims == 3 ? 2 : 1);
  g.W = (int)x.size(g.dims == 3 ? 3 : 2);
  g.C = (int)x.size(-1);
  return g;
}
std::vector<int64_t> shape_with_c(const Geo& g, int C, int scale = 1) {
  if (g.dims == 2) return {g.N, (int64_t)g.H * scale, (int64_t)g.W * scale, C};
  return {g.N, (int64_t)g.D * scale, (int64_t)g.H * scale, (int64_t)g.W * scale, C};
}

// shape of the 2x max-pooled tensor
std::vector<int64_t> pooled_shape(const Geo& g) {
  TORCH_CHECK(g.H % 2 == 0 && g.W % 2 == 0 && (g.dims == 2 || g.D % 2 == 0), "pool needs even dims");
  if (g.dims == 2) return {g.N, g.H / 2, g.W / 2, g.C};
  return {g.N, g.D / 2, g.H / 2, g.W / 2, g.C};
}

}  // namespace

// ---- what the last conv / convT / head / BatchNorm operator of this thread dispatched to
// (torch.ops.ddlpc.last_path): "<operator>:<kernel variant>:<decisions that change the code that
// runs>", e.g. "conv3_fwd:stream:cfg5:ks1", "conv3_wgrad:v3:bco128:ciw1", "convt_fwd:res",
// "head_ce_bwd:head32:defer:stats", "bn_backward:v2:pool:kwin"; the CPU kernels
// (cpu_ref.cpp) report "cpu".  Host-side bookkeeping only: tests assert that a shape written
// for one kernel variant still runs it after the launch heuristics are retuned.
namespace {
thread_local std::string g_last_path;
}  // namespace
void set_last_path(const std::string& path) { g_last_path = path; }
std::string last_path() { return g_last_path; }

// ---- A/B switches for experiments in progress: knob(name, def) = an in-process override
// (torch.ops.ddlpc.set_knob) or else the environment variable DDLPC_<NAME>, or else def.
// Every name a kernel reads is listed in kKnobs; set_knob rejects any other name, so an A/B
// (bench.py --ab, scripts/conv_micro.py --ab) can never silently time two identical
// configurations.
//   CROP_LDS_T (default 1): crop_gather's transposing codes through LDS; 0 = the direct
//   strided read, kept for scripts/crop_micro.py's A/B (docs/PERF.md)
//   WINDOW_LDS_T (default 1): the same choice for window_gather's transposing codes
//   (scripts/predict_micro.py --tta, docs/PERF.md)
//   CONVT_WGRAD_WIDE (default: unset = convt_wgrad_wide_rule): the transposed-conv weight
//   gradient's 256-column-tile kernel; 0 = never, 1 = wherever its shape constraints hold
//   (scripts/conv_micro.py --passes twgradbn --ab, tests/test_convt_wgrad_wide_gpu.py)
namespace {
const char* const kKnobs[] = {"CROP_LDS_T", "WINDOW_LDS_T", "CONVT_WGRAD_WIDE"};
bool knob_registered(const std::string& name) {
  for (const char* k : kKnobs)
    if (k[0] != 0 && name == k) return true;
  return false;
}
std::mutex g_knob_mu;
std::unordered_map<std::string, int>& knob_map() {
  static std::unordered_map<std::string, int> m;
  return m;
}
}  // namespace

int knob(const char* name, int def) {
  TORCH_CHECK(knob_registered(name), "knob '", name, "' read but not listed in kKnobs");
  std::lock_guard<std::mutex> lk(g_knob_mu);
  auto& m = knob_map();
  auto it = m.find(name);
  if (it != m.end()) return it->second;
  const std::string env = std::string("DDLPC_") + name;
  const char* e = getenv(env.c_str());
  const int v = e ? atoi(e) : def;
  m.emplace(name, v);                   // (cached: the environment is read once per name)
  return v;
}

namespace {

// in-process knob override -> the previous value (INT64_MIN: never read or set)
int64_t set_knob(const std::string& name, int64_t value) {
  TORCH_CHECK(knob_registered(name), "set_knob: no kernel reads a knob named '", name,
              "' (registered knobs are listed in kKnobs, csrc/bindings.cpp)");
  std::lock_guard<std::mutex> lk(g_knob_mu);
  auto& m = knob_map();
  auto it = m.find(name);
  const int64_t prev = it != m.end() ? it->second : INT64_MIN;
  if (value == INT64_MIN) {             // clear: the next knob() re-reads the environment
    if (it != m.end()) m.erase(it);
  } else {
    m[name] = (int)value;
  }
  return prev;
}

int phys_cus() {
  static int n = -1;
  if (n < 0) {
    hipDeviceProp_t prop;
    int dev = 0;
    hipGetDevice(&dev);
    n = (hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
  }
  return n;
}

// CUs left out of every persistent / chip-filling grid (set_cu_reserve): under data
// parallelism an RCCL kernel launched in the middle of backward needs free workgroup slots
// at once, but the persistent conv / head kernels otherwise hold every CU until they exit
int g_cu_reserve = 0;

// the CU count grids are sized for
int num_cus() { return std::max(8, phys_cus() - g_cu_reserve); }

// fp64 column sums of an fp32 [R][N] partial slab (deterministic two-pass reduction)
at::Tensor reduce_rows(const at::Tensor& partial, int64_t R, int64_t N) {
  checks::reduce_rows(partial, R, N);
  auto dopts = partial.options().dtype(at::kDouble);
  at::Tensor sums = at::empty({N}, dopts);
  const int RC = reduce_rows_chunks((int)R);
  at::Tensor tmp = RC > 1 ? at::empty({2 * RC * N}, dopts) : sums;
  reduce_rows_launch(partial.data_ptr<float>(), (int)R, N, tmp.data_ptr<double>(),
                     sums.data_ptr<double>(), cur_stream());
  return sums;
}

// dst (+)= the permuted fp64 row sums of an fp32 slab [R][N] of partial results (a split-K
// weight gradient, per-workgroup channel sums): reduce_rows_scatter_launch and its scratch
void sum_slab(const at::Tensor& slab, int R, long long N, at::Tensor& dst, int mode, int A, int T,
              int B, bool accumulate, long long ld = -1) {
  at::Tensor tmp = at::empty({(int64_t)reduce_rows_scatter_tmp(R, N)}, slab.options().dtype(at::kDouble));
  reduce_rows_scatter_launch(slab.data_ptr<float>(), R, N, tmp.data_ptr<double>(), dst.data_ptr<float>(),
                             mode, A, T, B, accumulate, cur_stream(), ld);
}

// sum_slab as an operator (the exact tests of the gradient tail drive every row-count regime
// and layout mode of reduce_rows_scatter_launch through it; the operators call sum_slab).
// Rows of N columns at a row stride of ld floats (-1: N); mode 0 / 1: N = A * T * B with
// A = N / (T * B)
void reduce_rows_scatter(const at::Tensor& slab, int64_t R, int64_t N, at::Tensor& dst, int64_t mode,
                         int64_t T, int64_t B, bool accumulate, int64_t ld) {
  CHECK_DEV(slab);
  const int64_t A = checks::reduce_rows_scatter(slab, R, N, dst, mode, T, B, ld);
  if (R == 0 || N == 0) return;
  c10::DeviceGuard guard(slab.device());
  sum_slab(slab, (int)R, N, dst, (int)mode, (int)A, (int)T, (int)B, accumulate, ld);
}

// BatchNorm-backward coefficients [k|m1|m2] x C and dgamma / dbeta (accumulated into the outs
// when given) from nb partial rows [nb][2][C] of (sum dyh, sum dyh * xhat): one kernel over
// the rows, or — many rows (per-tile epilogue partials) — the coalesced two-pass fp64
// reduction first.  dscale: optional device factor on the rows
struct BnGrad {
  at::Tensor coefs, dgamma, dbeta;
  bool two_pass;
};
BnGrad bn_grad_from_rows(const at::Tensor& partial, int nb, int C, double count, const at::Tensor& gamma,
                         const float* invstd, const c10::optional<at::Tensor>& dgamma_out,
                         const c10::optional<at::Tensor>& dbeta_out, const float* dscale = nullptr) {
  auto fopts = partial.options();
  const bool into = has(dgamma_out);
  BnGrad r{at::empty({3, C}, fopts), into ? *dgamma_out : at::empty({C}, fopts),
           into ? *dbeta_out : at::empty({C}, fopts), nb > 2048};
  if (!r.two_pass) {
    bn_grad_finalize_rows_launch(partial.data_ptr<float>(), nb, C, count, gamma.data_ptr<float>(), invstd,
                                 r.dgamma.data_ptr<float>(), r.dbeta.data_ptr<float>(),
                                 r.coefs.data_ptr<float>(), into, cur_stream(), dscale);
  } else {
    at::Tensor sums = reduce_rows(partial, nb, 2 * C);
    bn_grad_finalize_launch(sums.data_ptr<double>(), C, count, gamma.data_ptr<float>(), invstd,
                            r.dgamma.data_ptr<float>(), r.dbeta.data_ptr<float>(),
                            r.coefs.data_ptr<float>(), into, cur_stream(), dscale);
  }
  return r;
}

// an arena slot (optional, checked by checks::arena_arg): the pointer to column aoff of row 0
// and the row stride
std::pair<float*, long long> arena_slot(const c10::optional<at::Tensor>& arena, int64_t aoff) {
  if (!has(arena)) return {nullptr, 0};
  return {arena->data_ptr<float>() + aoff, (long long)arena->stride(0)};
}

// ------------------------------------------------------------------------ conv3 forward
std::vector<at::Tensor> conv3_fwd(const at::Tensor& x1, const c10::optional<at::Tensor>& x2,
                                  const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                                  const c10::optional<at::Tensor>& pscale,
                                  const c10::optional<at::Tensor>& pshift, int64_t cout,
                                  int64_t co1, bool want_stats_in,
                                  const c10::optional<at::Tensor>& pscale2,
                                  const c10::optional<at::Tensor>& pshift2,
                                  const c10::optional<at::Tensor>& bnb_y,
                                  const c10::optional<at::Tensor>& bnb_s4, int64_t groups) {
  CHECK_DEV(x1); CHECK_CONTIG(x1); CHECK_BF16(x1); CHECK_BF16(w); CHECK_CONTIG(w);
  c10::DeviceGuard guard(x1.device());
  const Geo g = geo_of(x1);
  bool want_stats = want_stats_in;
  ConvFwdArgs a{};
  a.dims = g.dims; a.N = g.N; a.D = g.D; a.H = g.H; a.W = g.W;
  a.C1 = g.C;
  a.C2 = 0;
  const bool dual = has(x2);
  if (dual) {
    CHECK_CONTIG(*x2); CHECK_BF16(*x2);
    const Geo g2 = geo_of(*x2);
    TORCH_CHECK(g2.N == g.N && g2.H == g.H && g2.W == g.W && g2.D == g.D, "concat shape mismatch");
    TORCH_CHECK(g.C % 8 == 0 && g2.C % 8 == 0, "concat inputs need C % 8 == 0");
    a.C2 = g2.C;
  }
  a.Cin = a.C1 + a.C2;
  a.taps = g.dims == 2 ? 9 : 27;
  TORCH_CHECK(w.dim() == 3 && w.size(0) == cout && w.size(1) == a.taps && w.size(2) >= a.Cin,
              "packed weight must be [Cout][taps][CinW>=Cin]");
  a.CinW = (int)w.size(2);
  TORCH_CHECK(a.CinW % 8 == 0, "packed weight ci stride must be a multiple of 8");
  a.Cout = (int)cout;
  a.Co1 = co1 > 0 ? (int)co1 : (int)cout;
  TORCH_CHECK(a.Cout % 8 == 0 && a.Co1 % 8 == 0, "Cout and Co1 must be multiples of 8");
  if (has(pscale)) TORCH_CHECK(a.C1 <= 512, "prologue supports C1 <= 512");
  // BN groups (ConvFwdArgs::groups): group-major statistics rows; pscale / pshift (and the
  // BNB table) per group — pscale / pshift are [groups][C1] views with a common row stride
  // (the scale / shift rows of group statistics [groups][4][C1])
  const bool grouped = groups > 1;
  if (grouped) {
    TORCH_CHECK(groups <= 1024 && g.N % groups == 0, "conv3_fwd: groups must divide the batch");
    TORCH_CHECK(!has(pscale2), "conv3_fwd groups: no X2 prologue");
    a.groups = (int)groups;
    if (has(pscale)) {
      TORCH_CHECK(has(pshift), "conv3_fwd groups: pscale needs pshift");
      CHECK_F32(*pscale); CHECK_F32(*pshift);
      TORCH_CHECK(pscale->dim() == 2 && pscale->size(0) == groups && pscale->size(1) == g.C &&
                  pscale->stride(1) == 1 && pshift->sizes() == pscale->sizes() &&
                  pshift->strides() == pscale->strides(),
                  "conv3_fwd groups: pscale / pshift must be [groups][C1] views with one row stride");
      a.gstride = pscale->stride(0);
    }
  }
  a.X1 = bptr(x1);
  a.X2 = dual ? bptr(*x2) : nullptr;
  a.pscale = fptr_opt(pscale);
  a.pshift = fptr_opt(pshift);
  a.pscale2 = fptr_opt(pscale2);
  a.pshift2 = fptr_opt(pshift2);
  if (a.pscale2 != nullptr)
    TORCH_CHECK(dual && a.pshift2 != nullptr && a.C1 + a.C2 <= 512 && pscale2->numel() == a.C2,
                "X2 prologue: needs x2, both pscale2/pshift2 [C2], and C1 + C2 <= 512");
  a.Wt = bptr(w);
  a.bias = fptr_opt(bias);
  if (has(bnb_y)) {
    // BN-backward epilogue: the stats rows become that BN's (sum dyh, sum dyh*xhat) partials
    CHECK_CONTIG(*bnb_y); CHECK_BF16(*bnb_y);
    const int64_t ng = grouped ? groups : 1;
    TORCH_CHECK(has(bnb_s4) && bnb_s4->numel() == ng * 4 * cout,
                "bnb: stats4 [4][Cout] ([groups][4][Cout] with groups) required");
    if (grouped) a.gstride = 4LL * cout;
    CHECK_F32(*bnb_s4); CHECK_CONTIG(*bnb_s4);
    const Geo gy = geo_of(*bnb_y);
    TORCH_CHECK(g.dims == 2 && gy.N == g.N && gy.H == g.H && gy.W == g.W && gy.C == cout,
                "bnb: 2-D, y must have the output's shape");
    TORCH_CHECK(a.Co1 == a.Cout && a.pscale == nullptr && a.pscale2 == nullptr && a.bias == nullptr,
                "bnb: single output, no prologue, no bias");
    a.bnb_y = bptr(*bnb_y);
    a.bnb_s4 = bnb_s4->data_ptr<float>();
    want_stats = true;
  }
  TORCH_CHECK(a.C2 == 0 || a.C1 % 32 == 0, "concat: first input needs C1 % 32 == 0");
  TORCH_CHECK((a.C1 % 8 == 0) && (a.C2 % 8 == 0), "input channels must be multiples of 8 "
              "(the engine pads the 3-channel image to 8)");
  a.npix = (long long)g.N * g.D * g.H * g.W;
  const ConvFwdPlan p = conv3_fwd_plan(a, num_cus(), want_stats);
  TORCH_CHECK(p.error == nullptr, p.error);
  auto opts = x1.options();
  at::Tensor none = at::empty({0}, opts);
  at::Tensor y1 = at::empty(shape_with_c(g, a.Co1), opts);
  at::Tensor y2 = a.Co1 < a.Cout ? at::empty(shape_with_c(g, a.Cout - a.Co1), opts) : none;
  at::Tensor stats = want_stats ? at::empty({(int64_t)p.stat_rows, 2, a.Cout}, opts.dtype(at::kFloat)) : none;
  at::Tensor part;                // split-K: fp32 partial sums [ksplit][npix][Cout]
  if (a.ksplit > 1) {
    part = at::empty({(int64_t)a.ksplit * a.npix * a.Cout}, opts.dtype(at::kFloat));
    a.part = part.data_ptr<float>();
  }
  a.Y1 = bptr_mut(y1);
  a.Y2 = a.Co1 < a.Cout ? bptr_mut(y2) : nullptr;
  a.stats = want_stats ? stats.data_ptr<float>() : nullptr;
  set_last_path(p.path);
  switch (p.kernel) {
    case CONV_FWD_DS: conv3d_ds_launch(a, p.grid, p.smem, cur_stream()); break;
    case CONV_FWD_RES: conv3_res_launch(a, p.variant, p.grid, p.smem, cur_stream()); break;
    default:
      conv3_fwd_launch(a, p.variant, cur_stream());
      if (a.ksplit > 1) conv3_splitk_finalize_launch(a, p.fin_grid, cur_stream());
  }
  return {y1, y2, stats};
}

// ------------------------------------------------------------------------ conv3 wgrad
at::Tensor conv3_wgrad(const at::Tensor& dy, const at::Tensor& x1,
                       const c10::optional<at::Tensor>& x2, const c10::optional<at::Tensor>& pscale,
                       const c10::optional<at::Tensor>& pshift,
                       const c10::optional<at::Tensor>& out,
                       const c10::optional<at::Tensor>& pscale2,
                       const c10::optional<at::Tensor>& pshift2,
                       const c10::optional<at::Tensor>& dy_y,
                       const c10::optional<at::Tensor>& dy_s4,
                       const c10::optional<at::Tensor>& dy_coefs, int64_t cin_real,
                       int64_t groups, const c10::optional<at::Tensor>& dy_out) {
  CHECK_DEV(dy); CHECK_CONTIG(dy); CHECK_BF16(dy); CHECK_CONTIG(x1); CHECK_BF16(x1);
  c10::DeviceGuard guard(dy.device());
  const Geo g = geo_of(x1);
  const Geo gy = geo_of(dy);
  TORCH_CHECK(gy.N == g.N && gy.H == g.H && gy.W == g.W && gy.D == g.D, "dy/x shape mismatch");
  ConvWgradArgs a{};
  a.dims = g.dims; a.N = g.N; a.D = g.D; a.H = g.H; a.W = g.W;
  a.C1 = g.C; a.C2 = 0;
  const bool dual = has(x2);
  if (dual) { CHECK_CONTIG(*x2); a.C2 = (int)x2->size(-1); }
  a.Cin = a.C1 + a.C2;
  a.Cout = gy.C;
  TORCH_CHECK(a.Cout % 8 == 0, "Cout must be a multiple of 8");
  a.taps = g.dims == 2 ? 9 : 27;
  a.dY = bptr(dy);
  a.X1 = bptr(x1);
  a.X2 = dual ? bptr(*x2) : nullptr;
  a.pscale = fptr_opt(pscale);
  a.pshift = fptr_opt(pshift);
  a.pscale2 = fptr_opt(pscale2);
  a.pshift2 = fptr_opt(pshift2);
  if (a.pscale) TORCH_CHECK(a.C1 <= 512, "prologue supports C1 <= 512");
  // BN groups: the X1 prologue constants per group of images (pscale / pshift: [groups][C1]
  // views with one row stride, as conv3_fwd's); v3 kernel only (checked below)
  if (groups > 1 && a.pscale != nullptr) {
    TORCH_CHECK(groups <= 1024 && g.N % groups == 0, "conv3_wgrad: groups must divide the batch");
    TORCH_CHECK(a.pscale2 == nullptr && !dual, "conv3_wgrad groups: single input, no X2 prologue");
    TORCH_CHECK(pscale->dim() == 2 && pscale->size(0) == groups && pscale->size(1) == a.C1 &&
                pscale->stride(1) == 1 && pshift->sizes() == pscale->sizes() &&
                pshift->strides() == pscale->strides(),
                "conv3_wgrad groups: pscale / pshift must be [groups][C1] views with one row stride");
    a.groups = (int)groups;
    a.gimg = g.N / (int)groups;
    a.gstride = pscale->stride(0);
  }
  if (a.pscale2) TORCH_CHECK(dual && a.pshift2 && a.C1 + a.C2 <= 512, "X2 prologue: x2, pscale2/pshift2, C1 + C2 <= 512");
  const bool emit = has(dy_out);
  if (has(dy_y)) {
    // dy holds dA; BN backward applied on load (which kernels can: conv3_wgrad_plan)
    CHECK_CONTIG(*dy_y); CHECK_BF16(*dy_y);
    TORCH_CHECK(dy_y->numel() == dy.numel(),
                "conv3_wgrad: the dY prologue needs the v2 kernel (2-D, C1 % 32 != 0 or a 32-channel "
                "first layer) or dy_out, and y of dY's shape");
    TORCH_CHECK(has(dy_s4) && dy_s4->numel() == 4 * a.Cout && has(dy_coefs) &&
                dy_coefs->numel() == 3 * a.Cout, "conv3_wgrad: dy_s4 [4][Cout] and dy_coefs [3][Cout]");
    CHECK_F32(*dy_s4); CHECK_F32(*dy_coefs);
    a.dyy = bptr(*dy_y);
    a.dys4 = dy_s4->data_ptr<float>();
    a.dycoef = dy_coefs->data_ptr<float>();
    if (emit) {
      CHECK_CONTIG(*dy_out); CHECK_BF16(*dy_out);
      TORCH_CHECK(dy_out->numel() == dy.numel(), "conv3_wgrad: dy_out must have dY's shape");
      a.dyout = reinterpret_cast<bf16_t*>(dy_out->data_ptr());
    }
  }
  TORCH_CHECK(!emit || a.dyy != nullptr, "conv3_wgrad: dy_out needs the dY prologue (dy_y, dy_s4, dy_coefs)");
  const bool into = has(out);
  if (into) {
    CHECK_F32(*out); CHECK_CONTIG(*out);
    TORCH_CHECK(out->numel() == (int64_t)a.Cout * a.Cin * a.taps, "dW out size mismatch");
  }
  const ConvWgradPlan p = conv3_wgrad_plan(a, num_cus(), (int)std::max<int64_t>(0, std::min<int64_t>(cin_real, INT32_MAX)), emit);
  TORCH_CHECK(p.error == nullptr, p.error);
  auto fopts = dy.options().dtype(at::kFloat);
  const long long NW = (long long)a.Cout * a.taps * a.Cin;
  at::Tensor part = at::empty({(int64_t)a.splits * NW}, fopts);
  a.partial = part.data_ptr<float>();
  std::vector<int64_t> wshape = {a.Cout, a.Cin, 3, 3};
  if (g.dims == 3) wshape.push_back(3);
  at::Tensor dW = into ? *out : at::empty(wshape, fopts);
  set_last_path(p.path);
  switch (p.kernel) {
    case WGRAD_DS: conv3d_wgrad_ds_launch(a, p.grid, cur_stream()); break;
    case WGRAD_C32: conv3_wgrad_c32_launch(a, p.grid, cur_stream()); break;
    case WGRAD_IMG: conv3_wgrad_img_launch(a, p.bco, cur_stream()); break;
    case WGRAD_V3: conv3_wgrad3_launch(a, p.bco, cur_stream()); break;
    case WGRAD_V2: conv3_wgrad2_launch(a, p.bco, cur_stream()); break;
    default: conv3_wgrad_launch(a, p.bco, cur_stream());
  }
  sum_slab(part, a.splits, NW, dW, 0, a.Cout, a.taps, a.Cin, into);
  return into ? at::empty({0}, fopts) : dW;
}

// ------------------------------------------------------------------------ fused 32-channel backward
// The second conv of a 32-channel DoubleConv (input relu(bn1(y))): data gradient dA with the
// BN1-backward partial rows [grid][2][32] and the weight gradient (OIHW [32][32][3][3],
// accumulated into dw_out when given) from one pass over dY and y (conv3x3_bwd32.hip)
std::vector<at::Tensor> conv3_bwd32(const at::Tensor& dy, const at::Tensor& y, const at::Tensor& s4,
                                    const at::Tensor& wd, const c10::optional<at::Tensor>& dw_out,
                                    int64_t groups) {
  CHECK_DEV(dy); CHECK_CONTIG(dy); CHECK_BF16(dy); CHECK_CONTIG(y); CHECK_BF16(y);
  CHECK_BF16(wd); CHECK_CONTIG(wd); CHECK_F32(s4); CHECK_CONTIG(s4);
  c10::DeviceGuard guard(dy.device());
  const Geo g = geo_of(dy);
  const Geo gy = geo_of(y);
  TORCH_CHECK(g.dims == 2 && g.C == 32 && gy.dims == 2 && gy.C == 32 && gy.N == g.N && gy.H == g.H &&
              gy.W == g.W, "conv3_bwd32: 2-D dY and y of one shape with 32 channels");
  const int G = groups > 1 ? (int)groups : 1;
  TORCH_CHECK(G <= 1024 && g.N % G == 0, "conv3_bwd32: groups must divide the batch");
  TORCH_CHECK(wd.numel() == 32 * 9 * 32 && s4.numel() == (int64_t)G * 4 * 32,
              "conv3_bwd32: data-gradient pack [32][9][32] and stats4 [4][32] ([groups][4][32])");
  TORCH_CHECK((long long)g.H * g.W * 64 < (1LL << 31), "conv3_bwd32: image too large for 32-bit offsets");
  Bwd32Args a{};
  a.N = g.N; a.H = g.H; a.W = g.W;
  a.dY = bptr(dy); a.Y = bptr(y); a.s4 = s4.data_ptr<float>(); a.Wd = bptr(wd);
  a.tilesH = (g.H + 15) / 16; a.tilesW = (g.W + 15) / 16;
  a.nTiles = g.N * a.tilesH * a.tilesW;
  a.groups = G;
  const int grid = conv3_bwd32_grid(a.nTiles, num_cus(), G);
  auto fopts = dy.options().dtype(at::kFloat);
  at::Tensor dA = at::empty_like(dy);
  at::Tensor bnpart = at::empty({grid, 2, 32}, fopts);
  at::Tensor wpart = at::empty({(int64_t)grid * 32 * 9 * 32}, fopts);
  a.dA = bptr_mut(dA); a.bnpart = bnpart.data_ptr<float>(); a.wpart = wpart.data_ptr<float>();
  set_last_path(G > 1 ? "conv3_bwd32:groups" : "conv3_bwd32");
  conv3_bwd32_launch(a, grid, cur_stream());
  const bool into = has(dw_out);
  if (into) {
    CHECK_F32(*dw_out); CHECK_CONTIG(*dw_out);
    TORCH_CHECK(dw_out->numel() == 32 * 32 * 9, "dW out size mismatch");
  }
  at::Tensor dW = into ? *dw_out : at::empty({32, 32, 3, 3}, fopts);
  sum_slab(wpart, grid, 32LL * 9 * 32, dW, 0, 32, 9, 32, into);
  return {dA, bnpart, into ? at::empty({0}, fopts) : dW};
}

// ------------------------------------------------------------------------ BatchNorm
// returns stats4 [4][C] = (mean, invstd, scale, shift)
at::Tensor bn_finalize(const at::Tensor& partial, double count, const at::Tensor& gamma,
                       const at::Tensor& beta, at::Tensor running_mean, at::Tensor running_var,
                       double momentum, double eps, bool update_running,
                       const c10::optional<at::Tensor>& nbt) {
  CHECK_DEV(partial); CHECK_CONTIG(partial); CHECK_CONTIG(gamma); CHECK_CONTIG(beta);
  checks::bn_finalize(partial, gamma, beta, running_mean, running_var, nbt);
  c10::DeviceGuard guard(partial.device());
  const int C = (int)gamma.numel();
  const int P = (int)(partial.numel() / (2 * C));
  at::Tensor st = at::empty({4, C}, partial.options());
  int64_t* nbp = has(nbt) ? nbt->data_ptr<int64_t>() : nullptr;
  if (P <= 4096) {
    bn_stats_finalize_rows_launch(partial.data_ptr<float>(), P, C, count, gamma.data_ptr<float>(),
                                  beta.data_ptr<float>(), running_mean.data_ptr<float>(),
                                  running_var.data_ptr<float>(), (float)momentum, (float)eps,
                                  st.data_ptr<float>(), update_running, nbp, cur_stream());
    set_last_path("bn_finalize:rows");
    return st;
  }
  set_last_path("bn_finalize:two_pass");
  at::Tensor sums = reduce_rows(partial, P, 2 * C);
  bn_stats_finalize_launch(sums.data_ptr<double>(), C, count, gamma.data_ptr<float>(),
                           beta.data_ptr<float>(), running_mean.data_ptr<float>(),
                           running_var.data_ptr<float>(), (float)momentum, (float)eps,
                           st.data_ptr<float>(), update_running, nbp, cur_stream());
  return st;
}

// deferred BatchNorm running-statistics updates, in micro-batch order (see reduce.hip)
void bn_running_apply(at::Tensor running_mean, at::Tensor running_var, const at::Tensor& slots,
                      double momentum, const c10::optional<at::Tensor>& nbt) {
  CHECK_DEV(slots);
  checks::bn_running_apply(running_mean, running_var, slots, nbt);
  const int C = (int)running_mean.numel();
  c10::DeviceGuard guard(slots.device());
  const int K = (int)slots.size(0);
  if (K == 0) return;
  int64_t* nbp = has(nbt) ? nbt->data_ptr<int64_t>() : nullptr;
  bn_running_apply_launch(running_mean.data_ptr<float>(), running_var.data_ptr<float>(),
                          slots.data_ptr<float>(), K, C, (long long)slots.stride(0), (float)momentum,
                          nbp, cur_stream());
}

// every BatchNorm's deferred running-statistics updates in one launch: entries [L][4] int64
// (running_mean*, running_var*, nbt* | 0, C | arena column << 32), arena rows 0..K-1
void bn_running_apply_all(const at::Tensor& entries, const at::Tensor& arena, int64_t K,
                          int64_t maxC, double momentum) {
  CHECK_DEV(arena); CHECK_CONTIG(entries);
  checks::bn_running_apply_all(entries, arena, K, maxC);
  TORCH_CHECK(entries.size(0) <= 65535, "bn_running_apply_all: at most 65535 layers");
  c10::DeviceGuard guard(arena.device());
  if (K == 0 || entries.size(0) == 0) return;
  bn_running_apply_all_launch(entries.data_ptr<int64_t>(), (int)entries.size(0), (int)maxC,
                              arena.data_ptr<float>(), (int)K, (long long)arena.stride(0),
                              (float)momentum, cur_stream());
}

std::vector<at::Tensor> bn_relu_apply(const at::Tensor& y, const at::Tensor& stats4, bool pool,
                                      bool full) {
  CHECK_DEV(y); CHECK_CONTIG(y); CHECK_CONTIG(stats4);
  checks::bn_relu_apply(y, stats4, pool, full);
  c10::DeviceGuard guard(y.device());
  const Geo g = geo_of(y);
  TORCH_CHECK(g.C % 8 == 0, "C must be a multiple of 8");
  const float* s = stats4.data_ptr<float>();
  at::Tensor a = full ? at::empty_like(y) : at::empty({0}, y.options());
  at::Tensor p;
  if (pool) p = at::empty(pooled_shape(g), y.options());
  const char* variant =
      bn_relu_apply_launch(bptr(y), s + 2 * g.C, s + 3 * g.C, full ? bptr_mut(a) : nullptr,
                           pool ? bptr_mut(p) : nullptr, g.dims, g.N, g.D, g.H, g.W, g.C, cur_stream());
  set_last_path(std::string("bn_relu_apply:") + variant + (g.dims == 3 ? ":3d" : ""));
  return {a, p.defined() ? p : at::empty({0}, y.options())};
}

// dY, dgamma, dbeta from dA (+ unpool(dP)) through ReLU and BN
std::vector<at::Tensor> bn_backward(const c10::optional<at::Tensor>& dA,
                                    const c10::optional<at::Tensor>& dP, const at::Tensor& y,
                                    const at::Tensor& stats4, const at::Tensor& gamma,
                                    const c10::optional<at::Tensor>& gscale,
                                    const c10::optional<at::Tensor>& dgamma_out,
                                    const c10::optional<at::Tensor>& dbeta_out,
                                    const c10::optional<at::Tensor>& partial_in) {
  CHECK_DEV(y); CHECK_CONTIG(y); CHECK_CONTIG(stats4); CHECK_CONTIG(gamma);
  checks::bn_backward(dA, dP, y, stats4, gamma, gscale, dgamma_out, dbeta_out, partial_in);
  c10::DeviceGuard guard(y.device());
  const Geo g = geo_of(y);
  const int C = g.C;
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  const bool hasA = has(dA);
  const bool hasP = has(dP);
  if (hasA) CHECK_CONTIG(*dA);
  if (hasP) CHECK_CONTIG(*dP);
  const float* s = stats4.data_ptr<float>();
  const float* gs = fptr_opt(gscale);
  const long long items = (long long)g.N * (hasP ? (g.dims == 3 ? g.D / 2 : 1) * (g.H / 2) * (g.W / 2)
                                                 : (long long)g.D * g.H * g.W);
  auto fopts = y.options().dtype(at::kFloat);
  const bf16_t* pA = hasA ? bptr(*dA) : nullptr;
  const bf16_t* pP = hasP ? bptr(*dP) : nullptr;
  // partial_in: (sum dyh, sum dyh*xhat) rows [R][2][C] already produced by the kernel that
  // wrote dA (deferred-BN epilogues); otherwise one reduction pass over dA (+dP) and y
  const bool pre = has(partial_in) && partial_in->numel() > 0;
  int nb;
  at::Tensor partial;
  if (pre) {
    CHECK_CONTIG(*partial_in);
    partial = *partial_in;
    nb = (int)(partial.numel() / (2 * C));
  } else {
    nb = bn_bwd_reduce_blocks(items);
    partial = at::empty({nb, 2, C}, fopts);
    bn_bwd_reduce_launch(pA, pP, bptr(y), s + 2 * C, s + 3 * C, s, s + C, gs,
                         partial.data_ptr<float>(), nb, g.dims, g.N, g.D, g.H, g.W, C, cur_stream());
  }
  const double count = (double)g.N * g.D * g.H * g.W;
  const BnGrad r = bn_grad_from_rows(partial, nb, C, count, gamma, s + C, dgamma_out, dbeta_out);
  at::Tensor dY = at::empty_like(y);
  const char* variant =
      bn_bwd_apply_launch(pA, pP, bptr(y), s + 2 * C, s + 3 * C, s, s + C, r.coefs.data_ptr<float>(), gs,
                          bptr_mut(dY), g.dims, g.N, g.D, g.H, g.W, C, cur_stream());
  set_last_path(std::string("bn_backward:") + variant + (g.dims == 3 ? ":3d" : "") + (pre ? ":rows" : "") +
                (r.two_pass ? ":two_pass" : ""));
  return {dY, r.dgamma, r.dbeta};
}

// BatchNorm backward WITHOUT the apply pass: from precomputed (sum dyh, sum dyh*xhat) rows,
// dgamma / dbeta (accumulated into the outs when given) and the dY coefficients [k|m1|m2]
// for a consumer that applies the backward on load (conv3_wgrad's dY prologue)
std::vector<at::Tensor> bn_grad_coefs(const at::Tensor& partial, const at::Tensor& y,
                                      const at::Tensor& stats4, const at::Tensor& gamma,
                                      const c10::optional<at::Tensor>& dgamma_out,
                                      const c10::optional<at::Tensor>& dbeta_out) {
  CHECK_DEV(partial); CHECK_CONTIG(partial); CHECK_CONTIG(stats4); CHECK_CONTIG(gamma);
  checks::bn_grad_coefs(partial, y, stats4, gamma, dgamma_out, dbeta_out);
  c10::DeviceGuard guard(partial.device());
  const Geo g = geo_of(y);
  const int C = g.C;
  const int nb = (int)(partial.numel() / (2 * C));
  const double count = (double)g.N * g.D * g.H * g.W;
  const BnGrad r = bn_grad_from_rows(partial, nb, C, count, gamma, stats4.data_ptr<float>() + C,
                                     dgamma_out, dbeta_out);
  set_last_path(r.two_pass ? "bn_grad_coefs:two_pass" : "bn_grad_coefs:rows");
  return {r.coefs, r.dgamma, r.dbeta};
}

// ------------------------------------------------------------------------ BatchNorm groups
// per-micro-batch statistics groups (Trainer bn_window): y holds `groups` micro-batches one
// after another; -> stats4 [groups][4][C]; with an arena [rows][...] the group's
// (mean | unbiased var) goes to arena row g at column aoff (in-order running-stat update)
at::Tensor bn_group_finalize(const at::Tensor& y, int64_t groups, const at::Tensor& gamma,
                             const at::Tensor& beta, double eps,
                             const c10::optional<at::Tensor>& arena, int64_t aoff) {
  CHECK_DEV(y); CHECK_CONTIG(y); CHECK_CONTIG(gamma); CHECK_CONTIG(beta);
  checks::bn_group_finalize(y, groups, gamma, beta, arena, aoff);
  c10::DeviceGuard guard(y.device());
  const Geo g = geo_of(y);
  TORCH_CHECK(bn_group_supported(g.dims, false, g.D, g.H, g.W, g.C),
              "bn_group_finalize: C / 8 must be a power of two <= 256");
  const long long gpix = (long long)(g.N / groups) * g.D * g.H * g.W;
  const int nb = bn_group_stats_rows(gpix, g.C, (int)groups);
  auto fopts = y.options().dtype(at::kFloat);
  at::Tensor part = at::empty({groups, nb, 2, g.C}, fopts);
  at::Tensor st = at::empty({groups, 4, g.C}, fopts);
  const auto [ap, astride] = arena_slot(arena, aoff);
  bn_group_stats_finalize_launch(bptr(y), (int)groups, gpix, g.C, gamma.data_ptr<float>(),
                                 beta.data_ptr<float>(), (float)eps, st.data_ptr<float>(), ap,
                                 astride, part.data_ptr<float>(), nb, cur_stream());
  return st;
}

// the same statistics from partial rows a conv epilogue wrote group-major (conv3_fwd with
// groups): partial [groups * nb][2][C], count = pixels per group
at::Tensor bn_group_finalize_rows(const at::Tensor& partial, int64_t groups, double count,
                                  const at::Tensor& gamma, const at::Tensor& beta, double eps,
                                  const c10::optional<at::Tensor>& arena, int64_t aoff) {
  CHECK_DEV(partial); CHECK_CONTIG(partial); CHECK_CONTIG(gamma); CHECK_CONTIG(beta);
  checks::bn_group_finalize_rows(partial, groups, gamma, beta, arena, aoff);
  c10::DeviceGuard guard(partial.device());
  const int64_t C = gamma.numel();
  const int nb = (int)(partial.numel() / (groups * 2 * C));
  at::Tensor st = at::empty({groups, 4, C}, partial.options());
  const auto [ap, astride] = arena_slot(arena, aoff);
  bn_group_finalize_rows_launch(partial.data_ptr<float>(), nb, (int)groups, (long long)count, (int)C,
                                gamma.data_ptr<float>(), beta.data_ptr<float>(), (float)eps,
                                st.data_ptr<float>(), ap, astride, cur_stream());
  return st;
}

std::vector<at::Tensor> bn_group_apply(const at::Tensor& y, const at::Tensor& stats4,
                                       int64_t groups, bool pool) {
  CHECK_DEV(y); CHECK_CONTIG(y); CHECK_CONTIG(stats4);
  checks::bn_group_apply(y, stats4, groups, pool);
  c10::DeviceGuard guard(y.device());
  const Geo g = geo_of(y);
  TORCH_CHECK(g.C % 8 == 0, "C must be a multiple of 8");
  at::Tensor a = at::empty_like(y);
  at::Tensor p;
  if (pool) p = at::empty(pooled_shape(g), y.options());
  const float* s = stats4.data_ptr<float>();
  const char* variant =
      bn_relu_apply_launch(bptr(y), s + 2 * g.C, s + 3 * g.C, bptr_mut(a), pool ? bptr_mut(p) : nullptr,
                           g.dims, g.N / (int)groups, g.D, g.H, g.W, g.C, cur_stream(), (int)groups,
                           4LL * g.C);
  set_last_path(std::string("bn_group_apply:") + variant + (g.dims == 3 ? ":3d" : "") +
                (groups > 1 ? ":groups" : ""));
  return {a, p.defined() ? p : at::empty({0}, y.options())};
}

// dY (+ dgamma, dbeta summed over the groups, accumulated into the outs when given)
std::vector<at::Tensor> bn_group_backward(const c10::optional<at::Tensor>& dA,
                                          const c10::optional<at::Tensor>& dP, const at::Tensor& y,
                                          const at::Tensor& stats4, const at::Tensor& gamma,
                                          int64_t groups,
                                          const c10::optional<at::Tensor>& dgamma_out,
                                          const c10::optional<at::Tensor>& dbeta_out,
                                          const c10::optional<at::Tensor>& partial) {
  CHECK_DEV(y); CHECK_CONTIG(y); CHECK_CONTIG(stats4); CHECK_CONTIG(gamma);
  checks::bn_group_backward(dA, dP, y, stats4, gamma, groups, dgamma_out, dbeta_out, partial);
  c10::DeviceGuard guard(y.device());
  const Geo g = geo_of(y);
  const int C = g.C;
  const bool hasA = has(dA);
  const bool hasP = has(dP);
  if (hasA) CHECK_CONTIG(*dA);
  if (hasP) CHECK_CONTIG(*dP);
  TORCH_CHECK(bn_group_supported(g.dims, hasP, g.D, g.H, g.W, C),
              "bn_group_backward: C / 8 a power of two <= 256, even dims with pool");
  const int Ng = g.N / (int)groups;
  const long long items = (long long)Ng * (hasP ? (g.dims == 3 ? g.D / 2 : 1) * (g.H / 2) * (g.W / 2)
                                                : (long long)g.D * g.H * g.W);
  // partial: group-major rows [groups * nb][2][C] of (sum dyh, sum dyh * xhat) from the
  // data-gradient conv's BN-backward epilogue (conv3_fwd with bnb_y and groups)
  // (an empty tensor means no rows, as for bn_backward and on the CPU)
  const bool have_part = has(partial) && partial->numel() > 0;
  if (have_part) CHECK_CONTIG(*partial);
  const int nb = have_part ? (int)(partial->numel() / (groups * 2 * C)) : bn_group_bwd_rows(items, (int)groups);
  auto fopts = y.options().dtype(at::kFloat);
  at::Tensor part = have_part ? *partial : at::empty({groups, nb, 2, C}, fopts);
  at::Tensor coefs = at::empty({groups, 3, C}, fopts);
  const bool into = has(dgamma_out);
  at::Tensor dgamma = into ? *dgamma_out : at::empty({C}, fopts);
  at::Tensor dbeta = into ? *dbeta_out : at::empty({C}, fopts);
  at::Tensor dY = at::empty_like(y);
  at::Tensor gsum = at::empty({groups, 2, C}, y.options().dtype(at::kDouble));
  const char* variant = bn_group_backward_launch(
      hasA ? bptr(*dA) : nullptr, hasP ? bptr(*dP) : nullptr, bptr(y), stats4.data_ptr<float>(),
      gamma.data_ptr<float>(), dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), into,
      coefs.data_ptr<float>(), part.data_ptr<float>(), nb, bptr_mut(dY), g.dims, (int)groups, Ng, g.D,
      g.H, g.W, C, cur_stream(), have_part, gsum.data_ptr<double>());
  set_last_path(std::string("bn_group_backward:") + variant + (g.dims == 3 ? ":3d" : "") +
                (have_part ? ":rows" : "") + (groups > 1 ? ":groups" : ""));
  return {dY, dgamma, dbeta};
}

static const float* bn4_ptr(const c10::optional<at::Tensor>& bn4, int C) {
  if (!has(bn4)) return nullptr;
  CHECK_F32(*bn4); CHECK_CONTIG(*bn4);
  TORCH_CHECK(bn4->numel() == 4 * C, "bn4 must be [4][C] (mean, invstd, scale, shift)");
  TORCH_CHECK(C <= 512, "deferred BatchNorm supports C <= 512");
  return bn4->data_ptr<float>();
}

// ------------------------------------------------------------------------ transposed conv
at::Tensor convt_fwd(const at::Tensor& x, const at::Tensor& wt, const c10::optional<at::Tensor>& bias,
                     int64_t cout, const c10::optional<at::Tensor>& bn4) {
  CHECK_DEV(x); CHECK_CONTIG(x); CHECK_BF16(x); CHECK_BF16(wt);
  c10::DeviceGuard guard(x.device());
  const Geo g = geo_of(x);
  const int S = g.dims == 2 ? 4 : 8;
  TORCH_CHECK(g.C % 8 == 0 && cout % 8 == 0, "channels must be multiples of 8");
  TORCH_CHECK(wt.numel() == (int64_t)S * cout * g.C, "packed convT weight size mismatch");
  GemmArgs a{};
  a.mode = GEMM_CONVT_FWD;
  a.M = g.N * g.D * g.H * g.W;
  a.N = S * (int)cout;
  a.K = g.C;
  a.A = bptr(x);
  a.B = bptr(wt);
  a.bias = fptr_opt(bias);
  a.dims = g.dims; a.Nimg = g.N; a.D = g.D; a.H = g.H; a.W = g.W;
  a.Cin = g.C; a.Cout = (int)cout;
  a.bn4 = bn4_ptr(bn4, g.C);
  TORCH_CHECK((int64_t)a.M * (g.dims == 2 ? 4 : 8) < (int64_t)INT32_MAX, "convT: too many pixels for 32-bit pixel indices");
  at::Tensor out = at::empty(shape_with_c(g, (int)cout, 2), x.options());
  a.C = out.data_ptr();
  const bool res = convt_res_launch(a, num_cus(), cur_stream());
  if (!res) gemm_launch(a, cur_stream());
  set_last_path(res ? "convt_fwd:res" : "convt_fwd:gemm");
  return out;
}

std::vector<at::Tensor> convt_dgrad(const at::Tensor& dout, const at::Tensor& wd, int64_t cin,
                                    const c10::optional<at::Tensor>& bny,
                                    const c10::optional<at::Tensor>& bn4) {
  CHECK_DEV(dout); CHECK_CONTIG(dout); CHECK_BF16(dout); CHECK_BF16(wd);
  c10::DeviceGuard guard(dout.device());
  const Geo go = geo_of(dout);
  Geo g = go;
  g.H /= 2; g.W /= 2; if (g.dims == 3) g.D /= 2;
  const int S = g.dims == 2 ? 4 : 8;
  GemmArgs a{};
  a.mode = GEMM_CONVT_DGRAD;
  a.M = g.N * g.D * g.H * g.W;
  a.N = (int)cin;
  a.K = S * go.C;
  a.A = bptr(dout);
  a.B = bptr(wd);
  a.dims = g.dims; a.Nimg = g.N; a.D = g.D; a.H = g.H; a.W = g.W;
  a.Cin = (int)cin; a.Cout = go.C;
  TORCH_CHECK(go.C % 32 == 0, "convT dgrad needs Cout % 32 == 0");
  TORCH_CHECK((int64_t)a.M * (g.dims == 2 ? 4 : 8) < (int64_t)INT32_MAX, "convT: too many pixels for 32-bit pixel indices");
  at::Tensor dx = at::empty(shape_with_c(g, (int)cin), dout.options());
  a.C = dx.data_ptr();
  at::Tensor bnpart = at::empty({0}, dout.options().dtype(at::kFloat));
  a.bn4 = bn4_ptr(bn4, (int)cin);
  if (a.bn4 != nullptr) {
    TORCH_CHECK(has(bny) && bny->is_contiguous() &&
                bny->numel() == dx.numel() && bny->scalar_type() == at::kBFloat16,
                "convt_dgrad: bny must be the deferred pre-BN input (shape of dx, bf16)");
    a.bny = bptr(*bny);
  }
  const int res_rows = convt_res_rows(a, num_cus());
  if (a.bn4 != nullptr) {
    // one fully written row per workgroup: the resident-weight kernel's persistent
    // workgroups, or the GEMM fallback's tiles (each writes its full-width row, zeros
    // outside its channel tile) — no zero-fill pass
    const long long grid = res_rows > 0 ? res_rows : gemm_nt_grid(a);
    bnpart = at::empty({(int64_t)grid, 2, (int64_t)cin}, dout.options().dtype(at::kFloat));
    a.bnpart = bnpart.data_ptr<float>();
  }
  const bool res = res_rows != 0 && convt_res_launch(a, num_cus(), cur_stream());
  if (!res) gemm_launch(a, cur_stream());
  set_last_path(res ? "convt_dgrad:res" : "convt_dgrad:gemm");
  return {dx, bnpart};
}

// bias gradient of a transposed conv: per-channel sum of dOut.  When dOut came out of a
// conv3 data-gradient epilogue, its per-workgroup channel sums are already there (rows
// [R][2][Ctot], sum part first): reduce those instead of re-reading dOut.
static at::Tensor convt_bias_grad(const at::Tensor& x, const at::Tensor& dout, const Geo& go,
                                  const c10::optional<at::Tensor>& colsum_rows,
                                  const c10::optional<at::Tensor>& db_out, bool into) {
  auto fopts = x.options().dtype(at::kFloat);
  at::Tensor db = into ? *db_out : at::empty({go.C}, fopts);
  if (has(colsum_rows) && colsum_rows->numel() > 0) {
    const at::Tensor& cr = *colsum_rows;
    TORCH_CHECK(cr.dim() == 3 && cr.size(1) == 2 && cr.size(2) >= go.C, "colsum rows [R][2][C]");
    sum_slab(cr, (int)cr.size(0), go.C, db, 2, 0, 0, 0, into, 2 * cr.size(2));
  } else {
    const long long P = (long long)go.N * go.D * go.H * go.W;
    const int nb = (int)std::max<long long>(1, std::min<long long>((P + 1023) / 1024, 1024));
    at::Tensor cpart = at::empty({nb, go.C}, fopts);
    channel_sum_launch(bptr(dout), P, go.C, cpart.data_ptr<float>(), nb, cur_stream());
    sum_slab(cpart, nb, go.C, db, 2, 0, 0, 0, into);
  }
  return db;
}

// weight (+ bias) gradient of a transposed conv: {dW, db} (accumulated into the outs when
// given, empty then)
std::vector<at::Tensor> convt_wgrad(const at::Tensor& x, const at::Tensor& dout,
                                    const c10::optional<at::Tensor>& dw_out,
                                    const c10::optional<at::Tensor>& db_out,
                                    const c10::optional<at::Tensor>& colsum_rows,
                                    const c10::optional<at::Tensor>& bn4) {
  CHECK_DEV(x); CHECK_CONTIG(x); CHECK_CONTIG(dout);
  c10::DeviceGuard guard(x.device());
  const Geo g = geo_of(x);
  const Geo go = geo_of(dout);
  const int S = g.dims == 2 ? 4 : 8;
  GemmArgs a{};
  a.mode = GEMM_CONVT_WGRAD;
  a.M = g.C;
  a.N = S * go.C;
  a.K = g.N * g.D * g.H * g.W;
  a.A = bptr(x);
  a.B = bptr(dout);
  a.dims = g.dims; a.Nimg = g.N; a.D = g.D; a.H = g.H; a.W = g.W;
  a.Cin = g.C; a.Cout = go.C;
  a.bn4 = bn4_ptr(bn4, g.C);
  const char* path = convt_wgrad_plan(a, num_cus());
  auto fopts = x.options().dtype(at::kFloat);
  const long long NW = (long long)a.M * a.N;
  at::Tensor part = at::empty({(int64_t)a.splits * NW}, fopts);
  a.partial = part.data_ptr<float>();
  std::vector<int64_t> ws = {g.C, go.C, 2, 2};
  if (g.dims == 3) ws.push_back(2);
  const bool into = has(dw_out);
  at::Tensor dW = into ? *dw_out : at::empty(ws, fopts);
  set_last_path(path);
  gemm_launch(a, cur_stream());
  sum_slab(part, a.splits, NW, dW, 1, g.C, S, go.C, into);
  at::Tensor db = convt_bias_grad(x, dout, go, colsum_rows, db_out, into);
  if (into) return {at::empty({0}, fopts), at::empty({0}, fopts)};
  return {dW, db};
}

// Fused data + weight gradient of a 2-D 64 -> 64-channel transposed conv (dOut read once):
// returns {dx, bnpart (deferred BN of x: [R][2][64] rows, else empty), dW, db} (dW / db
// accumulated into the outs when given, empty then).  Other shapes: the separate kernels.
std::vector<at::Tensor> convt_bwd_fused(const at::Tensor& x, const at::Tensor& dout, const at::Tensor& wd,
                                        const c10::optional<at::Tensor>& dw_out,
                                        const c10::optional<at::Tensor>& db_out,
                                        const c10::optional<at::Tensor>& colsum_rows,
                                        const c10::optional<at::Tensor>& bn4) {
  CHECK_DEV(x); CHECK_CONTIG(x); CHECK_BF16(x); CHECK_CONTIG(dout); CHECK_BF16(dout);
  CHECK_BF16(wd); CHECK_CONTIG(wd);
  c10::DeviceGuard guard(x.device());
  const bool into = has(dw_out);
  auto fopts = x.options().dtype(at::kFloat);
  if (!convt_bwd_fused_ok(x.sizes().data(), (int)x.dim(), dout.sizes().data(), (int)dout.dim(), num_cus())) {
    auto r = convt_dgrad(dout, wd, x.size(3), has(bn4) ? c10::optional<at::Tensor>(x) : c10::nullopt, bn4);
    auto w = convt_wgrad(x, dout, dw_out, db_out, colsum_rows, bn4);
    set_last_path("convt_bwd_fused:separate");
    return {r[0], r[1], w[0], w[1]};
  }
  TORCH_CHECK(wd.numel() == 64 * 256, "convt_bwd_fused: packed dgrad weights must be [64][256]");
  const Geo g = geo_of(x);
  const Geo go = geo_of(dout);
  GemmArgs a{};
  a.mode = GEMM_CONVT_WGRAD;
  a.M = 64; a.N = 256;
  a.K = g.N * g.H * g.W;
  a.A = bptr(x);
  a.B = bptr(dout);
  a.Wd2 = bptr(wd);
  a.dims = 2; a.Nimg = g.N; a.D = 1; a.H = g.H; a.W = g.W;
  a.Cin = 64; a.Cout = 64;
  a.bn4 = bn4_ptr(bn4, 64);
  a.splits = convt_bwd_fused_splits(a.K, num_cus());
  at::Tensor dx = at::empty_like(x);
  a.C = dx.data_ptr();
  const long long NW = 64LL * 256;
  at::Tensor part = at::empty({(int64_t)a.splits * NW}, fopts);
  a.partial = part.data_ptr<float>();
  at::Tensor bnpart = at::empty({a.bn4 != nullptr ? (int64_t)a.splits : 0, 2, 64}, fopts);
  if (a.bn4 != nullptr) a.bnpart = bnpart.data_ptr<float>();
  at::Tensor dW = into ? *dw_out : at::empty({64, 64, 2, 2}, fopts);
  set_last_path("convt_bwd_fused:fused");
  convt_bwd_fused_launch(a, cur_stream());
  sum_slab(part, a.splits, NW, dW, 1, 64, 4, 64, into);
  at::Tensor db = convt_bias_grad(x, dout, go, colsum_rows, db_out, into);
  if (into) return {dx, bnpart, at::empty({0}, fopts), at::empty({0}, fopts)};
  return {dx, bnpart, dW, db};
}

// ------------------------------------------------------------------------ head + CE
// the kernel family of the head's backward-side launches (head_ce.hip: every C = 32 head with
// a supported class count runs the MFMA head32 kernels, the other widths the channel-split ones)
static const char* head_variant(int C) { return C == 32 ? "head32" : "split"; }

// class_weight (optional): fp32 [K] on a's device — cross_entropy(weight=): a valid pixel
// carries w[label], out3[2] is the weight sum of the valid pixels (the count without weights)
// and loss and gradients are normalised by it; hits stay unweighted; a zero sum gives loss 0
// and zero gradients (PyTorch: NaN).  The passes of one backward must be given the same tensor.
static const float* class_weight_ptr(const c10::optional<at::Tensor>& cw, const at::Tensor& a, int K) {
  if (!has(cw)) return nullptr;
  CHECK_F32(*cw); CHECK_CONTIG(*cw);
  TORCH_CHECK(cw->dim() == 1 && cw->numel() == K && cw->device() == a.device(),
              "class_weight must be fp32 [K] on the activation's device");
  return cw->data_ptr<float>();
}

at::Tensor head_ce_fwd(const at::Tensor& a, const at::Tensor& Wh, const at::Tensor& bh,
                       const at::Tensor& labels, int64_t ignore_index,
                       const c10::optional<at::Tensor>& bn4,
                       const c10::optional<at::Tensor>& class_weight) {
  CHECK_DEV(a); CHECK_CONTIG(a); CHECK_BF16(a); CHECK_F32(Wh); CHECK_CONTIG(Wh);
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.is_contiguous(), "labels must be int64");
  c10::DeviceGuard guard(a.device());
  const int C = (int)a.size(-1), K = (int)Wh.size(0);
  TORCH_CHECK(head_supported(C, K), "head kernel: unsupported (C, K)");
  const long long P = a.numel() / C;
  TORCH_CHECK(labels.numel() == P, "labels size mismatch");
  const int nb = (int)std::max<long long>(1, std::min<long long>((P + 255) / 256, 2048));
  auto fopts = a.options().dtype(at::kFloat);
  at::Tensor partial = at::empty({nb, 3}, fopts);
  at::Tensor out3 = at::empty({3}, fopts);
  head_ce_fwd_launch(bptr(a), Wh.data_ptr<float>(), bh.data_ptr<float>(), labels.data_ptr<int64_t>(),
                     partial.data_ptr<float>(), out3.data_ptr<float>(), bn4_ptr(bn4, C), nb, P, C, K,
                     (int)ignore_index, cur_stream(), class_weight_ptr(class_weight, a, K));
  set_last_path(std::string("head_ce_fwd:split") + (bn4_ptr(bn4, C) != nullptr ? ":defer" : ""));
  return out3;
}

std::vector<at::Tensor> head_ce_bwd(const at::Tensor& a, const at::Tensor& Wh, const at::Tensor& bh,
                                    const at::Tensor& labels, const at::Tensor& out3,
                                    const c10::optional<at::Tensor>& gscale, int64_t ignore_index,
                                    const c10::optional<at::Tensor>& dw_out,
                                    const c10::optional<at::Tensor>& db_out,
                                    const c10::optional<at::Tensor>& bn4, bool store_da,
                                    const c10::optional<at::Tensor>& class_weight) {
  CHECK_DEV(a); CHECK_CONTIG(a);
  c10::DeviceGuard guard(a.device());
  const int C = (int)a.size(-1), K = (int)Wh.size(0);
  const float* pbn = bn4_ptr(bn4, C);
  TORCH_CHECK(head_supported(C, K), "head kernel: unsupported (C, K)");
  TORCH_CHECK(store_da || pbn != nullptr, "head_ce_bwd: store_da=False needs the deferred BN (bn4)");
  const long long P = a.numel() / C;
  const int nb = head_ce_bwd_blocks(C, K, P, num_cus());
  auto fopts = a.options().dtype(at::kFloat);
  // store_da=False: the stats pass of the two-pass backward (head_ce_bn_bwd writes dY)
  at::Tensor dA = store_da ? at::empty_like(a) : at::empty({0}, a.options());
  at::Tensor part = at::empty({nb, K * C + K}, fopts);
  // deferred BatchNorm input: the kernel also emits that BN's backward partial rows
  at::Tensor bnpart = pbn != nullptr ? at::empty({nb, 2, C}, fopts) : at::empty({0}, fopts);
  head_ce_bwd_launch(bptr(a), Wh.data_ptr<float>(), bh.data_ptr<float>(), labels.data_ptr<int64_t>(),
                     fptr_opt(gscale), out3.data_ptr<float>(), store_da ? bptr_mut(dA) : nullptr,
                     part.data_ptr<float>(), nb, P, C, K, (int)ignore_index, pbn,
                     pbn != nullptr ? bnpart.data_ptr<float>() : nullptr, cur_stream(),
                     class_weight_ptr(class_weight, a, K));
  set_last_path(std::string("head_ce_bwd:") + head_variant(C) + (pbn != nullptr ? ":defer" : "") +
                (store_da ? "" : ":stats"));
  const bool into = has(dw_out);
  at::Tensor sums = reduce_rows(part, nb, K * C + K);   // rows are [dW (K*C) | db (K)]
  if (into) {
    TORCH_CHECK(dw_out->is_contiguous() && db_out->is_contiguous(), "grad outs must be contiguous");
    scatter_sums_launch(sums.data_ptr<double>(), K * C, dw_out->data_ptr<float>(), 2, 0, 0, 0, 1.f,
                        true, cur_stream());
    scatter_sums_launch(sums.data_ptr<double>() + K * C, K, db_out->data_ptr<float>(), 2, 0, 0, 0,
                        1.f, true, cur_stream());
    at::Tensor none = at::empty({0}, fopts);
    return {dA, none, none, bnpart};
  }
  at::Tensor red = at::empty({K * C + K}, fopts);
  scatter_sums_launch(sums.data_ptr<double>(), K * C + K, red.data_ptr<float>(), 2, 0, 0, 0, 1.f,
                      false, cur_stream());
  at::Tensor dW = red.narrow(0, 0, K * C).view({K, C});
  at::Tensor db = red.narrow(0, K * C, K);
  return {dA, dW, db, bnpart};
}

// Second pass of the two-pass head backward: the last decoder block's BatchNorm backward
// applied to the recomputed head gradient.  partial: the stats pass's [R][2][C] rows;
// returns {dY, dgamma, dbeta} like bn_backward (accumulated into the outs when given)
std::vector<at::Tensor> head_ce_bn_bwd(const at::Tensor& a, const at::Tensor& Wh, const at::Tensor& bh,
                                       const at::Tensor& labels, const at::Tensor& out3,
                                       const c10::optional<at::Tensor>& gscale, int64_t ignore_index,
                                       const at::Tensor& bn4, const at::Tensor& partial,
                                       const at::Tensor& gamma,
                                       const c10::optional<at::Tensor>& dgamma_out,
                                       const c10::optional<at::Tensor>& dbeta_out,
                                       const c10::optional<at::Tensor>& pscale, int64_t groups,
                                       const c10::optional<at::Tensor>& class_weight) {
  CHECK_DEV(a); CHECK_CONTIG(a); CHECK_BF16(a);
  // pscale: device factor on the partial rows (rows from the fused forward at unit scale)
  const float* ps = fptr_opt(pscale);
  c10::DeviceGuard guard(a.device());
  const int C = (int)a.size(-1), K = (int)Wh.size(0);
  const float* pcw = class_weight_ptr(class_weight, a, K);
  if (groups > 1) {
    // BN groups (a batched window): bn4 [groups][4][C], partial rows group-major (the fused
    // forward's head_ce_fwd_stats with groups), per-group coefficients
    const long long P = a.numel() / C;
    TORCH_CHECK(C == 32 && K <= 16 && P % (groups * 16) == 0,
                "head_ce_bn_bwd groups: C = 32 head, pixels per group a multiple of 16");
    CHECK_F32(bn4); CHECK_CONTIG(bn4); CHECK_F32(partial); CHECK_CONTIG(partial); CHECK_F32(gamma);
    TORCH_CHECK(bn4.numel() == groups * 4 * C && partial.numel() % (groups * 2 * C) == 0,
                "head_ce_bn_bwd groups: bn4 [groups][4][C], partial [groups * R][2][C]");
    auto fopts = a.options().dtype(at::kFloat);
    const bool into = has(dgamma_out);
    at::Tensor dgamma = into ? *dgamma_out : at::empty({C}, fopts);
    at::Tensor dbeta = into ? *dbeta_out : at::empty({C}, fopts);
    at::Tensor coefs = at::empty({groups, 3, C}, fopts);
    at::Tensor gsum = at::empty({groups, 2, C}, a.options().dtype(at::kDouble));
    const int nb = (int)(partial.numel() / (groups * 2 * C));
    bn_group_grad_rows_launch(partial.data_ptr<float>(), nb, (int)groups, C, (double)(P / groups),
                              gamma.data_ptr<float>(), bn4.data_ptr<float>(), dgamma.data_ptr<float>(),
                              dbeta.data_ptr<float>(), into, coefs.data_ptr<float>(),
                              gsum.data_ptr<double>(), ps, cur_stream());
    at::Tensor dY = at::empty_like(a);
    head_bn_apply_launch(bptr(a), Wh.data_ptr<float>(), bh.data_ptr<float>(), labels.data_ptr<int64_t>(),
                         fptr_opt(gscale), out3.data_ptr<float>(), bn4.data_ptr<float>(),
                         coefs.data_ptr<float>(), bptr_mut(dY), P, C, K, (int)ignore_index, num_cus(),
                         cur_stream(), (int)groups, pcw);
    set_last_path("head_ce_bn_bwd:head32:groups");
    return {dY, dgamma, dbeta};
  }
  const float* pbn = bn4_ptr(bn4, C);
  TORCH_CHECK(head_supported(C, K), "head kernel: unsupported (C, K)");
  CHECK_F32(partial); CHECK_CONTIG(partial); CHECK_F32(gamma);
  TORCH_CHECK(partial.numel() % (2 * C) == 0 && partial.numel() > 0, "partial rows must be [R][2][C]");
  const long long P = a.numel() / C;
  const int nb = (int)(partial.numel() / (2 * C));
  const BnGrad r = bn_grad_from_rows(partial, nb, C, (double)P, gamma, pbn + C, dgamma_out, dbeta_out, ps);
  at::Tensor dY = at::empty_like(a);
  head_bn_apply_launch(bptr(a), Wh.data_ptr<float>(), bh.data_ptr<float>(), labels.data_ptr<int64_t>(),
                       fptr_opt(gscale), out3.data_ptr<float>(), pbn, r.coefs.data_ptr<float>(),
                       bptr_mut(dY), P, C, K, (int)ignore_index, num_cus(), cur_stream(), 1, pcw);
  set_last_path(std::string("head_ce_bn_bwd:") + head_variant(C));
  return {dY, r.dgamma, r.dbeta};
}

// Training forward of the head with the deferred BatchNorm, fused with the backward's
// statistics pass at a unit gradient scale: returns {out3 = (loss, correct, count),
// dW rows [R][K*C + K], BN partial rows [R][2][C]}.  The backward scales the reductions by
// dL/count on the device (head_wgrad_from_rows, head_ce_bn_bwd pscale).
std::vector<at::Tensor> head_ce_fwd_stats(const at::Tensor& a, const at::Tensor& Wh,
                                          const at::Tensor& bh, const at::Tensor& labels,
                                          int64_t ignore_index, const at::Tensor& bn4,
                                          int64_t groups,
                                          const c10::optional<at::Tensor>& class_weight) {
  CHECK_DEV(a); CHECK_CONTIG(a); CHECK_BF16(a); CHECK_CONTIG(labels);
  TORCH_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
  c10::DeviceGuard guard(a.device());
  const int C = (int)a.size(-1), K = (int)Wh.size(0);
  const long long P = a.numel() / C;
  const float* pbn = nullptr;
  if (groups > 1) {
    // BN groups: per-group statistics bn4 [groups][4][C], group-major rows (C = 32 kernel)
    CHECK_F32(bn4); CHECK_CONTIG(bn4);
    TORCH_CHECK(C == 32 && K <= 16 && P % (groups * 16) == 0 && bn4.numel() == groups * 4 * C,
                "head_ce_fwd_stats groups: C = 32 head, bn4 [groups][4][C], pixels per group a "
                "multiple of 16");
    pbn = bn4.data_ptr<float>();
  } else {
    pbn = bn4_ptr(bn4, C);
  }
  TORCH_CHECK(head_supported(C, K), "head kernel: unsupported (C, K)");
  TORCH_CHECK(labels.numel() == P, "labels / activation pixel count mismatch");
  const int nb = head_fwd_stats_blocks(C, K, P, num_cus(), groups > 1 ? (int)groups : 1);
  auto fopts = a.options().dtype(at::kFloat);
  at::Tensor wrows = at::empty({nb, K * C + K}, fopts);
  at::Tensor brows = at::empty({nb, 2, C}, fopts);
  at::Tensor lrows = at::empty({nb, 3}, fopts);
  at::Tensor out3 = at::empty({3}, fopts);
  head_ce_fwd_stats_launch(bptr(a), Wh.data_ptr<float>(), bh.data_ptr<float>(), labels.data_ptr<int64_t>(),
                           pbn, wrows.data_ptr<float>(), brows.data_ptr<float>(), lrows.data_ptr<float>(),
                           out3.data_ptr<float>(), nb, P, C, K, (int)ignore_index, cur_stream(),
                           groups > 1 ? (int)groups : 1, class_weight_ptr(class_weight, a, K));
  set_last_path(std::string("head_ce_fwd_stats:") + head_variant(C) + (groups > 1 ? ":groups" : ""));
  return {out3, wrows, brows};
}

// dWh, dbh from the fused forward's rows: deterministic fp64 row sums times a device scale
std::vector<at::Tensor> head_wgrad_from_rows(const at::Tensor& rows, const at::Tensor& scale, int64_t K,
                                             int64_t C, const c10::optional<at::Tensor>& dw_out,
                                             const c10::optional<at::Tensor>& db_out) {
  CHECK_F32(rows); CHECK_CONTIG(rows); CHECK_F32(scale);
  c10::DeviceGuard guard(rows.device());
  TORCH_CHECK(rows.dim() == 2 && rows.size(1) == K * C + K, "rows must be [R][K*C + K]");
  const int R = (int)rows.size(0);
  at::Tensor sums = reduce_rows(rows, R, K * C + K);
  auto fopts = rows.options();
  const bool into = has(dw_out);
  if (into) {
    TORCH_CHECK(dw_out->is_contiguous() && db_out->is_contiguous(), "grad outs must be contiguous");
    if (db_out->data_ptr<float>() == dw_out->data_ptr<float>() + K * C) {
      // adjacent in the flat gradient buffer (weight then bias): one launch
      scatter_sums_dscale_launch(sums.data_ptr<double>(), K * C + K, dw_out->data_ptr<float>(),
                                 scale.data_ptr<float>(), true, cur_stream());
    } else {
      scatter_sums_dscale_launch(sums.data_ptr<double>(), K * C, dw_out->data_ptr<float>(),
                                 scale.data_ptr<float>(), true, cur_stream());
      scatter_sums_dscale_launch(sums.data_ptr<double>() + K * C, K, db_out->data_ptr<float>(),
                                 scale.data_ptr<float>(), true, cur_stream());
    }
    return {at::empty({0}, fopts), at::empty({0}, fopts)};
  }
  at::Tensor red = at::empty({K * C + K}, fopts);
  scatter_sums_dscale_launch(sums.data_ptr<double>(), K * C + K, red.data_ptr<float>(),
                             scale.data_ptr<float>(), false, cur_stream());
  return {red.narrow(0, 0, K * C).view({K, C}), red.narrow(0, K * C, K)};
}

// dL/count as a device scalar from the loss kernel's out3 = (loss, correct, count) and the
// incoming dL (absent: 1)
at::Tensor head_grad_scale(const at::Tensor& out3, const c10::optional<at::Tensor>& gs) {
  CHECK_F32(out3); CHECK_CONTIG(out3);
  TORCH_CHECK(out3.numel() >= 3, "out3 must hold (loss, correct, count)");
  c10::DeviceGuard guard(out3.device());
  const float* pg = nullptr;
  if (has(gs)) {
    CHECK_F32(*gs); CHECK_CONTIG(*gs);
    TORCH_CHECK(gs->numel() == 1 && gs->device() == out3.device(), "gs must be one float on out3's device");
    pg = gs->data_ptr<float>();
  }
  at::Tensor scale = at::empty({1}, out3.options());
  head_grad_scale_launch(out3.data_ptr<float>(), pg, scale.data_ptr<float>(), cur_stream());
  return scale;
}

// DeviceMeter accumulation in one launch (buf: 4 doubles; loss / correct: one float each)
void meter_add(at::Tensor& buf, const at::Tensor& loss, const at::Tensor& correct, double pixels,
               double count) {
  TORCH_CHECK(buf.scalar_type() == at::kDouble && buf.numel() == 4 && buf.is_contiguous(),
              "meter buffer must be 4 contiguous doubles");
  CHECK_F32(loss); CHECK_F32(correct);
  TORCH_CHECK(loss.numel() == 1 && correct.numel() == 1, "loss / correct must be scalars");
  TORCH_CHECK(loss.device() == buf.device() && correct.device() == buf.device(), "device mismatch");
  c10::DeviceGuard guard(buf.device());
  meter_add_launch(buf.data_ptr<double>(), loss.data_ptr<float>(), correct.data_ptr<float>(), pixels,
                   count, cur_stream());
}

at::Tensor head_logits(const at::Tensor& a, const at::Tensor& Wh, const at::Tensor& bh,
                       const c10::optional<at::Tensor>& bn4) {
  CHECK_DEV(a); CHECK_CONTIG(a);
  c10::DeviceGuard guard(a.device());
  const Geo g = geo_of(a);
  const int C = g.C, K = (int)Wh.size(0);
  TORCH_CHECK(head_supported(C, K), "head kernel: unsupported (C, K)");
  const long long HW = (long long)g.D * g.H * g.W;
  std::vector<int64_t> os = g.dims == 2 ? std::vector<int64_t>{g.N, K, g.H, g.W}
                                        : std::vector<int64_t>{g.N, K, g.D, g.H, g.W};
  at::Tensor out = at::empty(os, a.options().dtype(at::kFloat));
  head_logits_launch(bptr(a), Wh.data_ptr<float>(), bh.data_ptr<float>(), out.data_ptr<float>(),
                     (long long)g.N * HW, HW, C, K, bn4_ptr(bn4, C), cur_stream());
  set_last_path(std::string("head_logits") + (bn4_ptr(bn4, C) != nullptr ? ":defer" : ""));
  return out;
}

// ------------------------------------------------------------------------ optimizer / pack
// the flat buffers of one Adam step: fp32, contiguous (the kernel walks raw pointers), one device
namespace {
void check_adam_buffers(const at::Tensor& p, const at::Tensor& g, const at::Tensor& m,
                        const at::Tensor& v) {
  CHECK_DEV(p); CHECK_F32(p); CHECK_F32(g); CHECK_F32(m); CHECK_F32(v);
  CHECK_CONTIG(p); CHECK_CONTIG(g); CHECK_CONTIG(m); CHECK_CONTIG(v);
  TORCH_CHECK(g.device() == p.device() && m.device() == p.device() && v.device() == p.device(),
              "adam: p, g, m, v must be on one device");
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(), "size");
}
}  // namespace

void adam_step(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v, double b1, double b2,
               double eps, double wd, double step_size, double inv_sqrt_bc2) {
  check_adam_buffers(p, g, m, v);
  if (p.numel() == 0) return;
  c10::DeviceGuard guard(p.device());
  adam_launch(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
              p.numel(), (float)b1, (float)b2, (float)eps, (float)wd, (float)step_size,
              (float)inv_sqrt_bc2, cur_stream());
}

// graph-capturable step: scal = device float[3] (t, step_size, inv_sqrt_bc2), advanced on
// the device by this call
void adam_step_dev(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v, at::Tensor scal,
                   double lr, double b1, double b2, double eps, double wd) {
  check_adam_buffers(p, g, m, v);
  CHECK_F32(scal);
  TORCH_CHECK(scal.numel() >= 3 && scal.is_contiguous() && scal.device() == p.device(),
              "scal must be float[3] on p's device");
  c10::DeviceGuard guard(p.device());
  adam_scalars_launch(scal.data_ptr<float>(), lr, b1, b2, cur_stream());
  if (p.numel() == 0) return;           // (the step counter advances, as on the CPU)
  adam_launch(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
              p.numel(), (float)b1, (float)b2, (float)eps, (float)wd, 0.f, 1.f, cur_stream(),
              scal.data_ptr<float>());
}

// graph-capturable step with a learning-rate schedule, gradient-norm clipping and coupled or
// decoupled weight decay (optim.hip): scal = device float[8] (the table of optim_math.h,
// scal[0] = steps taken, advanced here), partial = device double[>= grad_sqnorm_blocks(n)]
void adam_step_sched(at::Tensor p, const at::Tensor& g, at::Tensor m, at::Tensor v, at::Tensor scal,
                     at::Tensor partial, double lr, double b1, double b2, double eps, double wd,
                     bool decoupled, double max_norm, int64_t sched_kind, int64_t warmup,
                     int64_t total, double lr_min, double power) {
  check_adam_buffers(p, g, m, v);
  CHECK_F32(scal);
  TORCH_CHECK(scal.numel() == 8 && scal.is_contiguous() && scal.device() == p.device(),
              "scal must be float[8] on p's device");
  const long long n = p.numel();
  TORCH_CHECK(partial.scalar_type() == at::kDouble && partial.is_contiguous() &&
                  partial.device() == p.device() && partial.numel() >= grad_sqnorm_blocks(n),
              "partial must be double[>= grad_sqnorm_blocks(n)] on p's device");
  TORCH_CHECK(sched_kind >= 0 && sched_kind <= 2, "sched_kind: 0 constant, 1 poly, 2 cosine");
  TORCH_CHECK(warmup >= 0 && total >= 0, "warmup and total must be >= 0");
  c10::DeviceGuard guard(p.device());
  SchedArgs a{lr, b1, b2, wd, max_norm, lr_min, power, warmup, total, (int)sched_kind,
              decoupled ? 1 : 0};
  const int nb = max_norm > 0.0 ? grad_sqnorm_blocks(n) : 0;
  if (nb > 0) grad_sqnorm_launch(g.data_ptr<float>(), n, partial.data_ptr<double>(), cur_stream());
  sched_scalars_launch(scal.data_ptr<float>(), partial.data_ptr<double>(), nb, a, cur_stream());
  if (n == 0) return;                   // (the step counter advances, as in adam_step_dev)
  adam_sched_launch(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                    v.data_ptr<float>(), n, (float)b1, (float)b2, (float)eps, (float)wd, decoupled,
                    scal.data_ptr<float>(), cur_stream());
}

void weight_pack(const at::Tensor& entries, int64_t n, int64_t max_elems) {
  CHECK_DEV(entries); CHECK_CONTIG(entries);
  TORCH_CHECK(entries.scalar_type() == at::kLong && n >= 0 && entries.numel() == n * 6,
              "entries must be int64 [n, 6] (48-byte PackEntry records)");
  static_assert(sizeof(PackEntry) == 48, "PackEntry layout");
  if (n == 0) return;                   // (a grid of zero entries is no launch)
  c10::DeviceGuard guard(entries.device());
  weight_pack_launch(reinterpret_cast<const PackEntry*>(entries.data_ptr()), (int)n, max_elems,
                     cur_stream());
}

// ------------------------------------------------------------------------ codec
namespace {
// the flat fp32 buffer of a codec call and its segment table: int64 (start, end) pairs on the
// buffer's device -> the number of segments
int check_codec_segments(const at::Tensor& x, const at::Tensor& seg) {
  CHECK_DEV(x); CHECK_F32(x); CHECK_CONTIG(x); CHECK_CONTIG(seg);
  TORCH_CHECK(seg.scalar_type() == at::kLong && seg.device() == x.device() && seg.numel() % 2 == 0,
              "seg must be int64 (start, end) pairs on the buffer's device");
  return (int)(seg.numel() / 2);
}
void check_codec_id(int64_t codec) {
  TORCH_CHECK(codec == 0 || codec == 1, "codec must be 0 (fp16_absmax) or 1 (int8_absmax)");
}
}  // namespace

at::Tensor codec_absmax(const at::Tensor& x, const at::Tensor& seg) {
  const int nseg = check_codec_segments(x, seg);
  c10::DeviceGuard guard(x.device());
  at::Tensor s = at::empty({nseg}, x.options());
  if (nseg == 0) return s;
  codec_absmax_launch(x.data_ptr<float>(), seg.data_ptr<int64_t>(), nseg, s.data_ptr<float>(),
                      cur_stream());
  return s;
}

at::Tensor codec_encode(const at::Tensor& x, const at::Tensor& seg, const at::Tensor& scales,
                        int64_t codec) {
  const int nseg = check_codec_segments(x, seg);
  check_codec_id(codec);
  CHECK_F32(scales); CHECK_CONTIG(scales);
  TORCH_CHECK(scales.device() == x.device() && scales.numel() == nseg,
              "scales must be fp32 [nseg] on the buffer's device");
  c10::DeviceGuard guard(x.device());
  at::Tensor out = at::zeros({x.numel()}, x.options().dtype(codec == 0 ? at::kHalf : at::kChar));
  if (nseg == 0 || x.numel() == 0) return out;
  codec_encode_launch(x.data_ptr<float>(), seg.data_ptr<int64_t>(), nseg, scales.data_ptr<float>(),
                      out.data_ptr(), (int)codec, x.numel(), cur_stream());
  return out;
}

void codec_decode_sum(at::Tensor out, const at::Tensor& q, const at::Tensor& scales,
                      const at::Tensor& w, const at::Tensor& seg, int64_t codec) {
  const int nseg = check_codec_segments(out, seg);
  check_codec_id(codec);
  CHECK_CONTIG(q); CHECK_F32(scales); CHECK_CONTIG(scales); CHECK_F32(w); CHECK_CONTIG(w);
  TORCH_CHECK(q.dim() >= 1 && q.device() == out.device() &&
              q.scalar_type() == (codec == 0 ? at::kHalf : at::kChar),
              "q must be the codec's wire dtype (fp16 / int8) [world][n] on out's device");
  const int world = (int)q.size(0);
  TORCH_CHECK(q.numel() == (int64_t)world * out.numel(), "q must hold world x out.numel() elements");
  TORCH_CHECK(scales.device() == out.device() && scales.numel() == (int64_t)world * nseg,
              "scales must be fp32 [world][nseg] on out's device");
  TORCH_CHECK(w.device() == out.device() && w.numel() == world, "w must be fp32 [world] on out's device");
  if (nseg == 0 || out.numel() == 0) return;
  c10::DeviceGuard guard(out.device());
  codec_decode_sum_launch(out.data_ptr<float>(), q.data_ptr(), scales.data_ptr<float>(),
                          w.data_ptr<float>(), seg.data_ptr<int64_t>(), nseg, world, (int)codec,
                          out.numel(), cur_stream());
}

// ------------------------------------------------------------------------ misc
at::Tensor bilinear_up2(const at::Tensor& x) {
  CHECK_DEV(x); CHECK_CONTIG(x); CHECK_BF16(x);
  c10::DeviceGuard guard(x.device());
  const Geo g = geo_of(x);
  at::Tensor y = at::empty(shape_with_c(g, g.C, 2), x.options());
  bilinear_up2_launch(bptr(x), bptr_mut(y), g.dims, g.N, g.D, g.H, g.W, g.C, false, cur_stream());
  return y;
}

at::Tensor bilinear_up2_bwd(const at::Tensor& dy) {
  CHECK_DEV(dy); CHECK_CONTIG(dy); CHECK_BF16(dy);
  c10::DeviceGuard guard(dy.device());
  Geo g = geo_of(dy);
  g.H /= 2; g.W /= 2; if (g.dims == 3) g.D /= 2;
  at::Tensor dx = at::empty(shape_with_c(g, g.C), dy.options());
  at::Tensor tmp = at::empty({dx.numel()}, dy.options().dtype(at::kFloat));
  bilinear_up2_bwd_launch(bptr(dy), tmp.data_ptr<float>(), bptr_mut(dx), g.dims, g.N, g.D, g.H,
                          g.W, g.C, cur_stream());
  return dx;
}

// NCHW / NCDHW tensor (fp32 or bf16; contiguous or channels_last memory) -> channel-last bf16
// [N, (D,) H, W, Cp] with channels zero-padded to a multiple of `cpad`
at::Tensor to_nhwc_bf16(const at::Tensor& x, int64_t cpad) {
  CHECK_DEV(x);
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "fp32/bf16 input");
  TORCH_CHECK((x.dim() == 4 || x.dim() == 5) && cpad >= 1, "to_nhwc_bf16: [N, C, (D,) H, W] input, cpad >= 1");
  c10::DeviceGuard guard(x.device());
  const int N = (int)x.size(0), C = (int)x.size(1);
  const int Cp = (int)((C + cpad - 1) / cpad * cpad);
  long long S = 1;
  for (int i = 2; i < x.dim(); ++i) S *= x.size(i);
  // supported memory layouts: NCHW-contiguous or channel-last-contiguous
  long long sC, sS;
  if (x.is_contiguous()) { sC = S; sS = 1; }
  else {
    const auto cl = x.dim() == 4 ? at::MemoryFormat::ChannelsLast : at::MemoryFormat::ChannelsLast3d;
    TORCH_CHECK(x.is_contiguous(cl), "input must be contiguous or channels-last");
    sC = 1; sS = C;
  }
  std::vector<int64_t> shape = {N};
  for (int i = 2; i < x.dim(); ++i) shape.push_back(x.size(i));
  shape.push_back(Cp);
  at::Tensor y = at::empty(shape, x.options().dtype(at::kBFloat16));
  if (y.numel() == 0) return y;
  to_nhwc_pad_launch(x.data_ptr(), x.scalar_type() == at::kFloat ? 0 : 1, bptr_mut(y), N, C, Cp, S,
                     x.stride(0), sC, sS, cur_stream());
  return y;
}

// ------------------------------------------------------------------------ input pipeline
std::vector<int64_t> batch_shape(int64_t B, int64_t tile, int64_t dims) {
  std::vector<int64_t> s = {B};
  for (int i = 0; i < dims; ++i) s.push_back(tile);
  return s;
}

// synthetic Vaihingen-shape batch rendered in HBM -> {x [B, (T,) T, T, cpad] bf16, y int64}
std::vector<at::Tensor> synth_tiles(const at::Tensor& idx, int64_t seed, int64_t classes,
                                    int64_t in_ch, int64_t tile, int64_t dims, int64_t grid,
                                    double k, const at::Tensor& palette, int64_t cpad) {
  CHECK_DEV(idx); CHECK_CONTIG(idx); CHECK_DEV(palette); CHECK_CONTIG(palette);
  checks::synth_tiles(idx, classes, in_ch, tile, dims, grid, palette, cpad);
  c10::DeviceGuard guard(idx.device());
  const int64_t B = idx.numel();
  std::vector<int64_t> xs = batch_shape(B, tile, dims);
  at::Tensor y = at::empty(xs, idx.options());
  xs.push_back(cpad);
  at::Tensor x = at::empty(xs, idx.options().dtype(at::kBFloat16));
  if (B > 0)
    synth_tiles_launch(idx.data_ptr<int64_t>(), (int)B, (uint32_t)(seed & 0xffffffff), (int)classes,
                       (int)in_ch, (int)tile, (int)dims, (int)grid, (float)k,
                       palette.data_ptr<float>(), (int)cpad, bptr_mut(x), y.data_ptr<int64_t>(),
                       cur_stream());
  return {x, y};
}

// HBM-resident uint8 dataset [N, (D,) H, W, Cin] + uint8 labels -> gathered bf16 / int64 batch
std::vector<at::Tensor> tile_gather(const at::Tensor& src, const at::Tensor& lab,
                                    const at::Tensor& idx, int64_t cpad) {
  CHECK_DEV(src); CHECK_CONTIG(src); CHECK_DEV(lab); CHECK_CONTIG(lab); CHECK_DEV(idx);
  CHECK_CONTIG(idx);
  checks::tile_gather(src, lab, idx, cpad);
  const int64_t in_ch = src.size(-1);
  c10::DeviceGuard guard(src.device());
  const int64_t B = idx.numel();
  const long long S = lab.numel() / std::max<int64_t>(1, lab.size(0));
  std::vector<int64_t> ys = {B};
  for (int64_t i = 1; i < lab.dim(); ++i) ys.push_back(lab.size(i));
  at::Tensor y = at::empty(ys, idx.options());
  std::vector<int64_t> xs = ys;
  xs.push_back(cpad);
  at::Tensor x = at::empty(xs, src.options().dtype(at::kBFloat16));
  if (B > 0)
    tile_gather_launch(src.data_ptr<uint8_t>(), lab.data_ptr<uint8_t>(), idx.data_ptr<int64_t>(),
                       (int)B, S, (int)in_ch, (int)cpad, (long long)lab.size(0), bptr_mut(x),
                       y.data_ptr<int64_t>(), cur_stream());
  return {x, y};
}

// crop_gather / warp_gather, after checks::*: contiguous device tensors, a grid that fits -> colour
static const float* gather_device_args(const char* op, const at::Tensor& scenes, const at::Tensor& labels,
                                       const at::Tensor& table, const at::Tensor& params,
                                       const c10::optional<at::Tensor>& color, int64_t tile) {
  CHECK_DEV(scenes); CHECK_CONTIG(scenes); CHECK_DEV(labels); CHECK_CONTIG(labels);
  CHECK_DEV(table); CHECK_CONTIG(table); CHECK_DEV(params); CHECK_CONTIG(params);
  if (has(color)) { CHECK_DEV(*color); CHECK_CONTIG(*color); }
  const int64_t nb = crop_gather_blocks((int)tile);
  TORCH_CHECK(params.size(0) * nb * nb < (1LL << 31), op, ": batch too large");
  return fptr_opt(color);
}

// -> tile x tile crops per params (scene, y0, x0, code), mirrored borders, one of the 8
// symmetries of the square: {x bf16 [B, T, T, cpad], y int64}
std::vector<at::Tensor> crop_gather(const at::Tensor& scenes, const at::Tensor& labels,
                                    const at::Tensor& table, const at::Tensor& params,
                                    const c10::optional<at::Tensor>& color, int64_t tile,
                                    int64_t cpad) {
  checks::crop_gather(scenes, labels, table, params, color, tile, cpad);
  const float* pc = gather_device_args("crop_gather", scenes, labels, table, params, color, tile);
  const int64_t in_ch = scenes.size(1), B = params.size(0), n = table.size(0);
  c10::DeviceGuard guard(scenes.device());
  at::Tensor y = at::empty({B, tile, tile}, scenes.options().dtype(at::kLong));
  at::Tensor x = at::empty({B, tile, tile, cpad}, scenes.options().dtype(at::kBFloat16));
  if (B > 0)
    crop_gather_launch(scenes.data_ptr<uint8_t>(), labels.data_ptr<uint8_t>(), table.data_ptr<int64_t>(),
                       (int)n, (long long)labels.size(0), params.data_ptr<int>(), pc, (int)B, (int)in_ch,
                       (int)tile, (int)cpad, knob("CROP_LDS_T", 1) != 0, bptr_mut(x), y.data_ptr<int64_t>(),
                       cur_stream());
  return {x, y};
}

static void params_device_args(const at::Tensor& idx, const at::Tensor& cum, const at::Tensor& table) {
  CHECK_DEV(idx); CHECK_CONTIG(idx); CHECK_DEV(cum); CHECK_CONTIG(cum); CHECK_DEV(table); CHECK_CONTIG(table);
}

// virtual sample numbers -> {params int32 [B, 4], color fp32 [B, 2]} (counter-based: data_math.h)
std::vector<at::Tensor> crop_params(const at::Tensor& idx, const at::Tensor& cum, const at::Tensor& table,
                                    int64_t seed, int64_t tile, int64_t mode, double gain_jitter,
                                    double bias_jitter) {
  checks::params_args("crop_params", idx, cum, table, tile, mode);
  params_device_args(idx, cum, table);
  const int64_t B = idx.numel();
  c10::DeviceGuard guard(idx.device());
  at::Tensor params = at::empty({B, 4}, idx.options().dtype(at::kInt));
  at::Tensor color = at::empty({B, 2}, idx.options().dtype(at::kFloat));
  if (B > 0)
    crop_params_launch(idx.data_ptr<int64_t>(), (int)B, cum.data_ptr<int64_t>(), table.data_ptr<int64_t>(),
                       (int)table.size(0), (uint32_t)(seed & 0xffffffff), (int)tile, (int)mode,
                       (float)gain_jitter, (float)bias_jitter, params.data_ptr<int>(),
                       color.data_ptr<float>(), cur_stream());
  return {params, color};
}

// crop_gather under a zoom and a rotation: wparams int64 [B, 6] of (scene, cy, cx, code, A, Bm)
// rows, 16.16 fixed point (the recipe: data_math.h) -> {x bf16 [B, T, T, cpad], y int64}
std::vector<at::Tensor> warp_gather(const at::Tensor& scenes, const at::Tensor& labels,
                                    const at::Tensor& table, const at::Tensor& wparams,
                                    const c10::optional<at::Tensor>& color, int64_t tile,
                                    int64_t cpad) {
  checks::warp_gather(scenes, labels, table, wparams, color, tile, cpad);
  const float* pc = gather_device_args("warp_gather", scenes, labels, table, wparams, color, tile);
  const int64_t in_ch = scenes.size(1), B = wparams.size(0), n = table.size(0);
  c10::DeviceGuard guard(scenes.device());
  at::Tensor y = at::empty({B, tile, tile}, scenes.options().dtype(at::kLong));
  at::Tensor x = at::empty({B, tile, tile, cpad}, scenes.options().dtype(at::kBFloat16));
  if (B > 0)
    warp_gather_launch(scenes.data_ptr<uint8_t>(), labels.data_ptr<uint8_t>(), table.data_ptr<int64_t>(),
                       (int)n, (long long)labels.size(0), wparams.data_ptr<int64_t>(), pc, (int)B,
                       (int)in_ch, (int)tile, (int)cpad, bptr_mut(x), y.data_ptr<int64_t>(), cur_stream());
  return {x, y};
}

// virtual sample numbers -> {wparams int64 [B, 6], color fp32 [B, 2]}: crop_params with a zoom
// step and a rotation drawn from the int32 tables steps [S] and rot [T, 2] (data_math.h)
std::vector<at::Tensor> warp_params(const at::Tensor& idx, const at::Tensor& cum, const at::Tensor& table,
                                    const at::Tensor& steps, const at::Tensor& rot, int64_t seed,
                                    int64_t tile, int64_t mode, double gain_jitter, double bias_jitter) {
  checks::warp_params(idx, cum, table, steps, rot, tile, mode);
  CHECK_DEV(steps); CHECK_CONTIG(steps); CHECK_DEV(rot); CHECK_CONTIG(rot);
  params_device_args(idx, cum, table);
  const int64_t B = idx.numel();
  c10::DeviceGuard guard(idx.device());
  at::Tensor wparams = at::empty({B, 6}, idx.options().dtype(at::kLong));
  at::Tensor color = at::empty({B, 2}, idx.options().dtype(at::kFloat));
  if (B > 0)
    warp_params_launch(idx.data_ptr<int64_t>(), (int)B, cum.data_ptr<int64_t>(), table.data_ptr<int64_t>(),
                       (int)table.size(0), steps.data_ptr<int>(), (int)steps.size(0), rot.data_ptr<int>(),
                       (int)rot.size(0), (uint32_t)(seed & 0xffffffff), (int)tile, (int)mode,
                       (float)gain_jitter, (float)bias_jitter, wparams.data_ptr<int64_t>(),
                       color.data_ptr<float>(), cur_stream());
  return {wparams, color};
}

// ------------------------------------------------------------------------ scene prediction
// test-time augmentation: the symmetry codes of a call (int32 [S], 1 <= S <= 8, distinct values
// in 0..7; checks::codes) -> S and the codes packed 3 bits each (without codes: S = 1, code 0, no
// device read).  The values reach the kernels as a launch argument: the list is read
// back with one small blocking copy, once per tensor — a thread's last checked list is remembered
// (the tensor itself, so its memory cannot be handed out again, and its version counter, which
// every in-place write moves): a predictor pays the copy and the stall once per scene, not per pass
namespace {
struct CodesSeen {
  at::Tensor t;
  int64_t S = 0;
  uint32_t version = 0, packed = 0;
};
}  // namespace
static int pack_codes(const c10::optional<at::Tensor>& codes, const at::Tensor& like, uint32_t* packed) {
  *packed = 0u;
  const int64_t S = checks::codes(codes, like);
  if (!has(codes)) return 1;
  // (never freed: a device tensor must not be destroyed while the process exits)
  thread_local CodesSeen* seen_last = new CodesSeen();
  const bool versioned = !codes->is_inference();
  if (versioned && seen_last->t.defined() && seen_last->t.is_same(*codes) && seen_last->S == S &&
      seen_last->version == codes->_version()) {
    *packed = seen_last->packed;
    return (int)S;
  }
  const at::Tensor host = codes->contiguous().cpu();
  *packed = checks::pack_code_values(host.data_ptr<int>(), S);
  if (versioned) {
    seen_last->t = *codes;
    seen_last->S = S;
    seen_last->version = codes->_version();
    seen_last->packed = *packed;
  }
  return (int)S;
}

// HBM-resident uint8 scene [H, W, Cin] -> bf16 windows [B, tile, tile, cpad], mirrored borders;
// with codes [S]: [B * S, tile, tile, cpad], row b * S + j = window b under symmetry codes[j]
at::Tensor window_gather(const at::Tensor& scene, const at::Tensor& origins, int64_t tile,
                         int64_t cpad, const c10::optional<at::Tensor>& codes) {
  checks::window_gather(scene, origins, tile, cpad);
  CHECK_DEV(scene); CHECK_CONTIG(scene); CHECK_DEV(origins); CHECK_CONTIG(origins);
  const int64_t H = scene.size(0), W = scene.size(1), in_ch = scene.size(2);
  c10::DeviceGuard guard(scene.device());
  const int64_t B = origins.size(0);
  uint32_t packed = 0u;
  const int S = pack_codes(codes, scene, &packed);
  const int64_t nb = window_gather_blocks((int)tile);
  TORCH_CHECK(B * S * nb * nb < (1LL << 31), "window_gather: batch too large");
  at::Tensor x = at::empty({B * S, tile, tile, cpad}, scene.options().dtype(at::kBFloat16));
  if (B > 0)
    window_gather_launch(scene.data_ptr<uint8_t>(), origins.data_ptr<int>(), (int)B, S, packed, (int)H,
                         (int)W, (int)in_ch, (int)tile, (int)cpad, knob("WINDOW_LDS_T", 1) != 0,
                         bptr_mut(x), cur_stream());
  return x;
}

// acc[y0 + y, x0 + x, :K] += win[y] win[x] softmax(head(a)), acc[.., K] += win[y] win[x]
// PRECONDITION: the windows of one call are pairwise disjoint (plan_windows' colour groups):
// the kernel accumulates with plain read-modify-write, no atomics
void head_predict_accum(const at::Tensor& a, const at::Tensor& Wh, const at::Tensor& bh,
                        const at::Tensor& origins, const at::Tensor& win, at::Tensor& acc,
                        const c10::optional<at::Tensor>& bn4, const c10::optional<at::Tensor>& codes) {
  CHECK_DEV(a); CHECK_CONTIG(a);
  uint32_t packed = 0u;
  const int S = pack_codes(codes, a, &packed);
  checks::head_predict_accum(a, Wh, bh, origins, win, acc, S);
  const int64_t B = a.size(0) / S, tile = a.size(1);
  const int C = (int)a.size(3), K = (int)Wh.size(0);
  CHECK_DEV(Wh); CHECK_F32(Wh); CHECK_CONTIG(Wh); CHECK_DEV(bh); CHECK_F32(bh); CHECK_CONTIG(bh);
  TORCH_CHECK(head_supported(C, K), "head kernel: unsupported (C, K)");
  CHECK_DEV(origins); CHECK_CONTIG(origins); CHECK_DEV(win); CHECK_CONTIG(win); CHECK_DEV(acc); CHECK_CONTIG(acc);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(acc.data_ptr()) % 16 == 0, "acc must be 16-byte aligned");
  c10::DeviceGuard guard(a.device());
  const float* pbn = bn4_ptr(bn4, C);
  if (B == 0) return;
  head_predict_accum_launch(bptr(a), Wh.data_ptr<float>(), bh.data_ptr<float>(), origins.data_ptr<int>(),
                            win.data_ptr<float>(), acc.data_ptr<float>(), (int)B, S, packed, (int)tile,
                            (int)acc.size(0), (int)acc.size(1), (int)acc.size(2), C, K, pbn, cur_stream());
}

// accumulator [H, W, KA] -> {class map uint8 [H, W], confusion matrix int64 [K, K]}
std::vector<at::Tensor> scene_finalize(const at::Tensor& acc, int64_t K,
                                       const c10::optional<at::Tensor>& labels, int64_t ignore_index) {
  checks::scene_finalize(acc, K, labels);
  CHECK_DEV(acc); CHECK_CONTIG(acc);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(acc.data_ptr()) % 16 == 0, "acc must be 16-byte aligned");
  c10::DeviceGuard guard(acc.device());
  const int64_t H = acc.size(0), W = acc.size(1);
  const uint8_t* lp = nullptr;
  if (has(labels)) {
    CHECK_DEV(*labels); CHECK_CONTIG(*labels);
    lp = labels->data_ptr<uint8_t>();
  }
  at::Tensor pred = at::empty({H, W}, acc.options().dtype(at::kByte));
  at::Tensor cm = at::zeros({K, K}, acc.options().dtype(at::kLong));
  if (H * W > 0)
    scene_finalize_launch(acc.data_ptr<float>(), (long long)H * W, (int)K, (int)acc.size(2), lp,
                          (int)ignore_index, pred.data_ptr<uint8_t>(), cm.data_ptr<int64_t>(),
                          cur_stream());
  return {pred, cm};
}

// -> the CU count grids are sized for after reserving k CUs (k < 0: query only)
int64_t set_cu_reserve(int64_t k) {
  if (k >= 0) g_cu_reserve = (int)std::min<int64_t>(k, std::max(0, phys_cus() - 8));
  return num_cus();
}

// single-GPU stand-in for a bucket all-reduce (Trainer comm_proxy): `blocks` workgroups
// stream the bucket `passes` times (read + write back, values unchanged) on the current
// stream — RCCL's footprint (a few tens of channels, each a streaming workgroup)
void comm_proxy(const at::Tensor& g, int64_t blocks, int64_t passes) {
  CHECK_DEV(g); CHECK_CONTIG(g); CHECK_F32(g);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 == 0, "comm_proxy: 16-byte aligned buffer");
  c10::DeviceGuard guard(g.device());
  if (g.numel() == 0) return;
  comm_proxy_launch(g.data_ptr<float>(), g.numel(), (int)blocks, (int)passes, cur_stream());
}

}  // namespace

}  // namespace ddlpc

TORCH_LIBRARY(ddlpc, m) {
  m.def("set_cu_reserve(int k) -> int", &ddlpc::set_cu_reserve);
  m.def("set_knob(str name, int value) -> int", &ddlpc::set_knob);
  m.def("last_path() -> str", &ddlpc::last_path);
  m.def("comm_proxy(Tensor(a!) g, int blocks, int passes) -> ()");
  m.def("conv3_fwd(Tensor x1, Tensor? x2, Tensor w, Tensor? bias, Tensor? pscale, Tensor? pshift, "
        "int cout, int co1, bool stats, Tensor? pscale2=None, Tensor? pshift2=None, Tensor? bnb_y=None, "
        "Tensor? bnb_s4=None, int groups=0) -> Tensor[]");
  m.def("conv3_wgrad(Tensor dy, Tensor x1, Tensor? x2, Tensor? pscale, Tensor? pshift, Tensor(a!)? out=None, "
        "Tensor? pscale2=None, Tensor? pshift2=None, Tensor? dy_y=None, Tensor? dy_s4=None, "
        "Tensor? dy_coefs=None, int cin_real=0, int groups=0, Tensor(b!)? dy_out=None) -> Tensor");
  m.def("conv3_bwd32(Tensor dy, Tensor y, Tensor s4, Tensor wd, Tensor(a!)? dw_out=None, int groups=0) -> Tensor[]");
  m.def("reduce_rows(Tensor partial, int R, int N) -> Tensor");
  m.def("reduce_rows_scatter(Tensor slab, int R, int N, Tensor(a!) dst, int mode, int T, int B, "
        "bool accumulate, int ld=-1) -> ()");
  m.def("bn_finalize(Tensor partial, float count, Tensor gamma, Tensor beta, Tensor(a!) running_mean, "
        "Tensor(b!) running_var, float momentum, float eps, bool update_running, Tensor(c!)? nbt) -> Tensor");
  m.def("bn_relu_apply(Tensor y, Tensor stats4, bool pool, bool full=True) -> Tensor[]");
  m.def("bn_running_apply(Tensor(a!) running_mean, Tensor(b!) running_var, Tensor slots, float momentum, "
        "Tensor(c!)? nbt=None) -> ()");
  m.def("bn_grad_coefs(Tensor partial, Tensor y, Tensor stats4, Tensor gamma, "
        "Tensor(a!)? dgamma_out=None, Tensor(b!)? dbeta_out=None) -> Tensor[]");
  m.def("bn_group_finalize(Tensor y, int groups, Tensor gamma, Tensor beta, float eps, "
        "Tensor(a!)? arena=None, int aoff=0) -> Tensor");
  m.def("bn_group_apply(Tensor y, Tensor stats4, int groups, bool pool) -> Tensor[]");
  m.def("bn_running_apply_all(Tensor entries, Tensor(a!) arena, int K, int maxC, float momentum) -> ()");
  m.def("bn_group_backward(Tensor? dA, Tensor? dP, Tensor y, Tensor stats4, Tensor gamma, int groups, "
        "Tensor(a!)? dgamma_out=None, Tensor(b!)? dbeta_out=None, Tensor? partial=None) -> Tensor[]");
  m.def("bn_group_finalize_rows(Tensor partial, int groups, float count, Tensor gamma, Tensor beta, "
        "float eps, Tensor(a!)? arena=None, int aoff=0) -> Tensor");
  m.def("bn_backward(Tensor? dA, Tensor? dP, Tensor y, Tensor stats4, Tensor gamma, Tensor? gscale, "
        "Tensor(a!)? dgamma_out=None, Tensor(b!)? dbeta_out=None, Tensor? partial=None) -> Tensor[]");
  m.def("convt_fwd(Tensor x, Tensor wt, Tensor? bias, int cout, Tensor? bn4=None) -> Tensor");
  m.def("convt_dgrad(Tensor dout, Tensor wd, int cin, Tensor? bny=None, Tensor? bn4=None) -> Tensor[]");
  m.def("convt_wgrad(Tensor x, Tensor dout, Tensor(a!)? dw_out=None, Tensor(b!)? db_out=None, "
        "Tensor? colsum_rows=None, Tensor? bn4=None) -> Tensor[]");
  m.def("convt_bwd_fused(Tensor x, Tensor dout, Tensor wd, Tensor(a!)? dw_out=None, "
        "Tensor(b!)? db_out=None, Tensor? colsum_rows=None, Tensor? bn4=None) -> Tensor[]");
  m.def("head_ce_fwd(Tensor a, Tensor Wh, Tensor bh, Tensor labels, int ignore_index, Tensor? bn4=None, "
        "Tensor? class_weight=None) -> Tensor");
  m.def("head_ce_bwd(Tensor a, Tensor Wh, Tensor bh, Tensor labels, Tensor out3, Tensor? gscale, "
        "int ignore_index, Tensor(a!)? dw_out=None, Tensor(b!)? db_out=None, Tensor? bn4=None, "
        "bool store_da=True, Tensor? class_weight=None) -> Tensor[]");
  m.def("head_ce_bn_bwd(Tensor a, Tensor Wh, Tensor bh, Tensor labels, Tensor out3, Tensor? gscale, "
        "int ignore_index, Tensor bn4, Tensor partial, Tensor gamma, Tensor(a!)? dgamma_out=None, "
        "Tensor(b!)? dbeta_out=None, Tensor? pscale=None, int groups=0, "
        "Tensor? class_weight=None) -> Tensor[]");
  m.def("head_ce_fwd_stats(Tensor a, Tensor Wh, Tensor bh, Tensor labels, int ignore_index, "
        "Tensor bn4, int groups=0, Tensor? class_weight=None) -> Tensor[]");
  m.def("head_wgrad_from_rows(Tensor rows, Tensor scale, int K, int C, Tensor(a!)? dw_out=None, "
        "Tensor(b!)? db_out=None) -> Tensor[]");
  m.def("meter_add(Tensor(a!) buf, Tensor loss, Tensor correct, float pixels, float count=1.) -> ()");
  m.def("head_grad_scale(Tensor out3, Tensor? gs=None) -> Tensor");
  m.def("head_logits(Tensor a, Tensor Wh, Tensor bh, Tensor? bn4=None) -> Tensor");
  m.def("adam_step(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) v, float b1, float b2, float eps, "
        "float wd, float step_size, float inv_sqrt_bc2) -> ()");
  m.def("adam_step_dev(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor(d!) scal, "
        "float lr, float b1, float b2, float eps, float wd) -> ()");
  // sched_kind: 0 constant, 1 poly, 2 cosine (the schedule of csrc/optim_math.h)
  m.def("adam_step_sched(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) v, Tensor(d!) scal, "
        "Tensor(e!) partial, float lr, float b1, float b2, float eps, float wd, bool decoupled, "
        "float max_norm, int sched_kind, int warmup, int total, float lr_min, float power) -> ()");
  m.def("weight_pack(Tensor entries, int n, int max_elems) -> ()");
  m.def("codec_absmax(Tensor x, Tensor seg) -> Tensor");
  m.def("codec_encode(Tensor x, Tensor seg, Tensor scales, int codec) -> Tensor");
  m.def("codec_decode_sum(Tensor(a!) out, Tensor q, Tensor scales, Tensor w, Tensor seg, int codec) -> ()");
  m.def("bilinear_up2(Tensor x) -> Tensor");
  m.def("bilinear_up2_bwd(Tensor dy) -> Tensor");
  m.def("to_nhwc_bf16(Tensor x, int cpad=1) -> Tensor");
  m.def("synth_tiles(Tensor idx, int seed, int classes, int in_ch, int tile, int dims, int grid, "
        "float k, Tensor palette, int cpad) -> Tensor[]");
  m.def("tile_gather(Tensor src, Tensor lab, Tensor idx, int cpad) -> Tensor[]");
  m.def("crop_gather(Tensor scenes, Tensor labels, Tensor table, Tensor params, Tensor? color, "
        "int tile, int cpad) -> Tensor[]");
  m.def("crop_params(Tensor idx, Tensor cum, Tensor table, int seed, int tile, int mode, "
        "float gain_jitter, float bias_jitter) -> Tensor[]");
  m.def("warp_gather(Tensor scenes, Tensor labels, Tensor table, Tensor wparams, Tensor? color, "
        "int tile, int cpad) -> Tensor[]");
  m.def("warp_params(Tensor idx, Tensor cum, Tensor table, Tensor steps, Tensor rot, int seed, int tile, "
        "int mode, float gain_jitter, float bias_jitter) -> Tensor[]");
  m.def("window_gather(Tensor scene, Tensor origins, int tile, int cpad, Tensor? codes=None) -> Tensor");
  // (the windows of one call must be pairwise disjoint: acc is updated without atomics)
  m.def("head_predict_accum(Tensor a, Tensor Wh, Tensor bh, Tensor origins, Tensor win, Tensor(a!) acc, "
        "Tensor? bn4=None, Tensor? codes=None) -> ()");
  m.def("scene_finalize(Tensor acc, int K, Tensor? labels=None, int ignore_index=-100) -> Tensor[]");
}

TORCH_LIBRARY_IMPL(ddlpc, CUDA, m) {
  m.impl("conv3_fwd", &ddlpc::conv3_fwd);
  m.impl("conv3_wgrad", &ddlpc::conv3_wgrad);
  m.impl("bn_finalize", &ddlpc::bn_finalize);
  m.impl("reduce_rows", &ddlpc::reduce_rows);
  m.impl("reduce_rows_scatter", &ddlpc::reduce_rows_scatter);
  m.impl("bn_relu_apply", &ddlpc::bn_relu_apply);
  m.impl("bn_running_apply", &ddlpc::bn_running_apply);
  m.impl("bn_grad_coefs", &ddlpc::bn_grad_coefs);
  m.impl("conv3_bwd32", &ddlpc::conv3_bwd32);
  m.impl("bn_backward", &ddlpc::bn_backward);
  m.impl("bn_group_finalize", &ddlpc::bn_group_finalize);
  m.impl("bn_group_apply", &ddlpc::bn_group_apply);
  m.impl("bn_running_apply_all", &ddlpc::bn_running_apply_all);
  m.impl("bn_group_backward", &ddlpc::bn_group_backward);
  m.impl("bn_group_finalize_rows", &ddlpc::bn_group_finalize_rows);
  m.impl("convt_fwd", &ddlpc::convt_fwd);
  m.impl("convt_dgrad", &ddlpc::convt_dgrad);
  m.impl("convt_wgrad", &ddlpc::convt_wgrad);
  m.impl("convt_bwd_fused", &ddlpc::convt_bwd_fused);
  m.impl("head_ce_fwd", &ddlpc::head_ce_fwd);
  m.impl("head_ce_bwd", &ddlpc::head_ce_bwd);
  m.impl("head_ce_bn_bwd", &ddlpc::head_ce_bn_bwd);
  m.impl("head_ce_fwd_stats", &ddlpc::head_ce_fwd_stats);
  m.impl("head_wgrad_from_rows", &ddlpc::head_wgrad_from_rows);
  m.impl("head_grad_scale", &ddlpc::head_grad_scale);
  m.impl("meter_add", &ddlpc::meter_add);
  m.impl("head_logits", &ddlpc::head_logits);
  m.impl("adam_step", &ddlpc::adam_step);
  m.impl("adam_step_dev", &ddlpc::adam_step_dev);
  m.impl("adam_step_sched", &ddlpc::adam_step_sched);
  m.impl("weight_pack", &ddlpc::weight_pack);
  m.impl("codec_absmax", &ddlpc::codec_absmax);
  m.impl("codec_encode", &ddlpc::codec_encode);
  m.impl("codec_decode_sum", &ddlpc::codec_decode_sum);
  m.impl("bilinear_up2", &ddlpc::bilinear_up2);
  m.impl("bilinear_up2_bwd", &ddlpc::bilinear_up2_bwd);
  m.impl("to_nhwc_bf16", &ddlpc::to_nhwc_bf16);
  m.impl("synth_tiles", &ddlpc::synth_tiles);
  m.impl("tile_gather", &ddlpc::tile_gather);
  m.impl("crop_gather", &ddlpc::crop_gather);
  m.impl("crop_params", &ddlpc::crop_params);
  m.impl("warp_gather", &ddlpc::warp_gather);
  m.impl("warp_params", &ddlpc::warp_params);
  m.impl("window_gather", &ddlpc::window_gather);
  m.impl("head_predict_accum", &ddlpc::head_predict_accum);
  m.impl("scene_finalize", &ddlpc::scene_finalize);
  m.impl("comm_proxy", &ddlpc::comm_proxy);
}
