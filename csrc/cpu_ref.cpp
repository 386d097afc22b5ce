// CPU kernels of the ddlpc operator namespace: TORCH_LIBRARY_IMPL(ddlpc, CPU, ...).
//
// Every operator that bindings.cpp declares (TORCH_LIBRARY(ddlpc)) and registers for the
// GPU (TORCH_LIBRARY_IMPL(ddlpc, CUDA)) gets a plain C++ / ATen reference here, with the
// same schema, the same tensor conventions and the same numerics contract: bf16
// channel-last activations [N, (D,) H, W, C], fp32 accumulation, bf16 outputs, fp64
// statistics reductions, packed bf16 weights from weight_pack.  PyTorch's dispatcher picks
// the kernel by the tensors' device, so the engine (ops/fused_unet.py) runs one code path
// on either device and a CPU-only machine trains the same model through the same ops
// (one op namespace, CPU kernel = ATen reference, device dispatch by
// PyTorch).  The GPU tests compare every op on both devices (tests/test_cpu_ops.py).
//
// Partial-row outputs ([R][2][C] statistics, [R][K*C+K] head rows) use R = 1 row (per
// group where the op is grouped): consumers sum rows, so any R is valid.
// comm_proxy has no CPU kernel: it stands in for an RCCL collective on one GPU.
#include <ATen/ATen.h>
#include <ATen/Parallel.h>
#include <torch/library.h>

#include <array>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "bn_math.h"
#include "data_checks.h"
#include "data_math.h"
#include "optim_math.h"
#include "tail_checks.h"

namespace ddlpc {
void set_last_path(const std::string& path);    // bindings.cpp: torch.ops.ddlpc.last_path
int grad_sqnorm_blocks(long long n);            // optim.hip: the norm's partial sums (planner)
}

namespace ddlpc_cpu {

using at::Tensor;
using c10::optional;
using namespace ddlpc;      // the *_math.h and *_checks.h headers

namespace {

bool has(const optional<Tensor>& t) { return t.has_value() && t->defined(); }
bool has_nonempty(const optional<Tensor>& t) { return has(t) && t->numel() > 0; }
Tensor f32(const Tensor& t) { return t.to(at::kFloat); }
Tensor bf(const Tensor& t) { return t.to(at::kBFloat16); }
Tensor rbf(const Tensor& t) { return t.to(at::kBFloat16).to(at::kFloat); }    // bf16 rounding
Tensor empty_f(const Tensor& like) { return at::empty({0}, like.options().dtype(at::kFloat)); }

int sdims(const Tensor& x) {
  TORCH_CHECK(x.dim() == 4 || x.dim() == 5, "expected [N,(D,)H,W,C] channel-last tensor");
  return (int)x.dim() - 2;
}
// channel-last [N, S..., C] <-> channel-first [N, C, S...]
Tensor to_cf(const Tensor& x) {
  std::vector<int64_t> p = {0, x.dim() - 1};
  for (int64_t i = 1; i < x.dim() - 1; ++i) p.push_back(i);
  return x.permute(p);
}
Tensor to_cl(const Tensor& x) {
  std::vector<int64_t> p = {0};
  for (int64_t i = 2; i < x.dim(); ++i) p.push_back(i);
  p.push_back(1);
  return x.permute(p).contiguous();
}

// rows r of stats4 [4][C] -> [C]; grouped [G][4][C] -> [G][C]
Tensor s4row(const Tensor& s4, int64_t G, int64_t C, int r) {
  if (G > 1) return s4.reshape({G, 4, C}).select(1, r);
  return s4.reshape({4, C}).select(0, r);
}

// per-channel affine of a channel-last tensor; v: [C] or, with groups, [G][C] (the batch
// holds the G groups' images one after another)
Tensor chan(const Tensor& x, const Tensor& v, int64_t G) {
  const int64_t C = x.size(-1);
  if (G > 1 && v.dim() == 2) return v.reshape({G, 1, C});
  return v.reshape({C});
}
Tensor grouped(const Tensor& x, int64_t G) {
  return G > 1 ? x.reshape({G, -1, x.size(-1)}) : x;
}
// BN + ReLU of a pre-BN tensor, rounded to bf16 as a materialised activation
Tensor bn_act(const Tensor& yf, const Tensor& scale, const Tensor& shift, int64_t G) {
  const Tensor xg = grouped(yf, G);
  return rbf(at::relu(xg * chan(yf, scale, G) + chan(yf, shift, G))).reshape(yf.sizes());
}

// packed [Cout][taps][CinW] -> fp32 OIHW / OIDHW over the first Cin input channels
Tensor unpack_w3(const Tensor& wp, int64_t cin, int dims) {
  const int64_t cout = wp.size(0);
  Tensor w = f32(wp.narrow(2, 0, cin)).permute({0, 2, 1});
  if (dims == 2) return w.reshape({cout, cin, 3, 3});
  return w.reshape({cout, cin, 3, 3, 3});
}

// (a channel-last tensor viewed channel-first IS channels_last memory: oneDNN convolves it
// in place, no layout copies)
at::MemoryFormat cl_format(int dims) {
  return dims == 2 ? at::MemoryFormat::ChannelsLast : at::MemoryFormat::ChannelsLast3d;
}

Tensor conv_same(const Tensor& xcl, const Tensor& w, int dims) {
  const Tensor x = to_cf(xcl).contiguous(cl_format(dims));
  const Tensor y = dims == 2 ? at::conv2d(x, w, {}, 1, 1) : at::conv3d(x, w, {}, 1, 1);
  return to_cl(y);
}

Tensor wgrad_same(const Tensor& dycl, const Tensor& xcl, int dims) {
  const int64_t cout = dycl.size(-1), cin = xcl.size(-1);
  std::vector<int64_t> ws = {cout, cin, 3, 3};
  if (dims == 3) ws.push_back(3);
  const Tensor w = at::zeros(ws, xcl.options().dtype(at::kFloat));
  std::vector<int64_t> one(dims, 1), zero(dims, 0);
  auto r = at::convolution_backward(to_cf(dycl).contiguous(cl_format(dims)),
                                    to_cf(xcl).contiguous(cl_format(dims)), w.contiguous(cl_format(dims)),
                                    c10::nullopt, one, one, one, false, zero, 1,
                                    {false, true, false});
  return std::get<1>(r);
}

// (sum, sum^2) per channel -> [G][2][C] rows
Tensor stat_rows(const Tensor& yf, int64_t G) {
  const int64_t C = yf.size(-1);
  const Tensor d = yf.to(at::kDouble).reshape({G, -1, C});
  return at::stack({d.sum(1), (d * d).sum(1)}, 1).to(at::kFloat);
}

// BatchNorm-backward partial rows (sum dyh, sum dyh * xhat) of an activation gradient dA
// against the pre-BN y (ReLU mask from y * scale + shift): [G][2][C]
Tensor bnb_rows(const Tensor& dAf, const Tensor& yf, const Tensor& s4, int64_t G) {
  const int64_t C = yf.size(-1);
  const Tensor yg = grouped(yf, G), dg = grouped(dAf, G);
  const Tensor a = yg * chan(yf, s4row(s4, G, C, 2), G) + chan(yf, s4row(s4, G, C, 3), G);
  const Tensor dyh = at::where(a > 0, dg, at::zeros_like(dg)).to(at::kDouble);
  const Tensor xh = ((yg - chan(yf, s4row(s4, G, C, 0), G)) * chan(yf, s4row(s4, G, C, 1), G))
                        .to(at::kDouble);
  const Tensor d3 = dyh.reshape({G, -1, C}), x3 = xh.reshape({G, -1, C});
  return at::stack({d3.sum(1), (d3 * x3).sum(1)}, 1).to(at::kFloat);
}

// unpool a pooled gradient to the first arg-max of the bf16-rounded activation's windows
Tensor unpool(const Tensor& dPf, const Tensor& act, int dims) {
  const Tensor a = to_cf(act).contiguous();
  const Tensor g = to_cf(dPf).contiguous();
  std::vector<int64_t> k(dims, 2), zero(dims, 0), one(dims, 1);
  Tensor out;
  if (dims == 2) {
    auto r = at::max_pool2d_with_indices(a, k, k, zero, one, false);
    out = at::max_pool2d_with_indices_backward(g, a, k, k, zero, one, false, std::get<1>(r));
  } else {
    auto r = at::max_pool3d_with_indices(a, k, k, zero, one, false);
    out = at::max_pool3d_with_indices_backward(g, a, k, k, zero, one, false, std::get<1>(r));
  }
  return to_cl(out);
}

Tensor maxpool(const Tensor& act, int dims) {
  const Tensor a = to_cf(act).contiguous();
  return to_cl(dims == 2 ? at::max_pool2d(a, {2, 2}, {2, 2}) : at::max_pool3d(a, {2, 2, 2}, {2, 2, 2}));
}

// dY = k * (dyh - m1 - xhat * m2) with dyh = dt * gs where y * scale + shift > 0
struct BnBwd {
  Tensor dyh, xh;
};
BnBwd bn_terms(const Tensor& dtf, const Tensor& yf, const Tensor& s4, int64_t G, double gs) {
  const int64_t C = yf.size(-1);
  const Tensor yg = grouped(yf, G), dg = grouped(dtf, G);
  const Tensor a = yg * chan(yf, s4row(s4, G, C, 2), G) + chan(yf, s4row(s4, G, C, 3), G);
  BnBwd t;
  t.dyh = at::where(a > 0, dg * gs, at::zeros_like(dg));
  t.xh = (yg - chan(yf, s4row(s4, G, C, 0), G)) * chan(yf, s4row(s4, G, C, 1), G);
  return t;
}

// sums [G][2][C] (fp64) -> coefficients [G][3][C] = (gamma * invstd, s1 / count, s2 / count);
// dbeta / dgamma = sums over the groups in group order, written or accumulated
Tensor bn_coefs(const Tensor& sums, const Tensor& s4, const Tensor& gamma, int64_t G, double count,
                Tensor& dgamma, Tensor& dbeta, bool into) {
  const int64_t C = gamma.numel();
  const Tensor S = sums.contiguous(), gc = gamma.contiguous(), inv = s4row(s4, G, C, 1).reshape({G, C}).contiguous();
  Tensor coefs = at::empty({G, 3, C}, gamma.options());
  if (!into) {
    dbeta = at::empty({C}, gamma.options());
    dgamma = at::empty({C}, gamma.options());
  }
  TORCH_INTERNAL_ASSERT(dgamma.is_contiguous() && dbeta.is_contiguous() && dgamma.numel() == C && dbeta.numel() == C);
  const double* s = S.data_ptr<double>();
  const float* g = gc.data_ptr<float>();
  const float* iv = inv.data_ptr<float>();
  float* k = coefs.data_ptr<float>();
  float* db = dbeta.data_ptr<float>();
  float* dg = dgamma.data_ptr<float>();
  for (int64_t c = 0; c < C; ++c) {
    double a = 0.0, b = 0.0;
    for (int64_t q = 0; q < G; ++q) {
      const double t1 = s[(q * 2) * C + c], t2 = s[(q * 2 + 1) * C + c];
      const BnGradTerms t = bn_grad_terms(t1, t2, count, g[c], iv[q * C + c]);
      k[(q * 3) * C + c] = t.k;
      k[(q * 3 + 1) * C + c] = t.m1;
      k[(q * 3 + 2) * C + c] = t.m2;
      a += t1;
      b += t2;
    }
    db[c] = into ? db[c] + (float)a : (float)a;
    dg[c] = into ? dg[c] + (float)b : (float)b;
  }
  return coefs;
}

Tensor bn_apply_coefs(const BnBwd& t, const Tensor& coefs, const Tensor& like, int64_t G) {
  const int64_t C = like.size(-1);
  const Tensor cg = coefs.reshape({G, 3, C});
  auto col = [&](int r) { return G > 1 ? cg.select(1, r).reshape({G, 1, C}) : cg.select(1, r).reshape({C}); };
  const Tensor dy = col(0) * (t.dyh - col(1) - t.xh * col(2));
  return bf(dy.reshape(like.sizes()));
}

// dst (+)= v for a caller-owned gradient buffer of v's element count (any strides)
void add_to(Tensor dst, const Tensor& v) {
  TORCH_CHECK(dst.numel() == v.numel(), "gradient out size mismatch");
  dst.add_(v.reshape(dst.sizes()));
}

double scalar_or(const optional<Tensor>& t, double d) {
  return has(t) ? t->to(at::kDouble).reshape({-1})[0].item<double>() : d;
}

// ------------------------------------------------------------------------ conv 3x3(x3)
Tensor prologue_input(const Tensor& x1, const optional<Tensor>& x2, const optional<Tensor>& ps,
                      const optional<Tensor>& sh, const optional<Tensor>& ps2,
                      const optional<Tensor>& sh2, int64_t G) {
  Tensor a = f32(x1);
  if (has(ps)) a = bn_act(a, *ps, *sh, G);
  if (has(x2)) {
    Tensor b = f32(*x2);
    if (has(ps2)) b = bn_act(b, *ps2, *sh2, 1);
    a = at::cat({a, b}, -1);
  }
  return a;
}

std::vector<Tensor> conv3_fwd(const Tensor& x1, const optional<Tensor>& x2, const Tensor& w,
                              const optional<Tensor>& bias, const optional<Tensor>& pscale,
                              const optional<Tensor>& pshift, int64_t cout, int64_t co1, bool want_stats,
                              const optional<Tensor>& pscale2, const optional<Tensor>& pshift2,
                              const optional<Tensor>& bnb_y, const optional<Tensor>& bnb_s4, int64_t groups) {
  ddlpc::set_last_path("cpu");
  const int dims = sdims(x1);
  const int64_t G = groups > 1 ? groups : 1;
  TORCH_CHECK(x1.size(0) % G == 0, "conv3_fwd: groups must divide the batch");
  const Tensor xin = prologue_input(x1, x2, pscale, pshift, pscale2, pshift2, G);
  TORCH_CHECK(w.dim() == 3 && w.size(0) == cout && w.size(2) >= xin.size(-1),
              "packed weight must be [Cout][taps][CinW>=Cin]");
  Tensor out = conv_same(xin, unpack_w3(w, xin.size(-1), dims), dims);
  if (has(bias)) out = out + bias->reshape({cout});
  const Tensor yb = bf(out);
  const int64_t c1 = co1 > 0 ? co1 : cout;
  const Tensor none = at::empty({0}, x1.options());
  Tensor y1 = c1 < cout ? yb.narrow(-1, 0, c1).contiguous() : yb;
  Tensor y2 = c1 < cout ? yb.narrow(-1, c1, cout - c1).contiguous() : none;
  Tensor stats = none;
  // (statistics of the fp32 outputs before the bf16 store, as the GPU epilogues reduce them)
  if (has(bnb_y)) stats = bnb_rows(out, f32(*bnb_y), *bnb_s4, G);
  else if (want_stats) stats = stat_rows(out, G);
  return {y1, y2, stats};
}

Tensor conv3_wgrad(const Tensor& dy, const Tensor& x1, const optional<Tensor>& x2,
                   const optional<Tensor>& pscale, const optional<Tensor>& pshift,
                   const optional<Tensor>& out, const optional<Tensor>& pscale2,
                   const optional<Tensor>& pshift2, const optional<Tensor>& dy_y,
                   const optional<Tensor>& dy_s4, const optional<Tensor>& dy_coefs, int64_t cin_real,
                   int64_t groups, const optional<Tensor>& dy_out) {
  ddlpc::set_last_path("cpu");
  (void)cin_real;                       // (the GPU's image-layer kernel choice; same result)
  const int dims = sdims(x1);
  const int64_t G = groups > 1 ? groups : 1;
  Tensor d = f32(dy);
  if (has(dy_y)) {
    // dy holds dA: BatchNorm backward applied on load with the reduced coefficients
    TORCH_CHECK(has(dy_s4) && has(dy_coefs), "conv3_wgrad: dy_s4 [4][Cout] and dy_coefs [3][Cout]");
    const BnBwd t = bn_terms(d, f32(*dy_y), *dy_s4, 1, 1.0);
    const Tensor dY = bn_apply_coefs(t, *dy_coefs, dy, 1);
    if (has(dy_out)) dy_out->copy_(dY.reshape(dy_out->sizes()));
    d = f32(dY);
  }
  TORCH_CHECK(!has(dy_out) || has(dy_y), "conv3_wgrad: dy_out needs the dY prologue");
  const Tensor xin = prologue_input(x1, x2, pscale, pshift, pscale2, pshift2, G);
  const Tensor dW = wgrad_same(d, xin, dims);
  if (has(out)) {
    TORCH_CHECK(out->numel() == dW.numel(), "dW out size mismatch");
    add_to(*out, dW);
    return empty_f(dy);
  }
  return dW;
}

std::vector<Tensor> conv3_bwd32(const Tensor& dy, const Tensor& y, const Tensor& s4, const Tensor& wd,
                                const optional<Tensor>& dw_out, int64_t groups) {
  ddlpc::set_last_path("cpu");
  const int64_t G = groups > 1 ? groups : 1;
  const int64_t C = y.size(-1);
  const Tensor yf = f32(y);
  const Tensor dAf = conv_same(f32(dy), unpack_w3(wd, dy.size(-1), 2), 2);
  const Tensor dA = bf(dAf);
  const Tensor part = bnb_rows(dAf, yf, s4, G);
  const Tensor x = bn_act(yf, s4row(s4, G, C, 2), s4row(s4, G, C, 3), G);
  const Tensor dW = wgrad_same(f32(dy), x, 2);
  if (has(dw_out)) {
    add_to(*dw_out, dW);
    return {dA, part, empty_f(dy)};
  }
  return {dA, part, dW};
}

Tensor reduce_rows(const Tensor& partial, int64_t R, int64_t N) {
  checks::reduce_rows(partial, R, N);
  return partial.reshape({R, N}).to(at::kDouble).sum(0);
}

// dst[slab_perm(j)] (+)= float(fp64 sum over R rows of slab[r * ld + j]), in the summation
// order of the row-count regime reduce_rows_scatter_launch (csrc/reduce.hip) takes for R
void reduce_rows_scatter(const Tensor& slab, int64_t R, int64_t N, Tensor& dst, int64_t mode, int64_t T,
                         int64_t B, bool accumulate, int64_t ld) {
  checks::reduce_rows_scatter(slab, R, N, dst, mode, T, B, ld);
  if (R == 0 || N == 0) return;
  const float* in = slab.data_ptr<float>();
  float* out = dst.data_ptr<float>();
  for (int64_t j = 0; j < N; ++j) {
    const int64_t d = slab_perm((int)mode, j, (int)T, (int)B);
    const float v = (float)slab_column_sum(in, R, ld < 0 ? N : ld, j);
    out[d] = accumulate ? out[d] + v : v;
  }
}

// ------------------------------------------------------------------------ BatchNorm
// stats4 [G][4][C] from fp64 sums [G][2][C]; arena rows (mean | unbiased var) if given
Tensor stats4_from_sums(const Tensor& sums, double count, const Tensor& gamma, const Tensor& beta,
                        double eps, int64_t G, float* arena, int64_t astride) {
  const int64_t C = gamma.numel();
  Tensor st = at::empty({G, 4, C}, gamma.options());
  const auto S = sums.contiguous();
  const double* s = S.data_ptr<double>();
  const Tensor gc = gamma.contiguous(), bc = beta.contiguous();
  const float* g = gc.data_ptr<float>();
  const float* b = bc.data_ptr<float>();
  float* o = st.data_ptr<float>();
  for (int64_t k = 0; k < G; ++k)
    for (int64_t c = 0; c < C; ++c) {
      const BnStats4 r = bn_stats4(s[(k * 2) * C + c], s[(k * 2 + 1) * C + c], count, g[c], b[c], (float)eps);
      float* ok = o + k * 4 * C;
      ok[c] = r.mean;
      ok[C + c] = r.invstd;
      ok[2 * C + c] = r.scale;
      ok[3 * C + c] = r.shift;
      if (arena != nullptr) {
        arena[k * astride + c] = r.mean;
        arena[k * astride + C + c] = bn_unbiased_var(r.var, count);
      }
    }
  return st;
}

Tensor bn_finalize(const Tensor& partial, double count, const Tensor& gamma, const Tensor& beta,
                   Tensor running_mean, Tensor running_var, double momentum, double eps,
                   bool update_running, const optional<Tensor>& nbt) {
  checks::bn_finalize(partial, gamma, beta, running_mean, running_var, nbt);
  ddlpc::set_last_path("cpu");
  const int64_t C = gamma.numel();
  const Tensor sums = partial.reshape({-1, 2, C}).to(at::kDouble).sum(0, true);
  Tensor arena;
  float* ap = nullptr;
  if (update_running) {
    arena = at::empty({2 * C}, gamma.options());
    ap = arena.data_ptr<float>();
  }
  const Tensor st = stats4_from_sums(sums, count, gamma, beta, eps, 1, ap, 0).reshape({4, C});
  if (update_running) {
    float* rm = running_mean.data_ptr<float>();
    float* rv = running_var.data_ptr<float>();
    for (int64_t c = 0; c < C; ++c) {
      rm[c] = bn_momentum_update(rm[c], ap[c], (float)momentum);
      rv[c] = bn_momentum_update(rv[c], ap[C + c], (float)momentum);
    }
    if (has(nbt)) nbt->add_(1);
  }
  return st;
}

void bn_running_apply(Tensor running_mean, Tensor running_var, const Tensor& slots, double momentum,
                      const optional<Tensor>& nbt) {
  checks::bn_running_apply(running_mean, running_var, slots, nbt);
  const int C = (int)running_mean.numel(), K = (int)slots.size(0);
  for (int c = 0; c < C; ++c)
    bn_running_apply_channel(running_mean.data_ptr<float>(), running_var.data_ptr<float>(),
                             slots.data_ptr<float>(), K, C, slots.stride(0), c, (float)momentum);
  if (has(nbt) && K > 0) nbt->add_(K);
}

void bn_running_apply_all(const Tensor& entries, const Tensor& arena, int64_t K, int64_t maxC, double momentum) {
  checks::bn_running_apply_all(entries, arena, K, maxC);
  const Tensor e = entries.contiguous();
  const int64_t* ep = e.data_ptr<int64_t>();
  const float* a = arena.data_ptr<float>();
  const int64_t stride = arena.stride(0);
  for (int64_t l = 0; l < e.size(0); ++l) {
    float* rm = reinterpret_cast<float*>(ep[4 * l]);
    float* rv = reinterpret_cast<float*>(ep[4 * l + 1]);
    int64_t* nb = reinterpret_cast<int64_t*>(ep[4 * l + 2]);
    const int C = (int)(ep[4 * l + 3] & 0xffffffff);
    const int64_t off = (int64_t)((uint64_t)ep[4 * l + 3] >> 32);
    if (nb != nullptr) nb[0] += K;
    for (int c = 0; c < C; ++c) bn_running_apply_channel(rm, rv, a + off, (int)K, C, stride, c, (float)momentum);
  }
}

std::vector<Tensor> relu_apply_groups(const Tensor& y, const Tensor& stats4, int64_t G, bool pool, bool full) {
  ddlpc::set_last_path("cpu");
  const int64_t C = y.size(-1);
  const Tensor a = bn_act(f32(y), s4row(stats4, G, C, 2), s4row(stats4, G, C, 3), G);
  const Tensor none = at::empty({0}, y.options());
  return {full ? bf(a) : none, pool ? bf(maxpool(a, sdims(y))) : none};
}

std::vector<Tensor> bn_relu_apply(const Tensor& y, const Tensor& stats4, bool pool, bool full) {
  checks::bn_relu_apply(y, stats4, pool, full);
  return relu_apply_groups(y, stats4, 1, pool, full);
}

// dA (+ unpool(dP)) through ReLU and BN, per group; partial rows replace the reduction
std::vector<Tensor> bn_backward_groups(const optional<Tensor>& dA, const optional<Tensor>& dP, const Tensor& y,
                                       const Tensor& stats4, const Tensor& gamma, int64_t G, double gs,
                                       const optional<Tensor>& dgamma_out, const optional<Tensor>& dbeta_out,
                                       const optional<Tensor>& partial) {
  ddlpc::set_last_path("cpu");
  const bool hasA = has(dA), hasP = has(dP);
  const int64_t C = y.size(-1);
  const Tensor yf = f32(y);
  Tensor dt = hasA ? f32(*dA).reshape(y.sizes()) : at::zeros_like(yf);
  if (hasP) {
    const Tensor act = bn_act(yf, s4row(stats4, G, C, 2), s4row(stats4, G, C, 3), G);
    dt = dt + unpool(f32(*dP), act, sdims(y));
  }
  const BnBwd t = bn_terms(dt, yf, stats4, G, gs);
  Tensor sums;
  if (has_nonempty(partial)) {
    sums = partial->reshape({G, -1, 2, C}).to(at::kDouble).sum(1);
  } else {
    const Tensor d3 = t.dyh.to(at::kDouble).reshape({G, -1, C});
    const Tensor x3 = t.xh.to(at::kDouble).reshape({G, -1, C});
    sums = at::stack({d3.sum(1), (d3 * x3).sum(1)}, 1);
  }
  const bool into = has(dgamma_out);
  Tensor dgamma = into ? *dgamma_out : Tensor(), dbeta = into ? *dbeta_out : Tensor();
  const double count = (double)(y.numel() / C / G);
  const Tensor coefs = bn_coefs(sums, stats4, gamma, G, count, dgamma, dbeta, into);
  return {bn_apply_coefs(t, coefs, y, G), dgamma, dbeta};
}

std::vector<Tensor> bn_backward(const optional<Tensor>& dA, const optional<Tensor>& dP, const Tensor& y,
                                const Tensor& stats4, const Tensor& gamma, const optional<Tensor>& gscale,
                                const optional<Tensor>& dgamma_out, const optional<Tensor>& dbeta_out,
                                const optional<Tensor>& partial_in) {
  checks::bn_backward(dA, dP, y, stats4, gamma, gscale, dgamma_out, dbeta_out, partial_in);
  return bn_backward_groups(dA, dP, y, stats4, gamma, 1, scalar_or(gscale, 1.0), dgamma_out, dbeta_out,
                            partial_in);
}

std::vector<Tensor> bn_grad_coefs(const Tensor& partial, const Tensor& y, const Tensor& stats4, const Tensor& gamma,
                                  const optional<Tensor>& dgamma_out, const optional<Tensor>& dbeta_out) {
  checks::bn_grad_coefs(partial, y, stats4, gamma, dgamma_out, dbeta_out);
  ddlpc::set_last_path("cpu");
  const int64_t C = y.size(-1);
  const Tensor sums = partial.reshape({1, -1, 2, C}).to(at::kDouble).sum(1);
  const bool into = has(dgamma_out);
  Tensor dgamma = into ? *dgamma_out : Tensor(), dbeta = into ? *dbeta_out : Tensor();
  const Tensor coefs = bn_coefs(sums, stats4, gamma, 1, (double)(y.numel() / C), dgamma, dbeta, into);
  return {coefs.reshape({3, C}), dgamma, dbeta};
}

std::pair<float*, int64_t> arena_ptr(const optional<Tensor>& arena, int64_t aoff) {
  if (!has(arena)) return {nullptr, 0};
  return {arena->data_ptr<float>() + aoff, arena->stride(0)};
}

Tensor bn_group_finalize(const Tensor& y, int64_t groups, const Tensor& gamma, const Tensor& beta, double eps,
                         const optional<Tensor>& arena, int64_t aoff) {
  checks::bn_group_finalize(y, groups, gamma, beta, arena, aoff);
  const int64_t C = y.size(-1);
  const Tensor d = f32(y).to(at::kDouble).reshape({groups, -1, C});
  const Tensor sums = at::stack({d.sum(1), (d * d).sum(1)}, 1);
  auto ap = arena_ptr(arena, aoff);
  return stats4_from_sums(sums, (double)d.size(1), gamma, beta, eps, groups, ap.first, ap.second);
}

Tensor bn_group_finalize_rows(const Tensor& partial, int64_t groups, double count, const Tensor& gamma,
                              const Tensor& beta, double eps, const optional<Tensor>& arena, int64_t aoff) {
  checks::bn_group_finalize_rows(partial, groups, gamma, beta, arena, aoff);
  const int64_t C = gamma.numel();
  const Tensor sums = partial.reshape({groups, -1, 2, C}).to(at::kDouble).sum(1);
  auto ap = arena_ptr(arena, aoff);
  return stats4_from_sums(sums, count, gamma, beta, eps, groups, ap.first, ap.second);
}

std::vector<Tensor> bn_group_apply(const Tensor& y, const Tensor& stats4, int64_t groups, bool pool) {
  checks::bn_group_apply(y, stats4, groups, pool);
  return relu_apply_groups(y, stats4, groups, pool, true);
}

std::vector<Tensor> bn_group_backward(const optional<Tensor>& dA, const optional<Tensor>& dP, const Tensor& y,
                                      const Tensor& stats4, const Tensor& gamma, int64_t groups,
                                      const optional<Tensor>& dgamma_out, const optional<Tensor>& dbeta_out,
                                      const optional<Tensor>& partial) {
  checks::bn_group_backward(dA, dP, y, stats4, gamma, groups, dgamma_out, dbeta_out, partial);
  return bn_backward_groups(dA, dP, y, stats4, gamma, groups, 1.0, dgamma_out, dbeta_out, partial);
}

// ------------------------------------------------------------------------ transposed conv
// [M][S*cout] GEMM columns (sub-position major) <-> the 2x-up-sampled channel-last tensor
Tensor shuffle_up(const Tensor& cols, const Tensor& x, int64_t cout) {
  const int dims = sdims(x);
  const int64_t N = x.size(0);
  if (dims == 2) {
    const int64_t H = x.size(1), W = x.size(2);
    return cols.reshape({N, H, W, 2, 2, cout}).permute({0, 1, 3, 2, 4, 5}).reshape({N, 2 * H, 2 * W, cout});
  }
  const int64_t D = x.size(1), H = x.size(2), W = x.size(3);
  return cols.reshape({N, D, H, W, 2, 2, 2, cout}).permute({0, 1, 4, 2, 5, 3, 6, 7})
      .reshape({N, 2 * D, 2 * H, 2 * W, cout});
}
Tensor shuffle_down(const Tensor& dout) {          // -> [M][S*cout]
  const int dims = sdims(dout);
  const int64_t N = dout.size(0), co = dout.size(-1);
  if (dims == 2) {
    const int64_t H = dout.size(1) / 2, W = dout.size(2) / 2;
    return dout.reshape({N, H, 2, W, 2, co}).permute({0, 1, 3, 2, 4, 5}).reshape({N * H * W, 4 * co});
  }
  const int64_t D = dout.size(1) / 2, H = dout.size(2) / 2, W = dout.size(3) / 2;
  return dout.reshape({N, D, 2, H, 2, W, 2, co}).permute({0, 1, 3, 5, 2, 4, 6, 7})
      .reshape({N * D * H * W, 8 * co});
}
Tensor convt_input(const Tensor& x, const optional<Tensor>& bn4) {
  const int64_t C = x.size(-1);
  if (!has(bn4)) return f32(x);
  TORCH_CHECK(bn4->numel() == 4 * C, "bn4 must be [4][C] (mean, invstd, scale, shift)");
  return bn_act(f32(x), s4row(*bn4, 1, C, 2), s4row(*bn4, 1, C, 3), 1);
}

Tensor convt_fwd(const Tensor& x, const Tensor& wt, const optional<Tensor>& bias, int64_t cout,
                 const optional<Tensor>& bn4) {
  ddlpc::set_last_path("cpu");
  const int64_t C = x.size(-1);
  const Tensor xin = convt_input(x, bn4).reshape({-1, C});
  const Tensor cols = at::matmul(xin, f32(wt).reshape({-1, C}).t());
  Tensor out = shuffle_up(cols, x, cout);
  if (has(bias)) out = out + bias->reshape({cout});
  return bf(out);
}

std::vector<Tensor> convt_dgrad(const Tensor& dout, const Tensor& wd, int64_t cin, const optional<Tensor>& bny,
                                const optional<Tensor>& bn4) {
  ddlpc::set_last_path("cpu");
  const Tensor cols = shuffle_down(f32(dout));
  std::vector<int64_t> xs = dout.sizes().vec();
  for (size_t i = 1; i + 1 < xs.size(); ++i) xs[i] /= 2;
  xs.back() = cin;
  const Tensor dxf = at::matmul(cols, f32(wd).reshape({cin, -1}).t()).reshape(xs);
  const Tensor dx = bf(dxf);
  if (!has(bn4)) return {dx, empty_f(dout)};
  TORCH_CHECK(has(bny), "convt_dgrad: bny must be the deferred pre-BN input");
  return {dx, bnb_rows(dxf, f32(*bny), *bn4, 1)};
}

Tensor convt_bias(const Tensor& dout, const optional<Tensor>& colsum_rows) {
  const int64_t co = dout.size(-1);
  if (has_nonempty(colsum_rows))
    return colsum_rows->select(1, 0).narrow(1, 0, co).to(at::kDouble).sum(0).to(at::kFloat);
  return f32(dout).reshape({-1, co}).to(at::kDouble).sum(0).to(at::kFloat);
}

std::vector<Tensor> convt_wgrad(const Tensor& x, const Tensor& dout, const optional<Tensor>& dw_out,
                                const optional<Tensor>& db_out, const optional<Tensor>& colsum_rows,
                                const optional<Tensor>& bn4) {
  ddlpc::set_last_path("cpu");
  const int dims = sdims(x);
  const int64_t C = x.size(-1), co = dout.size(-1), S = dims == 2 ? 4 : 8;
  const Tensor xin = convt_input(x, bn4).reshape({-1, C});
  const Tensor cols = shuffle_down(f32(dout));                     // [M][S*co]
  std::vector<int64_t> ws = {C, co, 2, 2};
  if (dims == 3) ws.push_back(2);
  const Tensor dW = at::matmul(xin.t(), cols).reshape({C, S, co}).permute({0, 2, 1}).contiguous().reshape(ws);
  const Tensor db = convt_bias(dout, colsum_rows);
  if (has(dw_out)) {
    add_to(*dw_out, dW);
    add_to(*db_out, db);
    return {empty_f(x), empty_f(x)};
  }
  return {dW, db};
}

std::vector<Tensor> convt_bwd_fused(const Tensor& x, const Tensor& dout, const Tensor& wd,
                                    const optional<Tensor>& dw_out, const optional<Tensor>& db_out,
                                    const optional<Tensor>& colsum_rows, const optional<Tensor>& bn4) {
  ddlpc::set_last_path("cpu");
  auto r = convt_dgrad(dout, wd, x.size(-1), has(bn4) ? optional<Tensor>(x) : c10::nullopt, bn4);
  auto w = convt_wgrad(x, dout, dw_out, db_out, colsum_rows, bn4);
  return {r[0], r[1], w[0], w[1]};
}

// ------------------------------------------------------------------------ head + CE
// the head's input activation: bf16 a, or relu(bn(y)) rounded to bf16 (deferred BN,
// per group with [G][4][C] statistics)
Tensor head_act(const Tensor& a, const optional<Tensor>& bn4, int64_t G) {
  const int64_t C = a.size(-1);
  if (!has(bn4)) return f32(a).reshape({-1, C});
  return bn_act(f32(a), s4row(*bn4, G, C, 2), s4row(*bn4, G, C, 3), G).reshape({-1, C});
}

// class weights (cross_entropy(weight=)): pw = w[label] per valid pixel — 0 for a label
// outside [0, K) — multiplies the pixel's loss term and dlogits, and sum pw replaces the
// valid-pixel count (out3[2]); hits stay unweighted.  Without weights nothing is multiplied.
struct HeadFwd {
  Tensor A, logits, valid, lab, out3, pw;
};
HeadFwd head_forward(const Tensor& a, const Tensor& Wh, const Tensor& bh, const Tensor& labels,
                     int64_t ignore_index, const optional<Tensor>& bn4, int64_t G,
                     const optional<Tensor>& cw = c10::nullopt) {
  const int64_t K = Wh.size(0);
  ddlpc::set_last_path("cpu");
  HeadFwd h;
  h.A = head_act(a, bn4, G);
  h.logits = at::matmul(h.A, f32(Wh).reshape({K, -1}).t()) + f32(bh).reshape({K});
  const Tensor lab = labels.reshape({-1});
  h.valid = lab != ignore_index;
  h.lab = at::where(h.valid, lab, at::zeros_like(lab));
  const Tensor lse = at::logsumexp(h.logits, 1);
  const Tensor picked = h.logits.gather(1, h.lab.unsqueeze(1)).squeeze(1);
  Tensor ce = at::where(h.valid, lse - picked, at::zeros_like(lse)).to(at::kDouble);
  double count = h.valid.sum().item<double>();
  if (has(cw)) {
    TORCH_CHECK(cw->scalar_type() == at::kFloat && cw->dim() == 1 && cw->numel() == K,
                "class_weight must be fp32 [K] on the activation's device");
    // (the table is indexed by in-range labels only; h.lab is already 0 on ignored pixels)
    const Tensor in = h.valid & (lab >= 0) & (lab < K);
    const Tensor idx = at::where(in, lab, at::zeros_like(lab));
    h.pw = at::where(in, cw->index_select(0, idx), at::zeros_like(lse));
    h.lab = idx;
    ce = at::where(in, (lse - picked) * h.pw, at::zeros_like(lse)).to(at::kDouble);
    count = h.pw.to(at::kDouble).sum().item<double>();
  }
  const double correct = (h.logits.argmax(1) == lab).sum().item<double>();
  const double loss = count > 0 ? ce.sum().item<double>() / count : 0.0;
  h.out3 = at::tensor({(float)loss, (float)correct, (float)count}, a.options().dtype(at::kFloat));
  return h;
}
// dlogits = (softmax - onehot) * scale on valid pixels
Tensor head_dlogits(const HeadFwd& h, double scale) {
  Tensor p = at::softmax(h.logits, 1);
  p = p - at::one_hot(h.lab, h.logits.size(1)).to(at::kFloat);
  if (h.pw.defined())     // (softmax - onehot) * (scale * w): the GPU kernels' operand order
    return at::where(h.valid.unsqueeze(1), p * (h.pw * scale).unsqueeze(1), at::zeros_like(p));
  return at::where(h.valid.unsqueeze(1), p * scale, at::zeros_like(p));
}
double head_scale(const Tensor& out3, const optional<Tensor>& gs) {
  const double cnt = out3[2].item<double>();
  return scalar_or(gs, 1.0) / (cnt > 0 ? cnt : 1.0);
}
void add_into(const optional<Tensor>& dst, const Tensor& v) { add_to(*dst, v); }

Tensor head_ce_fwd(const Tensor& a, const Tensor& Wh, const Tensor& bh, const Tensor& labels,
                   int64_t ignore_index, const optional<Tensor>& bn4, const optional<Tensor>& class_weight) {
  return head_forward(a, Wh, bh, labels, ignore_index, bn4, 1, class_weight).out3;
}

std::vector<Tensor> head_ce_bwd(const Tensor& a, const Tensor& Wh, const Tensor& bh, const Tensor& labels,
                                const Tensor& out3, const optional<Tensor>& gscale, int64_t ignore_index,
                                const optional<Tensor>& dw_out, const optional<Tensor>& db_out,
                                const optional<Tensor>& bn4, bool store_da,
                                const optional<Tensor>& class_weight) {
  TORCH_CHECK(store_da || has(bn4), "head_ce_bwd: store_da=False needs the deferred BN (bn4)");
  const int64_t K = Wh.size(0), C = a.size(-1);
  const HeadFwd h = head_forward(a, Wh, bh, labels, ignore_index, bn4, 1, class_weight);
  const Tensor dl = head_dlogits(h, head_scale(out3, gscale));
  const Tensor dAf = at::matmul(dl, f32(Wh).reshape({K, C}));
  const Tensor dA = store_da ? bf(dAf.reshape(a.sizes())) : at::empty({0}, a.options());
  const Tensor dW = at::matmul(dl.t(), h.A), db = dl.sum(0);
  const Tensor bnpart = has(bn4) ? bnb_rows(rbf(dAf).reshape(a.sizes()), f32(a), *bn4, 1) : empty_f(a);
  if (has(dw_out)) {
    add_into(dw_out, dW);
    add_into(db_out, db);
    return {dA, empty_f(a), empty_f(a), bnpart};
  }
  return {dA, dW, db, bnpart};
}

std::vector<Tensor> head_ce_bn_bwd(const Tensor& a, const Tensor& Wh, const Tensor& bh, const Tensor& labels,
                                   const Tensor& out3, const optional<Tensor>& gscale, int64_t ignore_index,
                                   const Tensor& bn4, const Tensor& partial, const Tensor& gamma,
                                   const optional<Tensor>& dgamma_out, const optional<Tensor>& dbeta_out,
                                   const optional<Tensor>& pscale, int64_t groups,
                                   const optional<Tensor>& class_weight) {
  const int64_t G = groups > 1 ? groups : 1;
  const int64_t K = Wh.size(0), C = a.size(-1);
  const HeadFwd h = head_forward(a, Wh, bh, labels, ignore_index, bn4, G, class_weight);
  const Tensor dl = head_dlogits(h, head_scale(out3, gscale));
  const Tensor dAf = rbf(at::matmul(dl, f32(Wh).reshape({K, C}))).reshape(a.sizes());
  const BnBwd t = bn_terms(dAf, f32(a), bn4, G, 1.0);
  const Tensor sums = partial.reshape({G, -1, 2, C}).to(at::kDouble).sum(1) * scalar_or(pscale, 1.0);
  const bool into = has(dgamma_out);
  Tensor dgamma = into ? *dgamma_out : Tensor(), dbeta = into ? *dbeta_out : Tensor();
  const Tensor coefs = bn_coefs(sums, bn4, gamma, G, (double)(a.numel() / C / G), dgamma, dbeta, into);
  return {bn_apply_coefs(t, coefs, a, G), dgamma, dbeta};
}

std::vector<Tensor> head_ce_fwd_stats(const Tensor& a, const Tensor& Wh, const Tensor& bh, const Tensor& labels,
                                      int64_t ignore_index, const Tensor& bn4, int64_t groups,
                                      const optional<Tensor>& class_weight) {
  const int64_t G = groups > 1 ? groups : 1;
  const int64_t K = Wh.size(0), C = a.size(-1);
  const HeadFwd h = head_forward(a, Wh, bh, labels, ignore_index, bn4, G, class_weight);
  const Tensor dl = head_dlogits(h, 1.0);                   // unit gradient scale
  // (the unrounded dA, as the GPU kernels' unit-scale pass: nothing is stored here)
  const Tensor dAf = at::matmul(dl, f32(Wh).reshape({K, C})).reshape(a.sizes());
  const Tensor wrows = at::cat({at::matmul(dl.t(), h.A).reshape({-1}), dl.sum(0)}).reshape({1, K * C + K});
  return {h.out3, wrows, bnb_rows(dAf, f32(a), bn4, G)};
}

std::vector<Tensor> head_wgrad_from_rows(const Tensor& rows, const Tensor& scale, int64_t K, int64_t C,
                                         const optional<Tensor>& dw_out, const optional<Tensor>& db_out) {
  const Tensor s = (rows.to(at::kDouble).sum(0) * scale.to(at::kDouble).reshape({-1})[0]).to(at::kFloat);
  if (has(dw_out)) {
    add_into(dw_out, s.narrow(0, 0, K * C));
    add_into(db_out, s.narrow(0, K * C, K));
    return {empty_f(rows), empty_f(rows)};
  }
  return {s.narrow(0, 0, K * C).reshape({K, C}), s.narrow(0, K * C, K)};
}

Tensor head_grad_scale(const Tensor& out3, const optional<Tensor>& gs) {
  return at::tensor({(float)head_scale(out3, gs)}, out3.options());
}

void meter_add(Tensor& buf, const Tensor& loss, const Tensor& correct, double pixels, double count) {
  TORCH_CHECK(buf.scalar_type() == at::kDouble && buf.numel() == 4, "meter buffer must be 4 doubles");
  double* b = buf.data_ptr<double>();
  b[0] += loss.to(at::kDouble).item<double>() * count;
  b[1] += correct.to(at::kDouble).item<double>();
  b[2] += pixels;
  b[3] += count;
}

Tensor head_logits(const Tensor& a, const Tensor& Wh, const Tensor& bh, const optional<Tensor>& bn4) {
  const int64_t K = Wh.size(0);
  ddlpc::set_last_path("cpu");
  const Tensor A = head_act(a, bn4, 1);
  const Tensor l = at::matmul(A, f32(Wh).reshape({K, -1}).t()) + f32(bh).reshape({K});
  std::vector<int64_t> s = a.sizes().vec();
  s.back() = K;
  return to_cf(l.reshape(s)).contiguous();
}

// ------------------------------------------------------------------------ optimizer / pack
void adam_math(Tensor p, const Tensor& g, Tensor m, Tensor v, double b1, double b2, double eps, double wd,
               float step_size, float inv_sqrt_bc2) {
  float* P = p.data_ptr<float>();
  const Tensor gc = g.contiguous();
  const float* G = gc.data_ptr<float>();
  float* M = m.data_ptr<float>();
  float* V = v.data_ptr<float>();
  const float fb1 = (float)b1, fb2 = (float)b2, feps = (float)eps, fwd = (float)wd;
  const int64_t n = p.numel();
  at::parallel_for(0, n, 16384, [&](int64_t s, int64_t e) {
    for (int64_t i = s; i < e; ++i) {
      const float gr = fwd != 0.f ? G[i] + fwd * P[i] : G[i];
      M[i] = M[i] + (1.f - fb1) * (gr - M[i]);
      V[i] = fb2 * V[i] + (1.f - fb2) * gr * gr;
      P[i] = P[i] - step_size * M[i] / (std::sqrt(V[i]) * inv_sqrt_bc2 + feps);
    }
  });
}

void adam_step(Tensor p, const Tensor& g, Tensor m, Tensor v, double b1, double b2, double eps, double wd,
               double step_size, double inv_sqrt_bc2) {
  TORCH_CHECK(p.is_contiguous() && m.is_contiguous() && v.is_contiguous(), "adam: contiguous buffers");
  adam_math(p, g, m, v, b1, b2, eps, wd, (float)step_size, (float)inv_sqrt_bc2);
}

void adam_step_dev(Tensor p, const Tensor& g, Tensor m, Tensor v, Tensor scal, double lr, double b1, double b2,
                   double eps, double wd) {
  float* s = scal.data_ptr<float>();
  const double t = (double)s[0] + 1.0;
  s[0] = (float)t;
  s[1] = (float)(lr / (1.0 - std::pow(b1, t)));
  s[2] = (float)(1.0 / std::sqrt(1.0 - std::pow(b2, t)));
  adam_math(p, g, m, v, b1, b2, eps, wd, s[1], s[2]);
}

// the scheduled step of csrc/optim.hip: the same partials (workgroup b owns the float4s of
// index i with (i / 256) % nb == b, block 0 the tail; here each summed in index order, then
// the partials in order), the scalars of optim_math.h and the update of adam_sched_kernel
void adam_step_sched(Tensor p, const Tensor& g, Tensor m, Tensor v, Tensor scal, Tensor partial, double lr,
                     double b1, double b2, double eps, double wd, bool decoupled, double max_norm,
                     int64_t sched_kind, int64_t warmup, int64_t total, double lr_min, double power) {
  for (const Tensor* t : std::array<const Tensor*, 4>{&p, &g, &m, &v})
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == p.numel(),
                "adam: p, g, m, v must be contiguous fp32 buffers of one size");
  TORCH_CHECK(scal.scalar_type() == at::kFloat && scal.numel() == 8 && scal.is_contiguous(),
              "scal must be float[8]");
  const int64_t n = p.numel();
  const int nblk = ddlpc::grad_sqnorm_blocks(n);
  TORCH_CHECK(partial.scalar_type() == at::kDouble && partial.is_contiguous() && partial.numel() >= nblk,
              "partial must be double[>= grad_sqnorm_blocks(n)]");
  TORCH_CHECK(sched_kind >= 0 && sched_kind <= 2, "sched_kind: 0 constant, 1 poly, 2 cosine");
  TORCH_CHECK(warmup >= 0 && total >= 0, "warmup and total must be >= 0");
  const float* G = g.data_ptr<float>();
  double sq = 0.0;
  if (max_norm > 0.0 && nblk > 0) {
    double* part = partial.data_ptr<double>();
    for (int b = 0; b < nblk; ++b) part[b] = 0.0;
    const int64_t n4 = n / 4;
    for (int64_t i = 0; i < n4; ++i) {
      double& acc = part[(i / 256) % nblk];
      for (int j = 0; j < 4; ++j) acc += (double)G[4 * i + j] * (double)G[4 * i + j];
    }
    for (int64_t i = n4 * 4; i < n; ++i) part[0] += (double)G[i] * (double)G[i];
    for (int b = 0; b < nblk; ++b) sq += part[b];
  }
  float* s = scal.data_ptr<float>();
  const ddlpc::SchedArgs a{lr, b1, b2, wd, max_norm, lr_min, power, warmup, total, (int)sched_kind,
                           decoupled ? 1 : 0};
  ddlpc::sched_scalars(s, a, sq);
  if (n == 0) return;
  float* P = p.data_ptr<float>();
  float* M = m.data_ptr<float>();
  float* V = v.data_ptr<float>();
  const float fb1 = (float)b1, fb2 = (float)b2, feps = (float)eps, fwd = (float)wd;
  const float step_size = s[1], inv_sqrt_bc2 = s[2], coef = s[5], keep = 1.f - s[6];
  at::parallel_for(0, n, 16384, [&](int64_t lo, int64_t hi) {
#pragma clang fp contract(off)
    for (int64_t i = lo; i < hi; ++i) {
      const float gc = G[i] * coef;
      float gr, p0 = P[i];
      if (decoupled) { gr = gc; p0 = p0 * keep; }
      else gr = fwd != 0.f ? gc + fwd * p0 : gc;
      M[i] = M[i] + (1.f - fb1) * (gr - M[i]);
      V[i] = fb2 * V[i] + (1.f - fb2) * gr * gr;
      P[i] = p0 - step_size * M[i] / (std::sqrt(V[i]) * inv_sqrt_bc2 + feps);
    }
  });
}

// fp32 OIHW / IOHW parameters -> bf16 kernel layouts (see csrc/misc.hip weight_pack_kernel):
// entries [n][6] = (src*, fwd*, dgrad* | 0, kind | Cout << 32, Cin | taps << 32, CinW | CoutW << 32)
void weight_pack(const Tensor& entries, int64_t n, int64_t max_elems) {
  (void)max_elems;
  TORCH_CHECK(entries.scalar_type() == at::kLong && entries.numel() == n * 6, "entries must be int64 [n, 6]");
  const Tensor e = entries.contiguous();
  const int64_t* ep = e.data_ptr<int64_t>();
  for (int64_t i = 0; i < n; ++i) {
    const int64_t* r = ep + 6 * i;
    const float* src = reinterpret_cast<const float*>(r[0]);
    auto* fwd = reinterpret_cast<c10::BFloat16*>(r[1]);
    auto* dgr = reinterpret_cast<c10::BFloat16*>(r[2]);
    const int kind = (int)(r[3] & 0xffffffff);
    const int64_t Cout = (int64_t)((uint64_t)r[3] >> 32), Cin = r[4] & 0xffffffff;
    const int64_t T = (int64_t)((uint64_t)r[4] >> 32), CinW = r[5] & 0xffffffff;
    const int64_t CoutW = (int64_t)((uint64_t)r[5] >> 32);
    if (kind == 0) {                  // OIHW [co][ci][tap]
      for (int64_t co = 0; co < Cout; ++co)
        for (int64_t ci = 0; ci < Cin; ++ci)
          for (int64_t t = 0; t < T; ++t) {
            const float v = src[(co * Cin + ci) * T + t];
            fwd[(co * T + t) * CinW + ci] = c10::BFloat16(v);
            if (dgr != nullptr) dgr[(ci * T + (T - 1 - t)) * CoutW + co] = c10::BFloat16(v);
          }
    } else {                          // IOHW [ci][co][sub]
      for (int64_t ci = 0; ci < Cin; ++ci)
        for (int64_t co = 0; co < Cout; ++co)
          for (int64_t s = 0; s < T; ++s) {
            const float v = src[(ci * Cout + co) * T + s];
            fwd[(s * Cout + co) * Cin + ci] = c10::BFloat16(v);
            if (dgr != nullptr) dgr[(ci * T + s) * Cout + co] = c10::BFloat16(v);
          }
    }
  }
}

// ------------------------------------------------------------------------ codec
std::vector<std::pair<int64_t, int64_t>> segments(const Tensor& seg) {
  const Tensor s = seg.to(at::kLong).contiguous();
  const int64_t* p = s.data_ptr<int64_t>();
  std::vector<std::pair<int64_t, int64_t>> out;
  for (int64_t i = 0; i + 1 < s.numel(); i += 2) out.emplace_back(p[i], p[i + 1]);
  return out;
}

Tensor codec_absmax(const Tensor& x, const Tensor& seg) {
  const auto segs = segments(seg);
  Tensor s = at::zeros({(int64_t)segs.size()}, x.options());
  for (size_t k = 0; k < segs.size(); ++k)
    if (segs[k].second > segs[k].first)
      s[k] = x.narrow(0, segs[k].first, segs[k].second - segs[k].first).abs().max();
  return s;
}

Tensor codec_encode(const Tensor& x, const Tensor& seg, const Tensor& scales, int64_t codec) {
  const auto segs = segments(seg);
  const float L = codec == 0 ? 100.f : 10.f;
  Tensor out = at::zeros({x.numel()}, x.options().dtype(codec == 0 ? at::kHalf : at::kChar));
  const Tensor sc = scales.contiguous();
  for (size_t k = 0; k < segs.size(); ++k) {
    const int64_t a = segs[k].first, len = segs[k].second - segs[k].first;
    const float s = sc.data_ptr<float>()[k];
    if (len <= 0 || !(s > 0.f) || std::isinf(s)) continue;        // zero / NaN / Inf scale: zeros
    const Tensor q = at::round(x.narrow(0, a, len) / s * L);      // round half to even
    out.narrow(0, a, len).copy_(q);
  }
  return out;
}

void codec_decode_sum(Tensor out, const Tensor& q, const Tensor& scales, const Tensor& w, const Tensor& seg,
                      int64_t codec) {
  const auto segs = segments(seg);
  const float L = codec == 0 ? 100.f : 10.f;
  const int64_t world = q.size(0), n = out.numel();
  const Tensor sc = scales.reshape({world, -1});
  const Tensor qf = f32(q.reshape({world, n}));
  for (size_t k = 0; k < segs.size(); ++k) {
    const int64_t a = segs[k].first, len = segs[k].second - segs[k].first;
    if (len <= 0) continue;
    Tensor acc = at::zeros({len}, out.options());
    for (int64_t r = 0; r < world; ++r)
      acc = acc + w[r] * (qf[r].narrow(0, a, len) / L * sc[r][(int64_t)k]);
    out.narrow(0, a, len).copy_(acc);
  }
}

// ------------------------------------------------------------------------ misc
Tensor bilinear_up2(const Tensor& x) {
  const Tensor xc = to_cf(f32(x)).contiguous();
  Tensor y;
  if (x.dim() == 4)
    y = at::upsample_bilinear2d(xc, {2 * x.size(1), 2 * x.size(2)}, true);
  else
    y = at::upsample_trilinear3d(xc, {2 * x.size(1), 2 * x.size(2), 2 * x.size(3)}, true);
  return bf(to_cl(y));
}

Tensor bilinear_up2_bwd(const Tensor& dy) {
  const Tensor g = to_cf(f32(dy)).contiguous();
  Tensor dx;
  if (dy.dim() == 4) {
    const int64_t H = dy.size(1) / 2, W = dy.size(2) / 2;
    dx = at::upsample_bilinear2d_backward(g, {2 * H, 2 * W}, {dy.size(0), dy.size(3), H, W}, true);
  } else {
    const int64_t D = dy.size(1) / 2, H = dy.size(2) / 2, W = dy.size(3) / 2;
    dx = at::upsample_trilinear3d_backward(g, {2 * D, 2 * H, 2 * W}, {dy.size(0), dy.size(4), D, H, W}, true);
  }
  return bf(to_cl(dx));
}

Tensor to_nhwc_bf16(const Tensor& x, int64_t cpad) {
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "fp32/bf16 input");
  const int64_t C = x.size(1), Cp = (C + cpad - 1) / cpad * cpad;
  Tensor y = to_cl(x.to(at::kBFloat16));
  if (Cp > C) y = at::constant_pad_nd(y, {0, Cp - C}, 0);
  return y.contiguous();
}

// ------------------------------------------------------------------------ input pipeline
// The CPU twins of data.hip / scene.hip: loops around the recipe of data_math.h behind the checks
// of data_checks.h (synth_tiles spells its recipe as synth_tiles_kernel does, line for line).

// 8 channel values -> cpad bf16 (channels at and above in_ch are zero)
void store_px(c10::BFloat16* o, const float* f, int64_t cpad) {
  for (int64_t c = 0; c < cpad; ++c) o[c] = c10::BFloat16(f[c]);
}

std::vector<Tensor> synth_tiles(const Tensor& idx, int64_t seed, int64_t classes, int64_t in_ch, int64_t tile,
                                int64_t dims, int64_t grid, double k, const Tensor& palette, int64_t cpad) {
  checks::synth_tiles(idx, classes, in_ch, tile, dims, grid, palette, cpad);
  const Tensor ix = idx.contiguous(), pal = palette.contiguous();
  const int64_t B = ix.numel();
  const int64_t S = dims == 3 ? tile * tile * tile : tile * tile;
  std::vector<int64_t> ys = {B};
  for (int i = 0; i < dims; ++i) ys.push_back(tile);
  Tensor y = at::empty(ys, idx.options());
  std::vector<int64_t> xs = ys;
  xs.push_back(cpad);
  Tensor x = at::empty(xs, idx.options().dtype(at::kBFloat16));
  const float* pp = pal.data_ptr<float>();
  const int64_t* ip = ix.data_ptr<int64_t>();
  int64_t* yp = y.data_ptr<int64_t>();
  auto* xp = x.data_ptr<c10::BFloat16>();
  const uint32_t skey = mix32((uint32_t)(seed & 0xffffffff) ^ 0x9E3779B9u);
  const float kf = (float)k;
  const int64_t g = grid;
  at::parallel_for(0, B * S, 4096, [&](int64_t s0, int64_t s1) {
    for (int64_t e = s0; e < s1; ++e) {
      const int64_t b = e / S, p = e - b * S;
      const int64_t w = p % tile, h = (p / tile) % tile, d = dims == 3 ? p / tile / tile : 0;
      const uint32_t key = mix32(skey ^ (uint32_t)ip[b]);
      const uint32_t cell = (uint32_t)((d * g / tile * g + h * g / tile) * g + w * g / tile);
      const int lab = (int)(mix32(key ^ mix32(cell + 0x632BE5ABu)) % (uint32_t)classes);
      yp[e] = lab;
      float f[8] = {};
      for (int c = 0; c < in_ch; ++c) {
        const uint32_t base = key ^ mix32((uint32_t)(p * 8 + c) + 0x1B873593u);
        float s = u24(mix32(base));
        s = add_rn(s, u24(mix32(base + 0x9E3779B9u)));
        s = add_rn(s, u24(mix32(base + 2u * 0x9E3779B9u)));
        s = add_rn(s, u24(mix32(base + 3u * 0x9E3779B9u)));
        f[c] = fminf(fmaxf(add_rn(pp[lab * in_ch + c], mul_rn(add_rn(s, -2.0f), kf)), 0.f), 1.f);
      }
      store_px(xp + e * cpad, f, cpad);
    }
  });
  return {x, y};
}

std::vector<Tensor> tile_gather(const Tensor& src, const Tensor& lab, const Tensor& idx, int64_t cpad) {
  checks::tile_gather(src, lab, idx, cpad);
  const int64_t in_ch = src.size(-1), N = lab.size(0);
  const Tensor ix = idx.contiguous();
  const int64_t B = ix.numel();
  const int64_t S = lab.numel() / std::max<int64_t>(1, N);
  std::vector<int64_t> ys = {B};
  for (int64_t i = 1; i < lab.dim(); ++i) ys.push_back(lab.size(i));
  Tensor y = at::empty(ys, idx.options());
  std::vector<int64_t> xs = ys;
  xs.push_back(cpad);
  Tensor x = at::empty(xs, src.options().dtype(at::kBFloat16));
  const Tensor sc = src.contiguous(), lc = lab.contiguous();
  const uint8_t *sp = sc.data_ptr<uint8_t>(), *lp = lc.data_ptr<uint8_t>();
  const int64_t* ip = ix.data_ptr<int64_t>();
  int64_t* yp = y.data_ptr<int64_t>();
  auto* xp = x.data_ptr<c10::BFloat16>();
  for (int64_t e = 0; e < B * S; ++e) {
    const int64_t b = e / S, p = e - b * S, n = ip[b];
    const bool in_range = n >= 0 && n < N;      // out of range reads nothing: zero image, label -100
    const int64_t q = in_range ? n * S + p : 0;
    yp[e] = in_range ? (int64_t)lp[q] : (int64_t)-100;
    float f[8] = {};
    for (int c = 0; c < in_ch && in_range; ++c) f[c] = u8_unit(sp[q * in_ch + c]);
    store_px(xp + e * cpad, f, cpad);
  }
  return {x, y};
}

// ------------------------------------------------------------------------ scene prediction
// test-time augmentation: the symmetry codes of a call -> the list, {0} (the plain window) without
std::vector<int> codes_of(const optional<Tensor>& codes, const Tensor& like) {
  const int64_t S = checks::codes(codes, like);
  if (!has(codes)) return {0};
  const uint32_t packed = checks::pack_code_values(codes->contiguous().data_ptr<int>(), S);
  std::vector<int> out(S);
  for (int64_t j = 0; j < S; ++j) out[j] = (int)((packed >> (3 * j)) & 7u);
  return out;
}

Tensor window_gather(const Tensor& scene, const Tensor& origins, int64_t tile, int64_t cpad,
                     const optional<Tensor>& codes) {
  checks::window_gather(scene, origins, tile, cpad);
  const int64_t H = scene.size(0), W = scene.size(1), in_ch = scene.size(2), B = origins.size(0);
  const Tensor sc = scene.contiguous(), oc = origins.contiguous();
  const uint8_t* sp = sc.data_ptr<uint8_t>();
  const int* op = oc.data_ptr<int>();
  const std::vector<int> cs = codes_of(codes, scene);
  const int64_t S = (int64_t)cs.size();
  Tensor x = at::empty({B * S, tile, tile, cpad}, scene.options().dtype(at::kBFloat16));
  auto* xp = x.data_ptr<c10::BFloat16>();
  for (int64_t v = 0; v < B * S; ++v) {
    const int64_t b = v / S;
    const int code = cs[v - b * S];
    for (int64_t oy = 0; oy < tile; ++oy)
      for (int64_t ox = 0; ox < tile; ++ox) {
        const Index2<int64_t> s = d4_forward(code, tile, oy, ox);
        const uint8_t* q = sp + (reflect_fast(op[2 * b] + s.a, H) * W + reflect_fast(op[2 * b + 1] + s.b, W)) * in_ch;
        float f[8] = {};
        for (int64_t ch = 0; ch < in_ch; ++ch) f[ch] = u8_unit(q[ch]);
        store_px(xp + ((v * tile + oy) * tile + ox) * cpad, f, cpad);
      }
  }
  return x;
}

// ------------------------------------------------------------------------ augmented crops
std::vector<Tensor> crop_params(const Tensor& idx, const Tensor& cum, const Tensor& table, int64_t seed,
                                int64_t tile, int64_t mode, double gain_jitter, double bias_jitter) {
  checks::params_args("crop_params", idx, cum, table, tile, mode);
  const Tensor ix = idx.contiguous(), cc = cum.contiguous(), tc = table.contiguous();
  const int64_t B = ix.numel();
  const int n = (int)table.size(0);
  const int64_t *ip = ix.data_ptr<int64_t>(), *cp = cc.data_ptr<int64_t>(), *tp = tc.data_ptr<int64_t>();
  Tensor params = at::empty({B, 4}, idx.options().dtype(at::kInt));
  Tensor color = at::empty({B, 2}, idx.options().dtype(at::kFloat));
  int* pp = params.data_ptr<int>();
  float* op = color.data_ptr<float>();
  for (int64_t i = 0; i < B; ++i) {
    const uint32_t key = sample_key((uint32_t)(seed & 0xffffffff), (uint64_t)ip[i]);
    const int lo = pick_scene(cp, n, draw(key, 0));
    pp[4 * i] = lo;
    pp[4 * i + 1] = (int)scale_draw(draw(key, 1), origin_count(tp[3 * lo + 1], tile));
    pp[4 * i + 2] = (int)scale_draw(draw(key, 2), origin_count(tp[3 * lo + 2], tile));
    pp[4 * i + 3] = symmetry_code(draw(key, 3), (int)mode);
    color_jitter(draw(key, 4), draw(key, 5), (float)gain_jitter, (float)bias_jitter, op + 2 * i);
  }
  return {params, color};
}

// the rows of warp_gather (arguments checked by the caller); bounded: a row must pass warp_row_valid
std::vector<Tensor> gather_rows(const Tensor& scenes, const Tensor& labels, const Tensor& table,
                                const Tensor& wparams, const optional<Tensor>& color, int64_t tile,
                                int64_t cpad, bool bounded) {
  const int64_t in_ch = scenes.size(1), B = wparams.size(0), n = table.size(0), P = labels.size(0);
  const bool has_color = has(color);
  const Tensor cc = has_color ? color->contiguous() : Tensor();
  const Tensor sc = scenes.contiguous(), lc = labels.contiguous(), tc = table.contiguous(),
               wc = wparams.contiguous();
  const uint8_t *sp = sc.data_ptr<uint8_t>(), *lp = lc.data_ptr<uint8_t>();
  const int64_t *tp = tc.data_ptr<int64_t>(), *wp = wc.data_ptr<int64_t>();
  const float* cp = has_color ? cc.data_ptr<float>() : nullptr;
  Tensor y = at::empty({B, tile, tile}, scenes.options().dtype(at::kLong));
  Tensor x = at::empty({B, tile, tile, cpad}, scenes.options().dtype(at::kBFloat16));
  int64_t* yp = y.data_ptr<int64_t>();
  auto* xp = x.data_ptr<c10::BFloat16>();
  at::parallel_for(0, B * tile, 16, [&](int64_t row0, int64_t row1) {
    for (int64_t row = row0; row < row1; ++row) {
      const int64_t b = row / tile;
      const int oy = (int)(row - b * tile);
      const int64_t* w = wp + 6 * b;
      const int64_t cy = w[1], cx = w[2];
      const int code = (int)w[3] & 7;
      const bool listed = w[0] >= 0 && w[0] < n;
      const int64_t* t = tp + (listed ? 3 * w[0] : 0);
      const int64_t off = listed ? t[0] : 0, H = listed ? t[1] : 1, W = listed ? t[2] : 1;
      const bool valid = scene_row_valid(listed, off, H, W, P) && (!bounded || warp_row_valid(w[4], w[5], cy, cx));
      const int A = valid ? (int)w[4] : 0, Bm = valid ? (int)w[5] : 0;
      const float gain = has_color ? cp[2 * b] : 1.f, bias = has_color ? cp[2 * b + 1] : 0.f;
      for (int ox = 0; ox < tile; ++ox) {
        const int64_t e = row * tile + ox;
        float f[8] = {};
        yp[e] = -100;
        if (valid) {
          const Index2<int> s = d4_forward(code, (int)tile, oy, ox);
          const Index2<long long> p = warp_coord(cy, cx, A, Bm, (int)tile, s.a, s.b);
          const int64_t iy = warp_tap(p.a), ix = warp_tap(p.b);
          const float wy = warp_weight(p.a), wx = warp_weight(p.b);
          const int64_t r0 = off + reflect_fast(iy, H) * W, r1 = off + reflect_fast(iy + 1, H) * W;
          const int64_t c0 = reflect_fast(ix, W), c1 = reflect_fast(ix + 1, W);
          for (int64_t ch = 0; ch < in_ch; ++ch) {
            const float p00 = (float)sp[(r0 + c0) * in_ch + ch], p01 = (float)sp[(r0 + c1) * in_ch + ch];
            const float p10 = (float)sp[(r1 + c0) * in_ch + ch], p11 = (float)sp[(r1 + c1) * in_ch + ch];
            f[ch] = div_rn(bilinear(p00, p01, p10, p11, wx, wy), 255.0f);
            if (has_color) f[ch] = color_clamp(f[ch], gain, bias);
          }
          yp[e] = (int64_t)lp[off + reflect_fast<int64_t>(warp_nearest(p.a), H) * W +
                              reflect_fast<int64_t>(warp_nearest(p.b), W)];
        }
        store_px(xp + e * cpad, f, cpad);
      }
    }
  });
  return {x, y};
}

std::vector<Tensor> warp_gather(const Tensor& scenes, const Tensor& labels, const Tensor& table,
                                const Tensor& wparams, const optional<Tensor>& color, int64_t tile,
                                int64_t cpad) {
  checks::warp_gather(scenes, labels, table, wparams, color, tile, cpad);
  return gather_rows(scenes, labels, table, wparams, color, tile, cpad, true);
}

// (A, Bm) = (ONE, 0), cy = (2 y0 + tile - 1) * 32768: the (y0, x0) crop bit for bit, any int32 origin
std::vector<Tensor> crop_gather(const Tensor& scenes, const Tensor& labels, const Tensor& table,
                                const Tensor& params, const optional<Tensor>& color, int64_t tile,
                                int64_t cpad) {
  checks::crop_gather(scenes, labels, table, params, color, tile, cpad);
  const Tensor p = params.to(at::kLong), one = at::full_like(p.slice(1, 0, 1), 65536);
  const Tensor w = at::cat({p.slice(1, 0, 1), (2 * p.slice(1, 1, 3) + (tile - 1)) * 32768, p.slice(1, 3, 4), one,
                            at::zeros_like(one)}, 1);
  return gather_rows(scenes, labels, table, w, color, tile, cpad, false);
}

std::vector<Tensor> warp_params(const Tensor& idx, const Tensor& cum, const Tensor& table, const Tensor& steps,
                                const Tensor& rot, int64_t seed, int64_t tile, int64_t mode, double gain_jitter,
                                double bias_jitter) {
  checks::warp_params(idx, cum, table, steps, rot, tile, mode);
  const Tensor ix = idx.contiguous(), cc = cum.contiguous(), tc = table.contiguous(), stc = steps.contiguous(),
               rc = rot.contiguous();
  const int64_t B = ix.numel(), S = steps.size(0), T = rot.size(0);
  const int n = (int)table.size(0);
  const int64_t *ip = ix.data_ptr<int64_t>(), *cp = cc.data_ptr<int64_t>(), *tp = tc.data_ptr<int64_t>();
  const int *stp = stc.data_ptr<int>(), *rp = rc.data_ptr<int>();
  Tensor wparams = at::empty({B, 6}, idx.options().dtype(at::kLong));
  Tensor color = at::empty({B, 2}, idx.options().dtype(at::kFloat));
  float* op = color.data_ptr<float>();
  for (int64_t i = 0; i < B; ++i) {
    const uint32_t key = sample_key((uint32_t)(seed & 0xffffffff), (uint64_t)ip[i]);
    const int lo = pick_scene(cp, n, draw(key, 0));
    const long long step = stp[scale_draw(draw(key, 6), (uint64_t)S)];
    const uint64_t k = scale_draw(draw(key, 7), (uint64_t)T);
    const long long F = footprint((int)tile, step);
    int64_t* w = wparams.data_ptr<int64_t>() + 6 * i;
    w[0] = lo;
    w[1] = footprint_centre(draw(key, 1), tp[3 * lo + 1], F);
    w[2] = footprint_centre(draw(key, 2), tp[3 * lo + 2], F);
    w[3] = symmetry_code(draw(key, 3), (int)mode);
    w[4] = matrix_entry(step, rp[2 * k]);
    w[5] = matrix_entry(step, rp[2 * k + 1]);
    color_jitter(draw(key, 4), draw(key, 5), (float)gain_jitter, (float)bias_jitter, op + 2 * i);
  }
  return {wparams, color};
}

void head_predict_accum(const Tensor& a, const Tensor& Wh, const Tensor& bh, const Tensor& origins,
                        const Tensor& win, Tensor& acc, const optional<Tensor>& bn4,
                        const optional<Tensor>& codes) {
  const std::vector<int> cs = codes_of(codes, a);
  const int64_t S = (int64_t)cs.size();
  checks::head_predict_accum(a, Wh, bh, origins, win, acc, S);
  TORCH_CHECK(acc.is_contiguous(), "acc must be contiguous");
  const int64_t B = a.size(0) / S, tile = a.size(1), K = Wh.size(0), C = a.size(3);
  TORCH_CHECK(K >= 1 && K <= 16 && (C == 8 || C == 16 || C == 32 || C == 64), "head kernel: unsupported (C, K)");
  const int64_t H = acc.size(0), W = acc.size(1), KA = acc.size(2);
  const Tensor A = head_act(a, bn4, 1);
  const Tensor l = (at::matmul(A, f32(Wh).reshape({K, -1}).t()) + f32(bh).reshape({K})).contiguous();
  const Tensor oc = origins.contiguous(), wc = win.contiguous();
  const float* lp = l.data_ptr<float>();
  const int* op = oc.data_ptr<int>();
  const float* wp = wc.data_ptr<float>();
  float* ap = acc.data_ptr<float>();
  // one update per window-frame pixel (wa, wb): the S views through the inverse index map,
  // their softmaxes summed in ascending j, acc += (w2 / S) * sum
  const float fS = (float)S;
  for (int64_t b = 0; b < B; ++b)
    for (int64_t wa = 0; wa < tile; ++wa) {
      const int64_t sy = op[2 * b] + wa;
      if (sy < 0 || sy >= H) continue;
      for (int64_t wb = 0; wb < tile; ++wb) {
        const int64_t sx = op[2 * b + 1] + wb;
        const float w2 = wp[wa] * wp[wb];
        if (sx < 0 || sx >= W || w2 == 0.f) continue;
        float sum[16];
        for (int64_t j = 0; j < S; ++j) {
          const Index2<int64_t> o = d4_inverse(cs[j], tile, wa, wb);
          const float* z = lp + (((b * S + j) * tile + o.a) * tile + o.b) * K;
          float m = z[0], e[16], se = 0.f;
          for (int64_t k = 1; k < K; ++k) m = std::max(m, z[k]);
          for (int64_t k = 0; k < K; ++k) {
            e[k] = std::exp(z[k] - m);
            se += e[k];
          }
          for (int64_t k = 0; k < K; ++k) sum[k] = j == 0 ? e[k] / se : sum[k] + e[k] / se;
        }
        const float wS = w2 / fS;
        float* o = ap + (sy * W + sx) * KA;
        for (int64_t k = 0; k < K; ++k) o[k] += wS * sum[k];
        o[K] += w2;
      }
    }
}

std::vector<Tensor> scene_finalize(const Tensor& acc, int64_t K, const optional<Tensor>& labels,
                                   int64_t ignore_index) {
  checks::scene_finalize(acc, K, labels);
  const int64_t H = acc.size(0), W = acc.size(1), KA = acc.size(2);
  const Tensor ac = acc.contiguous();
  const float* ap = ac.data_ptr<float>();
  Tensor pred = at::empty({H, W}, acc.options().dtype(at::kByte));
  Tensor cm = at::zeros({K, K}, acc.options().dtype(at::kLong));
  uint8_t* pp = pred.data_ptr<uint8_t>();
  int64_t* cp = cm.data_ptr<int64_t>();
  Tensor lc;
  const uint8_t* lp = nullptr;
  if (has(labels)) {
    lc = labels->contiguous();
    lp = lc.data_ptr<uint8_t>();
  }
  for (int64_t px = 0; px < H * W; ++px) {
    const float* z = ap + px * KA;
    int64_t am = 0;
    for (int64_t k = 1; k < K; ++k)
      if (z[k] > z[am]) am = k;
    pp[px] = (uint8_t)am;
    if (lp != nullptr && lp[px] < K && lp[px] != ignore_index) cp[lp[px] * K + am] += 1;
  }
  return {pred, cm};
}

}  // namespace
}  // namespace ddlpc_cpu

TORCH_LIBRARY_IMPL(ddlpc, CPU, m) {
  using namespace ddlpc_cpu;
  m.impl("conv3_fwd", &conv3_fwd);
  m.impl("conv3_wgrad", &conv3_wgrad);
  m.impl("conv3_bwd32", &conv3_bwd32);
  m.impl("reduce_rows", &reduce_rows);
  m.impl("reduce_rows_scatter", &reduce_rows_scatter);
  m.impl("bn_finalize", &bn_finalize);
  m.impl("bn_relu_apply", &bn_relu_apply);
  m.impl("bn_running_apply", &bn_running_apply);
  m.impl("bn_grad_coefs", &bn_grad_coefs);
  m.impl("bn_group_finalize", &bn_group_finalize);
  m.impl("bn_group_apply", &bn_group_apply);
  m.impl("bn_running_apply_all", &bn_running_apply_all);
  m.impl("bn_group_backward", &bn_group_backward);
  m.impl("bn_group_finalize_rows", &bn_group_finalize_rows);
  m.impl("bn_backward", &bn_backward);
  m.impl("convt_fwd", &convt_fwd);
  m.impl("convt_dgrad", &convt_dgrad);
  m.impl("convt_wgrad", &convt_wgrad);
  m.impl("convt_bwd_fused", &convt_bwd_fused);
  m.impl("head_ce_fwd", &head_ce_fwd);
  m.impl("head_ce_bwd", &head_ce_bwd);
  m.impl("head_ce_bn_bwd", &head_ce_bn_bwd);
  m.impl("head_ce_fwd_stats", &head_ce_fwd_stats);
  m.impl("head_wgrad_from_rows", &head_wgrad_from_rows);
  m.impl("meter_add", &meter_add);
  m.impl("head_grad_scale", &head_grad_scale);
  m.impl("head_logits", &head_logits);
  m.impl("adam_step", &adam_step);
  m.impl("adam_step_dev", &adam_step_dev);
  m.impl("adam_step_sched", &adam_step_sched);
  m.impl("weight_pack", &weight_pack);
  m.impl("codec_absmax", &codec_absmax);
  m.impl("codec_encode", &codec_encode);
  m.impl("codec_decode_sum", &codec_decode_sum);
  m.impl("bilinear_up2", &bilinear_up2);
  m.impl("bilinear_up2_bwd", &bilinear_up2_bwd);
  m.impl("to_nhwc_bf16", &to_nhwc_bf16);
  m.impl("synth_tiles", &synth_tiles);
  m.impl("tile_gather", &tile_gather);
  m.impl("window_gather", &window_gather);
  m.impl("crop_gather", &crop_gather);
  m.impl("crop_params", &crop_params);
  m.impl("warp_gather", &warp_gather);
  m.impl("warp_params", &warp_params);
  m.impl("head_predict_accum", &head_predict_accum);
  m.impl("scene_finalize", &scene_finalize);
}
