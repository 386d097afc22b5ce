// Argument checks of the top-k and low-rank gradient codec operators, one function per operator, called by both
// registrations (bindings.cpp, cpu_ref.cpp).  The kernels index with 32-bit integers and write
// through raw pointers, so sizes, dtypes and k are refused here before any launch.  What depends
// on the backend stays with it: is_cuda.
#pragma once

#include <algorithm>
#include <initializer_list>
#include <utility>
#include <vector>

#include "data_checks.h"      // T
#include "powersgd_math.h"

namespace ddlpc {
namespace checks {

inline void flat_f32(const char* op, const char* name, T t) {
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.dim() == 1 && t.is_contiguous(), op, ": ", name,
              " must be a contiguous 1-D fp32 tensor");
}

// g, residual: n fp32 elements each; 1 <= k <= n < 2^31
inline void topk_encode(T g, T residual, int64_t k) {
  flat_f32("topk_encode", "g", g);
  flat_f32("topk_encode", "residual", residual);
  TORCH_CHECK(residual.numel() == g.numel() && residual.device() == g.device(),
              "topk_encode: residual must have g's size and device");
  TORCH_CHECK(g.numel() < (1LL << 31), "topk_encode: n must be below 2^31");
  TORCH_CHECK(k >= 1 && k <= g.numel(), "topk_encode: 1 <= k <= n, got k = ", k, ", n = ", g.numel());
}

// out fp32 [n]; idx int32 [W][k] (each row ascending, values in [0, n)); val fp32 [W][k]; w fp32 [W]
inline void topk_decode_sum(T out, T idx, T val, T w) {
  flat_f32("topk_decode_sum", "out", out);
  TORCH_CHECK(out.numel() >= 1 && out.numel() < (1LL << 31), "topk_decode_sum: 1 <= n < 2^31");
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.dim() == 2 && idx.is_contiguous() && idx.size(0) >= 1 &&
              idx.size(1) >= 1 && idx.size(1) <= out.numel(),
              "topk_decode_sum: idx must be contiguous int32 [W][k] with 1 <= k <= n");
  TORCH_CHECK(val.scalar_type() == at::kFloat && val.is_contiguous() && val.sizes() == idx.sizes(),
              "topk_decode_sum: val must be contiguous fp32 of idx's shape");
  TORCH_CHECK(w.scalar_type() == at::kFloat && w.is_contiguous() && w.numel() == idx.size(0),
              "topk_decode_sum: w must hold W fp32 weights");
  TORCH_CHECK(idx.device() == out.device() && val.device() == out.device() && w.device() == out.device(),
              "topk_decode_sum: tensors on different devices");
}

// ---- low-rank codec (powersgd.hip).  The kernels address g / e / wire_p / wire_q by the tables'
// values, so the shapes are refused by psgd_args and every row by psgd_tables before any launch;
// how the tables' values reach the host stays with the backend (the GPU binding copies a table once).

// the fp32 buffers of one call (all on the first one's device, below 2^31 elements), the tables
// (low int32 [T][5], raw int32 [R][3] or absent) and the rank
inline void psgd_args(const char* op, std::initializer_list<std::pair<const char*, const at::Tensor*>> bufs,
                      T low, const at::Tensor* raw, int64_t rank) {
  const at::Tensor& first = *bufs.begin()->second;
  for (const auto& b : bufs) {
    flat_f32(op, b.first, *b.second);
    TORCH_CHECK(b.second->device() == first.device() && b.second->numel() < (1LL << 31), op, ": ", b.first,
                " must be on ", bufs.begin()->first, "'s device and hold fewer than 2^31 elements");
  }
  TORCH_CHECK(rank >= 1 && rank <= kPsgdMaxRank, op, ": 1 <= rank <= ", kPsgdMaxRank, ", got ", rank);
  TORCH_CHECK(low.scalar_type() == at::kInt && low.dim() == 2 && low.size(1) == 5 && low.is_contiguous() &&
              low.device() == first.device(), op, ": low must be contiguous int32 [T][5] on the buffers' device");
  if (raw)
    TORCH_CHECK(raw->scalar_type() == at::kInt && raw->dim() == 2 && raw->size(1) == 3 && raw->is_contiguous() &&
                raw->device() == first.device(), op, ": raw must be contiguous int32 [R][3] on the buffers' device");
}

// the tables' values (host pointers) against ng floats of gradient / residual, np of wire_p and nq
// of a Q buffer (-1: the operator has no such buffer): every row inside its buffers, no two rows
// on one element of the bucket or of wire_p or of the Q buffer -> the launches' item counts
inline PsgdCounts psgd_tables(const char* op, const int* low, int64_t Tn, const int* raw, int64_t Rn, int64_t ng,
                              int64_t np, int64_t nq, int64_t rank) {
  PsgdCounts c;
  std::vector<std::pair<int64_t, int64_t>> in_g, in_p, in_q;
  for (int64_t t = 0; t < Tn; ++t) {
    const int64_t off = low[5 * t], n = low[5 * t + 1], m = low[5 * t + 2], po = low[5 * t + 3], qo = low[5 * t + 4];
    TORCH_CHECK(off >= 0 && n >= 1 && m >= 1 && po >= 0 && qo >= 0 && n * m < (1LL << 31), op, ": low row ", t,
                " must hold offsets >= 0 and 1 <= n, m with n m < 2^31");
    TORCH_CHECK((ng < 0 || n * m <= ng - off) && (np < 0 || n * rank <= np - po) && (nq < 0 || m * rank <= nq - qo),
                op, ": low row ", t, " (offset ", off, ", ", n, " x ", m, ", p_off ", po, ", q_off ", qo,
                ") points past a buffer (", ng, " gradient, ", np, " wire_p, ", nq, " wire_q floats)");
    in_g.emplace_back(off, off + n * m);
    in_p.emplace_back(po, po + n * rank);
    in_q.emplace_back(qo, qo + m * rank);
    const int64_t rb = (n + kPsgdRows - 1) / kPsgdRows;
    c.rowblocks += rb;
    c.colblocks += (m + kPsgdBpCols - 1) / kPsgdBpCols;
    c.tiles += rb * ((m + kPsgdCols - 1) / kPsgdCols);
  }
  for (int64_t s = 0; s < Rn; ++s) {
    const int64_t off = raw[3 * s], len = raw[3 * s + 1], wo = raw[3 * s + 2];
    TORCH_CHECK(off >= 0 && len >= 1 && wo >= 0 && (ng < 0 || len <= ng - off) && (np < 0 || len <= np - wo), op,
                ": raw row ", s, " (offset ", off, ", length ", len, ", wire_off ", wo, ") points past a buffer (",
                ng, " gradient, ", np, " wire_p floats)");
    in_g.emplace_back(off, off + len);
    in_p.emplace_back(wo, wo + len);
    c.rawchunks += (len + kPsgdRawChunk - 1) / kPsgdRawChunk;
  }
  const char* names[3] = {"the bucket", "wire_p", "the Q buffer"};
  std::vector<std::pair<int64_t, int64_t>>* spans[3] = {&in_g, &in_p, &in_q};
  for (int k = 0; k < 3; ++k) {
    std::sort(spans[k]->begin(), spans[k]->end());
    for (size_t i = 1; i < spans[k]->size(); ++i)
      TORCH_CHECK((*spans[k])[i].first >= (*spans[k])[i - 1].second, op, ": two table rows overlap in ", names[k]);
  }
  TORCH_CHECK(c.rowblocks + c.rawchunks < (1LL << 31) && c.colblocks < (1LL << 31) &&
              c.tiles + c.rawchunks < (1LL << 31), op, ": too many work items");
  return c;
}

// one function per operator (buffer sizes that must agree); -> (ng, np, nq) for psgd_tables
struct PsgdSizes { int64_t ng, np, nq; };
inline PsgdSizes psgd_project(T g, T e, T q, T wire_p, T low, T raw, int64_t rank) {
  psgd_args("psgd_project", {{"g", &g}, {"e", &e}, {"q", &q}, {"wire_p", &wire_p}}, low, &raw, rank);
  TORCH_CHECK(e.numel() == g.numel(), "psgd_project: e must have g's size");
  return {g.numel(), wire_p.numel(), q.numel()};
}
inline PsgdSizes psgd_orthonormalize(T wire_p, T low, int64_t rank) {
  psgd_args("psgd_orthonormalize", {{"wire_p", &wire_p}}, low, nullptr, rank);
  return {-1, wire_p.numel(), -1};
}
inline PsgdSizes psgd_backproject(T e, T wire_p, T q_loc, T wire_q, T low, int64_t rank) {
  psgd_args("psgd_backproject", {{"e", &e}, {"wire_p", &wire_p}, {"q_loc", &q_loc}, {"wire_q", &wire_q}}, low,
            nullptr, rank);
  TORCH_CHECK(wire_q.numel() == q_loc.numel(), "psgd_backproject: wire_q must have q_loc's size");
  return {e.numel(), wire_p.numel(), q_loc.numel()};
}
inline PsgdSizes psgd_residual(T e, T wire_p, T q_loc, T low, int64_t rank) {
  psgd_args("psgd_residual", {{"e", &e}, {"wire_p", &wire_p}, {"q_loc", &q_loc}}, low, nullptr, rank);
  return {e.numel(), wire_p.numel(), q_loc.numel()};
}
inline PsgdSizes psgd_decode(T g, T wire_p, T wire_q, T low, T raw, int64_t rank) {
  psgd_args("psgd_decode", {{"g", &g}, {"wire_p", &wire_p}, {"wire_q", &wire_q}}, low, &raw, rank);
  return {g.numel(), wire_p.numel(), wire_q.numel()};
}

}  // namespace checks
}  // namespace ddlpc
