// Argument checks of the BatchNorm / gradient-tail operators, one function per operator, called by
// both registrations (bindings.cpp, cpu_ref.cpp): dtype, rank, element counts against C and
// `groups`, same-device, ranges.  A wrong size would reach a kernel as an out-of-bounds pointer,
// so every call is refused here before any launch.  What depends on the backend stays with it:
// is_cuda, contiguity where the CPU twin calls .contiguous(), grid limits (C % 8, the group
// kernels' channel counts).
#pragma once

#include "data_checks.h"      // T, OptT, has

namespace ddlpc {
namespace checks {

// n fp32 elements on `like`'s device
inline void f32_n(const char* op, const char* name, T t, int64_t n, T like) {
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.numel() == n, op, ": ", name, " must hold ", n, " fp32 elements");
  TORCH_CHECK(t.device() == like.device(), op, ": ", name, " on another device");
}

// ... that a kernel also writes through its raw pointer
inline void f32_buf(const char* op, const char* name, T t, int64_t n, T like) {
  f32_n(op, name, t, n, like);
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

inline void nbt_arg(const char* op, OptT nbt, T like) {
  if (has(nbt))
    TORCH_CHECK(nbt->scalar_type() == at::kLong && nbt->numel() >= 1 && nbt->device() == like.device(), op,
                ": num_batches_tracked must be int64 on the device of the other tensors");
}

// a channel-last activation [N, (D,) H, W, C] -> C
inline int64_t act_channels(const char* op, T y) {
  TORCH_CHECK(y.dim() == 4 || y.dim() == 5, op, ": expected [N,(D,)H,W,C] channel-last tensor");
  TORCH_CHECK(y.scalar_type() == at::kBFloat16 && y.size(-1) >= 1, op, ": y must be bf16 with C >= 1");
  return y.size(-1);
}

inline void groups_of(const char* op, T y, int64_t groups) {
  TORCH_CHECK(groups >= 1 && groups <= 1024 && y.size(0) % groups == 0, op,
              ": 1 <= groups <= 1024 dividing the batch");
}

// partial rows [R][2][C] (per group: [groups * R][2][C]) -> R
inline int64_t stat_rows(const char* op, T partial, int64_t C, int64_t groups, T like) {
  TORCH_CHECK(partial.scalar_type() == at::kFloat && C >= 1 && partial.numel() % (groups * 2 * C) == 0, op,
              ": partial must be fp32 rows [R][2][C]");
  TORCH_CHECK(partial.device() == like.device(), op, ": partial on another device");
  return partial.numel() / (groups * 2 * C);
}

// the caller's gradient accumulators: both or neither, C fp32 elements each
inline void grad_outs(const char* op, OptT dgamma_out, OptT dbeta_out, int64_t C, T like) {
  TORCH_CHECK(has(dgamma_out) == has(dbeta_out), op, ": dgamma_out and dbeta_out go together");
  if (!has(dgamma_out)) return;
  f32_buf(op, "dgamma_out", *dgamma_out, C, like);
  f32_buf(op, "dbeta_out", *dbeta_out, C, like);
}

// `groups` arena rows of (mean | unbiased var) = 2C floats at column aoff
inline void arena_arg(const char* op, OptT arena, int64_t groups, int64_t aoff, int64_t C, T like) {
  if (!has(arena)) return;
  TORCH_CHECK(arena->scalar_type() == at::kFloat && arena->dim() == 2 && arena->size(0) >= groups &&
              arena->stride(1) == 1 && aoff >= 0 && aoff + 2 * C <= arena->size(1), op,
              ": arena fp32 [rows >= groups][>= aoff + 2C]");
  TORCH_CHECK(arena->device() == like.device(), op, ": arena on another device");
}

inline void bn_finalize(T partial, T gamma, T beta, T running_mean, T running_var, OptT nbt) {
  const int64_t C = gamma.numel();
  stat_rows("bn_finalize", partial, C, 1, partial);
  f32_n("bn_finalize", "gamma", gamma, C, partial);
  f32_n("bn_finalize", "beta", beta, C, partial);
  f32_buf("bn_finalize", "running_mean", running_mean, C, partial);
  f32_buf("bn_finalize", "running_var", running_var, C, partial);
  nbt_arg("bn_finalize", nbt, partial);
}

// slots: [K][2C] rows of (mean | unbiased var), any row stride (a column slice of a
// per-micro-batch arena), rows contiguous
inline void bn_running_apply(T running_mean, T running_var, T slots, OptT nbt) {
  const int64_t C = running_mean.numel();
  f32_buf("bn_running_apply", "running_mean", running_mean, C, slots);
  f32_buf("bn_running_apply", "running_var", running_var, C, slots);
  TORCH_CHECK(slots.scalar_type() == at::kFloat && slots.dim() == 2 && slots.size(1) == 2 * C &&
              slots.stride(1) == 1 && slots.size(0) < (1LL << 31),
              "bn_running_apply: slots fp32 [K][2C] with contiguous rows");
  nbt_arg("bn_running_apply", nbt, slots);
}

// entries [L][4] int64 (running_mean*, running_var*, nbt* | 0, C | arena column << 32): the
// pointers and columns are the caller's (device data on the GPU)
inline void bn_running_apply_all(T entries, T arena, int64_t K, int64_t maxC) {
  TORCH_CHECK(entries.scalar_type() == at::kLong && entries.dim() == 2 && entries.size(1) == 4,
              "bn_running_apply_all: entries [L][4] int64");
  TORCH_CHECK(arena.scalar_type() == at::kFloat && arena.dim() == 2 && arena.stride(1) == 1 && K >= 0 &&
              K < (1LL << 31) && arena.size(0) >= K, "bn_running_apply_all: arena fp32 [rows >= K][cols]");
  TORCH_CHECK(maxC >= 1 && 2 * maxC <= arena.size(1), "bn_running_apply_all: 1 <= maxC, 2 maxC <= the arena's columns");
  TORCH_CHECK(entries.device() == arena.device(), "bn_running_apply_all: tensors on different devices");
}

inline void bn_group_apply(T y, T stats4, int64_t groups, bool pool) {
  (void)pool;
  const int64_t C = act_channels("bn_group_apply", y);
  groups_of("bn_group_apply", y, groups);
  f32_n("bn_group_apply", "stats4 [groups][4][C]", stats4, groups * 4 * C, y);
}

inline void bn_relu_apply(T y, T stats4, bool pool, bool full) {
  TORCH_CHECK(full || pool, "bn_relu_apply: full=False only with pool (deferred skip)");
  bn_group_apply(y, stats4, 1, pool);
}

// dA (same elements as y) and / or the pooled dP (a 2^dims-th of them); partial: precomputed rows
inline void bn_group_backward(OptT dA, OptT dP, T y, T stats4, T gamma, int64_t groups, OptT dgamma_out,
                              OptT dbeta_out, OptT partial, const char* op = "bn_group_backward") {
  const int64_t C = act_channels(op, y);
  groups_of(op, y, groups);
  TORCH_CHECK(has(dA) || has(dP), op, " needs dA or dP");
  if (has(dA))
    TORCH_CHECK(dA->scalar_type() == at::kBFloat16 && dA->numel() == y.numel() && dA->device() == y.device(),
                op, ": dA must be bf16 of y's shape");
  if (has(dP))
    TORCH_CHECK(dP->scalar_type() == at::kBFloat16 && dP->numel() * (y.dim() == 5 ? 8 : 4) == y.numel() &&
                dP->device() == y.device(), op, ": dP must be bf16 of y's pooled shape");
  f32_n(op, "stats4 [groups][4][C]", stats4, groups * 4 * C, y);
  f32_n(op, "gamma", gamma, C, y);
  grad_outs(op, dgamma_out, dbeta_out, C, y);
  if (has(partial) && partial->numel() > 0) {
    TORCH_CHECK(!has(dP), op, ": precomputed partial rows, no pooled gradient");
    stat_rows(op, *partial, C, groups, y);
  }
}

inline void bn_backward(OptT dA, OptT dP, T y, T stats4, T gamma, OptT gscale, OptT dgamma_out, OptT dbeta_out,
                        OptT partial_in) {
  bn_group_backward(dA, dP, y, stats4, gamma, 1, dgamma_out, dbeta_out, partial_in, "bn_backward");
  if (has(gscale))
    TORCH_CHECK(gscale->scalar_type() == at::kFloat && gscale->numel() >= 1 && gscale->device() == y.device(),
                "bn_backward: gscale must be fp32 on y's device");
  if (has(partial_in) && partial_in->numel() > 0)
    TORCH_CHECK(!has(gscale), "bn_backward: precomputed partial rows, no grad scale");
}

inline void bn_grad_coefs(T partial, T y, T stats4, T gamma, OptT dgamma_out, OptT dbeta_out) {
  const int64_t C = act_channels("bn_grad_coefs", y);
  TORCH_CHECK(stat_rows("bn_grad_coefs", partial, C, 1, y) >= 1, "bn_grad_coefs: no partial rows");
  f32_n("bn_grad_coefs", "stats4 [4][C]", stats4, 4 * C, y);
  f32_n("bn_grad_coefs", "gamma", gamma, C, y);
  grad_outs("bn_grad_coefs", dgamma_out, dbeta_out, C, y);
}

inline void bn_group_finalize(T y, int64_t groups, T gamma, T beta, OptT arena, int64_t aoff) {
  const int64_t C = act_channels("bn_group_finalize", y);
  groups_of("bn_group_finalize", y, groups);
  f32_n("bn_group_finalize", "gamma", gamma, C, y);
  f32_n("bn_group_finalize", "beta", beta, C, y);
  arena_arg("bn_group_finalize", arena, groups, aoff, C, y);
}

inline void bn_group_finalize_rows(T partial, int64_t groups, T gamma, T beta, OptT arena, int64_t aoff) {
  const int64_t C = gamma.numel();
  TORCH_CHECK(groups >= 1 && groups <= 1024, "bn_group_finalize_rows: 1 <= groups <= 1024");
  stat_rows("bn_group_finalize_rows", partial, C, groups, partial);
  f32_n("bn_group_finalize_rows", "gamma", gamma, C, partial);
  f32_n("bn_group_finalize_rows", "beta", beta, C, partial);
  arena_arg("bn_group_finalize_rows", arena, groups, aoff, C, partial);
}

// reduce_rows_launch's multi-level loop has one scratch region for its intermediate passes:
// above 64^3 rows a second intermediate pass would read and write it at once
inline void reduce_rows(T partial, int64_t R, int64_t N) {
  TORCH_CHECK(R >= 0 && R <= 262144, "reduce_rows: at most 262144 rows");
  TORCH_CHECK(partial.scalar_type() == at::kFloat && N >= 0 && N < (1LL << 40) && partial.numel() >= R * N,
              "reduce_rows: partial must hold R * N fp32 elements");
}

// rows of N columns at a row stride of ld floats (-1: N); mode 0 / 1: N = A * T * B -> A
inline int64_t reduce_rows_scatter(T slab, int64_t R, int64_t N, T dst, int64_t mode, int64_t Tt, int64_t B,
                                   int64_t ld) {
  TORCH_CHECK(slab.scalar_type() == at::kFloat && slab.is_contiguous(), "slab must be contiguous fp32");
  TORCH_CHECK(dst.scalar_type() == at::kFloat && dst.is_contiguous(), "dst must be contiguous fp32");
  TORCH_CHECK(slab.device() == dst.device(), "reduce_rows_scatter: slab and dst on different devices");
  TORCH_CHECK(mode >= 0 && mode <= 2, "reduce_rows_scatter: mode must be 0, 1 or 2");
  TORCH_CHECK(R >= 0 && R <= INT32_MAX && N >= 0, "reduce_rows_scatter: bad R / N");
  TORCH_CHECK(ld == -1 || ld >= N, "reduce_rows_scatter: ld must be -1 or at least N");
  TORCH_CHECK(dst.numel() == N, "reduce_rows_scatter: dst must hold exactly N elements");
  int64_t A = 0;
  if (mode != 2) {
    TORCH_CHECK(Tt > 0 && B > 0 && Tt <= INT32_MAX && B <= INT32_MAX && N % (Tt * B) == 0,
                "reduce_rows_scatter: N must be A * T * B");
    A = N / (Tt * B);
  }
  if (R > 0 && N > 0)
    TORCH_CHECK(slab.numel() >= (R - 1) * (ld < 0 ? N : ld) + N,
                "reduce_rows_scatter: slab shorter than (R - 1) * ld + N");
  return A;
}

}  // namespace checks
}  // namespace ddlpc
