// The arithmetic of the BatchNorm statistics / gradient tail as host+device functions: the
// gfx950 kernels (reduce.hip, bn.hip) and their CPU twins (cpu_ref.cpp) call them, so the two
// backends round alike.  The kernels are the specification: where the device compiler fuses a
// multiply into an add the fused operation is written out (fma / fmaf), everything else rounds
// on its own (contraction off).  Free of torch, and of HIP when compiled as plain C++.
//
//   * stats4 from the fp64 sums s1 = sum y, s2 = sum y^2 over `count` pixels:
//       mean = s1 / count,  var = max(fma(-mean, mean, s2 / count), 0),
//       invstd = float(1 / sqrt(var + eps)),  scale = gamma invstd,
//       shift = fmaf(-float(mean), scale, beta);  the running variance takes the unbiased one
//   * running <- fmaf(m, x, (1 - m) running), slot after slot in micro-batch order
//   * gradient finalize from t1 = sum dyh, t2 = sum dyh xhat (after the optional dscale):
//       dbeta = float(t1), dgamma = float(t2), k = gamma invstd, m1 = float(t1 / count),
//       m2 = float(t2 / count)
//   * slab_perm: where column j of a weight-gradient slab goes in the parameter's layout
//   * the row-count regimes of the slab sums and their summation orders (slab_column_sum)
#pragma once

#include <cmath>

#include "hd.h"

namespace ddlpc {

struct BnStats4 {
  float mean, invstd, scale, shift;
  double var;                      // clamped, biased
};

DDLPC_HDI BnStats4 bn_stats4(double s1, double s2, double count, float gamma, float beta, float eps) {
#pragma clang fp contract(off)
  const double mean = s1 / count;
  double var = fma(-mean, mean, s2 / count);
  if (var < 0) var = 0;
  const float inv = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gamma * inv;
  return {(float)mean, inv, sc, fmaf(-(float)mean, sc, beta), var};
}

// the unbiased variance the running statistics take (a single pixel keeps the biased one)
DDLPC_HDI float bn_unbiased_var(double var, double count) {
#pragma clang fp contract(off)
  return (float)(count > 1 ? var * count / (count - 1) : var);
}

// running <- (1 - m) running + m x, in one fixed fp32 form: the deferred (per-micro-batch
// slot) updates reproduce the in-kernel ones bit for bit; with m = 1 a slot receives x exactly
DDLPC_HDI float bn_momentum_update(float running, float x, float m) {
#pragma clang fp contract(off)
  return fmaf(m, x, (1.f - m) * running);
}

// channel c's K deferred updates, in slot order; slot k: [mean (C) | var (C)] at k * stride
DDLPC_HDI void bn_running_apply_channel(float* running_mean, float* running_var, const float* slots, int K,
                                        int C, long long stride, int c, float m) {
  float rm = running_mean[c], rv = running_var[c];
  for (int k = 0; k < K; ++k) {
    rm = bn_momentum_update(rm, slots[k * stride + c], m);
    rv = bn_momentum_update(rv, slots[k * stride + C + c], m);
  }
  running_mean[c] = rm;
  running_var[c] = rv;
}

struct BnGradTerms {
  float dbeta, dgamma, k, m1, m2;
};

DDLPC_HDI BnGradTerms bn_grad_terms(double t1, double t2, double count, float gamma, float invstd) {
#pragma clang fp contract(off)
  return {(float)t1, (float)t2, gamma * invstd, (float)(t1 / count), (float)(t2 / count)};
}

// mode 0: conv slab [co][tap][ci] -> OIHW [co][ci][tap]  (T = taps, B = Cin;  j = (co*T + tap)*B + ci)
// mode 1: convT slab [ci][(sub, co)] -> IOHW [ci][co][sub] (T = subs, B = Cout; j = (ci*T + sub)*B + co)
// — one map [a][t][b] -> [a][b][t], written in mode 0's names; any other mode: identity
DDLPC_HDI long long slab_perm(int mode, long long j, int T, int B) {
  if (mode != 0 && mode != 1) return j;
  const int ci = (int)(j % B);
  const int tap = (int)((j / B) % T);
  const long long co = j / ((long long)B * T);
  return (co * B + ci) * T + tap;
}

// The slab sums' row-count regimes (reduce_rows_scatter_launch): up to kSlabChunkRows rows one
// serial pass; up to kWideMaxRows the one-launch form, kWideWaves interleaved row sets added in
// order; above, chunks of kSlabChunkRows rows, then the chunk sums.
constexpr int kSlabChunkRows = 64;
constexpr int kWideWaves = 4;
constexpr int kWideMaxRows = 1024;   // (why 1024: at rows_sum_wide_kernel, reduce.hip)

// column j of in[R][ld] summed in fp64 in the order the launcher's regime for R sums it
inline double slab_column_sum(const float* in, long long R, long long ld, long long j) {
  double s = 0.0;
  if (R <= kSlabChunkRows) {
    for (long long r = 0; r < R; ++r) s += (double)in[r * ld + j];
  } else if (R <= kWideMaxRows) {
    double w[kWideWaves] = {};
    for (int k = 0; k < kWideWaves; ++k)
      for (long long r = k; r < R; r += kWideWaves) w[k] += (double)in[r * ld + j];
    for (int k = 0; k < kWideWaves; ++k) s += w[k];
  } else {
    for (long long r0 = 0; r0 < R; r0 += kSlabChunkRows) {
      double c = 0.0;
      for (long long r = r0; r < R && r < r0 + kSlabChunkRows; ++r) c += (double)in[r * ld + j];
      s += c;
    }
  }
  return s;
}

}  // namespace ddlpc
