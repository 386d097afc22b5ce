// The arithmetic of the soft-Dice term of the head's loss as host+device functions: the gfx950
// kernels (head_ce.hip) and their CPU twins (cpu_ref.cpp) call them.  Free of torch, and of HIP
// when compiled as plain C++.
//
//   per-class sums over the valid pixels (label != ignore_index) of one call, p = softmax:
//       I_c = sum p_c [y = c]     S_c = sum p_c     Y_c = sum [y = c]     D_c = S_c + Y_c + eps
//       dice = 1 - (1 / K) sum_{c < K} (2 I_c + eps) / D_c          L = L_CE + lambda dice
//   its gradient on a valid pixel, with g_c = B_c + A_c [y = c]:
//       A_c = -2 lambda / (K D_c)      B_c = lambda (2 I_c + eps) / (K D_c^2)
//       d(lambda dice) / dz_j = p_j (g_j - sum_c p_c g_c)
//   the device table (kDiceTable floats): A[16] | B[16] | dice | L_CE | 0 ...  — padded classes
//   (c >= K) carry A = B = 0; a call without a valid pixel has dice = 0 and a table of zeros.
#pragma once

#include <cmath>

#include "hd.h"

namespace ddlpc {

constexpr int kDiceK = 16;                 // class slots of a partial row and of the table
constexpr int kDiceRow = 3 * kDiceK;       // one partial row: I[16] | S[16] | Y[16]
constexpr int kDiceTable = 40;

// ce3 = fp64 sums (loss terms, hits, count or weight sum), isy = fp64 sums I | S | Y
// -> out3 = [L, hits, count] and the table
DDLPC_HDI void dice_finalize(const double* ce3, const double* isy, int K, float lambda, float eps,
                             float* out3, float* tab) {
  const double cnt = ce3[2];
  const double ce = ce3[0] / (cnt > 0 ? cnt : 1.0);
  double pixels = 0;                       // sum_c S_c: the valid pixels (each softmax sums to 1)
  for (int c = 0; c < kDiceK; ++c) pixels += isy[kDiceK + c];
  double sum = 0;
  for (int c = 0; c < kDiceK; ++c) {
    float A = 0.f, B = 0.f;
    if (c < K && pixels > 0) {
      const double D = isy[kDiceK + c] + isy[2 * kDiceK + c] + (double)eps;
      const double num = 2.0 * isy[c] + (double)eps;
      sum += num / D;
      A = (float)(-2.0 * (double)lambda / (K * D));
      B = (float)((double)lambda * num / (K * D * D));
    }
    tab[c] = A;
    tab[kDiceK + c] = B;
  }
  const double dice = pixels > 0 ? 1.0 - sum / K : 0.0;
  tab[2 * kDiceK] = (float)dice;
  tab[2 * kDiceK + 1] = (float)ce;
  for (int i = 2 * kDiceK + 2; i < kDiceTable; ++i) tab[i] = 0.f;
  out3[0] = (float)(ce + (double)lambda * dice);
  out3[1] = (float)ce3[1];
  out3[2] = (float)cnt;
}

// g_c of a pixel, and the pixel's Dice dlogit from p_j, g_j and dot = sum_c p_c g_c
DDLPC_HDI float dice_g(float A, float B, bool is_label) { return is_label ? B + A : B; }
DDLPC_HDI float dice_dz(float p, float g, float dot) { return fmaf(-p, dot, p * g); }

}  // namespace ddlpc
