// Arithmetic and geometry of the low-rank gradient codec (PowerSGD, Vogels et al. 2019), shared by
// the gfx950 kernels (powersgd.hip) and their CPU twins (cpu_ref.cpp): one text.  parallel/codec.py
// holds the contract of the five steps (project, orthonormalise, back-project, residual, decode).
//
// Tables (int32, built once per bucket by powersgd_plan; codec_checks.h refuses a row that leaves a
// buffer or overlaps another):
//     low [T][5] = (offset in the bucket, n, m, p_off, q_off): an n x m row-major matrix of the
//                  gradient, its P block (n x r, row-major) at wire_p + p_off, its Q block (m x r)
//                  at q_off of wire_q / q_prev / q_loc
//     raw [R][3] = (offset in the bucket, length, wire_off): a span sent as it is, at wire_p + wire_off
// The alignment gaps of the flat layout belong to no row and are never touched.
//
// Work items (a launch's grid is the sum of its items over the table: a function of the table alone):
//     project               ceil(n / kPsgdRows) row blocks per tensor, then the raw chunks
//     back-project          ceil(m / kPsgdBpCols) column blocks per tensor
//     residual / decode     ceil(n / kPsgdRows) x ceil(m / kPsgdCols) tiles per tensor (decode: then
//                           the raw chunks)
//     raw spans             ceil(length / kPsgdRawChunk) chunks per span
#pragma once

#include <cmath>

#include "hd.h"

namespace ddlpc {

constexpr int kPsgdMaxRank = 16;       // r is padded to the MFMA's 16-wide N tile
constexpr int kPsgdRows = 16;          // rows of a project item and of a residual / decode tile
constexpr int kPsgdCols = 256;         // columns of a residual / decode tile; K-chunk of the project
constexpr int kPsgdBpCols = 64;        // columns of a back-project item (one per lane, 4 waves split the rows)
constexpr int kPsgdRawChunk = 1024;    // floats of a raw-span item

struct PsgdCounts { long long rowblocks = 0, colblocks = 0, tiles = 0, rawchunks = 0; };

// element (row, col) of P Q^T: an fma chain over j = 0 .. r - 1 from +0.f; ps / qs: the strides of
// the two rows (1 in global memory; the kernels keep Q transposed in LDS).  Residual and decode of
// both kernel sets call this, so they agree bit for bit on the same P, Q.
DDLPC_HDI float psgd_dot(const float* p, int ps, const float* q, int qs, int r) {
  float acc = 0.f;
  for (int j = 0; j < r; ++j) acc = __builtin_fmaf(p[j * ps], q[j * qs], acc);
  return acc;
}

// the scale of a column from its squared norm (summed in double): fp32(1 / sqrt(s2)); a squared
// norm of 0 marks a zero column (-> +0.f, the caller writes zeros); NaN stays NaN, +Inf gives 0
DDLPC_HDI float psgd_inv_norm(double s2) { return s2 == 0.0 ? 0.f : (float)(1.0 / sqrt(s2)); }

}  // namespace ddlpc
