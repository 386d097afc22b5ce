// The recipe of the label distance transform and the boundary erosion as host+device functions:
// the gfx950 kernel (boundary.hip) and its CPU twin (cpu_ref.cpp) call them, each function under
// its line of the recipe.  The independent statement of the contract is the torch brute force of
// tests/test_boundary.py, which both backends are compared against (integers: exact equality).
// Free of torch, and of HIP when compiled as plain C++.
//
//   A label image l[H][W], K classes (1..16), ignore_index.
//   * valid(p)   iff 0 <= l(p) < K and l(p) != ignore_index            -> label_class (else -1)
//   * d2(p)      = min |p - q|^2 over the valid q of the same image with l(q) != l(p), Euclidean,
//                  in integer squared pixels, truncated at R = 16: without such a q inside
//                  |p - q|^2 <= 256, d2(p) = 257 ("far").  An invalid p has d2 = 0.  Nothing lies
//                  outside the image (no mirroring, no wrap), images of a batch never meet.
//   * erode(r)   a valid p with d2(p) <= r^2 becomes `fill`, everything else is copied; r = 0 is
//                  the identity (d2 >= 1 for every valid pixel), r = 3 the ISPRS disc.
//
// Both backends work on 32 x 32 output tiles inside a 64 x 64 stage (the tile and a 16-pixel halo
// on each side), one bit per pixel: a staged row is one 64-bit word per class,
//   ne[row][k] = bit c set iff staged pixel (row, c) is valid and its class is not k,
// built from the row's validity word and the four bit planes of its labels (other_mask).  The
// output pixel at stage position (row, b), b in 16..47, of class L then needs, for each dy in
// -16..16, only the set bit of ne[row + dy][L] nearest to b (nearest_dx): 33 steps of shifts, a
// count-trailing-zeros, a count-leading-zeros and a multiply-add, no inner x loop (pixel_dist2).
#pragma once

#include <stdint.h>

#include "hd.h"

namespace ddlpc {

constexpr int kLabelR = 16;                       // truncation radius
constexpr int kLabelFar = kLabelR * kLabelR + 1;  // d2 of a pixel with no other class within R
constexpr int kLabelTile = 32;                    // output tile side
constexpr int kLabelStage = kLabelTile + 2 * kLabelR;   // 64: one word per staged row and class
constexpr int kLabelMaxK = 16;

// the class code of a label: 0..K-1 for a valid pixel, -1 otherwise
DDLPC_HDI int label_class(long long l, int K, int ignore_index) {
  return (l >= 0 && l < K && l != ignore_index) ? (int)l : -1;
}

// ne[row][k] from the row's words: valid = its valid pixels, plane[j] = the pixels whose class
// code has bit j set (any value at invalid pixels)
DDLPC_HDI uint64_t other_mask(uint64_t valid, const uint64_t* plane, int k) {
  uint64_t eq = valid;
#pragma unroll
  for (int j = 0; j < 4; ++j) eq &= ((k >> j) & 1) ? plane[j] : ~plane[j];
  return valid & ~eq;
}

// |x - b| of the set bit x of `word` nearest to bit b (16 <= b <= 47), 17 if none within 16:
// to the right bits b..b+16 (count-trailing-zeros over a guard bit at 17), to the left bits
// b-16..b, bit i at distance 16 - i (count-leading-zeros; shifted up by one over a guard bit 0)
DDLPC_HDI int nearest_dx(uint64_t word, int b) {
  const uint32_t right = ((uint32_t)(word >> b) & 0x1ffffu) | 0x20000u;
  const uint32_t left = (((uint32_t)(word >> (b - kLabelR)) & 0x1ffffu) << 1) | 1u;
  const int dr = __builtin_ctz(right), dl = __builtin_clz(left) - 14;
  return dr < dl ? dr : dl;
}

// min over |dy| <= reach of nearest_dx^2 + dy^2, clipped: above 256 -> 257.  ne: the stage's
// words [kLabelStage][kLabelMaxK]; (row, b) the pixel's stage position, both in 16..47; L its
// class.  reach = 16 is d2; a smaller reach r is exact wherever d2 <= r^2 (a q at |p - q| <= r
// has |dy| <= r) and gives a value > r^2 elsewhere: all the erosion asks
DDLPC_HDI int pixel_dist2(const uint64_t* ne, int row, int b, int L, int reach) {
  int best = kLabelFar;
  for (int dy = -reach; dy <= reach; ++dy) {
    const int dx = nearest_dx(ne[(row + dy) * kLabelMaxK + L], b);
    const int c = dx * dx + dy * dy;
    best = c < best ? c : best;
  }
  return best;
}

// the transform's value at a pixel of class code `cls`: 0 for an invalid pixel
DDLPC_HDI int label_dist2_at(const uint64_t* ne, int row, int b, int cls, int reach) {
  return cls < 0 ? 0 : pixel_dist2(ne, row, b, cls, reach);
}

// erosion: a valid pixel within radius r of another class is rewritten
DDLPC_HDI bool label_eroded(int cls, int d2, int r) { return cls >= 0 && d2 <= r * r; }

}  // namespace ddlpc
