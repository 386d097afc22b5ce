// The recipe of the input and prediction pipeline as host+device functions: the gfx950 kernels
// (data.hip, scene.hip, the index map of head_ce.hip) and their CPU twins (cpu_ref.cpp) call
// them, each function under its line of the recipe.  The independent statement of the contract
// is the numpy twin (data/scenes.py *_reference, data/datasets.py), which the tests compare both
// backends against.  Free of torch, and of HIP when compiled as plain C++.  Where calling a
// function changed a kernel's instructions and cost time (docs/PERF.md) the kernel spells that
// part itself: synth_tiles_kernel its whole recipe (as its CPU twin), the three gather kernels
// the D4 map, crop_gather_kernel and warp_gather_kernel the validity predicates.
//
//   * synth_tiles: the synthetic Vaihingen-shape generator.  Sample i depends only on (seed, i):
//     a counter-based hash (no RNG state), so a batch is the same whichever rank, batch position
//     or resume point renders it.
//       key     = mix(mix(seed ^ 0x9E3779B9) ^ i)
//       coarse  = mix(key ^ mix(cell + 0x632BE5AB)) % classes   on a grid^dims lattice
//       label   = coarse[(h*grid)/tile][(w*grid)/tile]           (nearest up-sampling)
//       u_j     = (mix(key ^ mix(p*8 + ch + 0x1B873593) + j*0x9E3779B9) >> 8) * 2^-24
//       x       = clamp(palette[label][ch] + (((u0+u1)+u2)+u3 - 2) * k, 0, 1)   -> bf16
//     (Irwin-Hall noise: k = noise*sqrt(3) gives std `noise`; every float op rounds on its own.)
//   * tile_gather: a uint8 NHWC dataset (+ uint8 label maps) resident in HBM: gather the batch's
//     sample indices, /255 (IEEE division), pad, bf16; labels widen to int64.
//   * crop_params + crop_gather: the scenes are uploaded once, packed: uint8 pixels [total, in_ch],
//     uint8 labels [total] and an int64 table [n, 3] of (pixel offset, H, W) rows.  A batch is
//     tile x tile random crops under one of the 8 symmetries of the square and a per-sample gain /
//     bias.  Virtual sample s depends only on (seed, s): key and draws r_0..r_5 below; scene =
//     pick_scene(r0) over cum, the prefix sum of the scenes' valid-origin counts ny * nx (crops
//     are uniform over all valid crops; cum[n] < 2^32); y0, x0 = the origin draws of r1, r2; code,
//     gain, bias from r3, r4, r5.  Output pixel (oy, ox) reads source pixel (y0 + a, x0 + b),
//     (a, b) = d4_forward, mirrored into the scene; v = u8 / 255, with colour the clamp, then bf16.
//     window_gather reads through the same map, head_predict_accum through its inverse.
//   * warp_params + warp_gather: the same crops under a random zoom and a rotation by an arbitrary
//     angle.  Coordinates are 16.16 fixed point in int64 (ONE = 65536; >> is arithmetic = floor).
//     Zoom and angle reach the kernels as two int32 tables the host builds in float64
//     (data/scenes.py): steps[S] = rint(ONE / z_k), z_k = zoom_min (zoom_max / zoom_min)^((k + .5)
//     / S) and rot[T] = (rint(cos t_k ONE), rint(sin t_k ONE)), t_k = -rotate_deg + (k + .5) 2
//     rotate_deg / T: integers only on the device.  warp_params: crop_params's key, scene, code
//     and colour (the scene choice keeps the unit-scale cum table), step = steps[(r6 * S) >> 32],
//     (c, sn) = rot[(r7 * T) >> 32], A, Bm = matrix_entry, F = footprint, cy, cx =
//     footprint_centre of r1, r2 -> wparams int64 [B, 6] = (scene, cy, cx, code, A, Bm).
//     warp_gather: warp_coord of (a, b); taps p00, p01, p10, p11 at rows reflect(iy), reflect(iy +
//     1), columns reflect(ix), reflect(ix + 1), blended per channel (bilinear), / 255, the colour
//     clamp, bf16; label: nearest.  A row that fails scene_row_valid or warp_row_valid reads
//     nothing (zero image, labels -100).  (A, Bm) = (ONE, 0), cy = (2 y0 + tile - 1) * 32768 is
//     crop_gather's (y0, x0) crop, bit for bit.
#pragma once

#include <stdint.h>

#include <cmath>
#include <type_traits>

#include "hd.h"

namespace ddlpc {

// mix: the 32-bit finalizer every key and draw goes through
DDLPC_HDI uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// u24(h) = (h >> 8) * 2^-24: a uniform in [0, 1), exact in fp32
DDLPC_HDI float u24(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

// key = mix(mix(mix(seed ^ 0xC2B2AE35) ^ lo32(s)) ^ mix(hi32(s) + 0x85EBCA6B))
DDLPC_HDI uint32_t sample_key(uint32_t seed, uint64_t s) {
  const uint32_t skey = mix32(seed ^ 0xC2B2AE35u);
  return mix32(mix32(skey ^ (uint32_t)s) ^ mix32((uint32_t)(s >> 32) + 0x85EBCA6Bu));
}

// r_j = mix(key + (j + 1) * 0x9E3779B9)
DDLPC_HDI uint32_t draw(uint32_t key, int j) { return mix32(key + (uint32_t)(j + 1) * 0x9E3779B9u); }

// the scene k with cum[k] <= (r0 * cum[n]) >> 32 < cum[k + 1]
DDLPC_HDI int pick_scene(const int64_t* __restrict__ cum, int n, uint32_t r0) {
  const uint64_t t = ((uint64_t)r0 * (uint64_t)cum[n]) >> 32;
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((uint64_t)cum[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// (r * n) >> 32: a draw scaled to [0, n)
DDLPC_HDI uint64_t scale_draw(uint32_t r, uint64_t n) { return ((uint64_t)r * n) >> 32; }

// ny = max(size - span, 0) + 1 (unsigned: a wild table entry wraps, the gather rejects its row)
DDLPC_HDI uint64_t origin_count(long long size, long long span) {
  return (size > span ? (uint64_t)size - (uint64_t)span : 0u) + 1u;
}

// code = 0 | r3 & 3 | r3 & 7                                   (mode: none | flip | d4)
DDLPC_HDI int symmetry_code(uint32_t r3, int mode) {
  return mode == 0 ? 0 : (int)(r3 & (mode == 1 ? 3u : 7u));
}

// gain = 1 + gain_jitter * (2 u24(r4) - 1),  bias = bias_jitter * (2 u24(r5) - 1) -> color[0..1]
DDLPC_HDI void color_jitter(uint32_t r4, uint32_t r5, float gj, float bj, float* __restrict__ color) {
  color[0] = add_rn(1.0f, mul_rn(gj, add_rn(mul_rn(2.0f, u24(r4)), -1.0f)));
  color[1] = mul_rn(bj, add_rn(mul_rn(2.0f, u24(r5)), -1.0f));
}

// F = (tile * step + 65535) >> 16: the un-rotated source footprint of a tile at a zoom step
DDLPC_HDI long long footprint(int tile, long long step) { return ((long long)tile * step + 65535) >> 16; }

// cy = (2 y0 + F - 1) * 32768, y0 = (r * ny) >> 32: the 16.16 centre of an F-pixel footprint
DDLPC_HDI long long footprint_centre(uint32_t r, long long size, long long F) {
  const uint64_t o = scale_draw(r, origin_count(size, F));
  return (long long)((2u * o + (uint64_t)F - 1u) * 32768u);
}

// A = (step * c + 32768) >> 16 (and Bm from sn): a 16.16 product rounded to nearest
DDLPC_HDI long long matrix_entry(long long step, long long c) { return (step * c + 32768) >> 16; }

// mirror index i into [0, n): period 2 (n - 1), edge pixel not repeated; a window may wrap
// several times over a scene smaller than itself
template <typename I>
DDLPC_HDI I reflect_index(I i, I n) {
  if (n == 1) return 0;
  const I p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i >= n ? p - i : i;
}

// reflect_index without the division for a coordinate already inside the scene
template <typename I>
DDLPC_HDI I reflect_fast(I i, I n) {
  typedef typename std::make_unsigned<I>::type U;
  return (U)i < (U)n ? i : reflect_index(i, n);
}

template <typename I>
struct Index2 {
  I a, b;       // (row, column)
};

// D4 forward map, output pixel (oy, ox) -> source-frame pixel (a, b):
// (a, b) = (oy, ox); code & 4: swap a, b; code & 2: a = tile - 1 - a; code & 1: b = tile - 1 - b
template <typename I>
DDLPC_HDI Index2<I> d4_forward(int code, I tile, I oy, I ox) {
  I a = (code & 4) ? ox : oy, b = (code & 4) ? oy : ox;
  if (code & 2) a = tile - 1 - a;
  if (code & 1) b = tile - 1 - b;
  return {a, b};
}

// D4 inverse map, source-frame pixel (a, b) -> the output pixel (oy, ox) that reads it
template <typename I>
DDLPC_HDI Index2<I> d4_inverse(int code, I tile, I a, I b) {
  const I ia = (code & 2) ? tile - 1 - a : a;
  const I ib = (code & 1) ? tile - 1 - b : b;
  return {(code & 4) ? ib : ia, (code & 4) ? ia : ib};
}

// a scene outside [0, n) reads nothing, nor does a table row (off, H, W) outside the pixel
// buffer (the table is device data: the host cannot check it without a read-back)
DDLPC_HDI bool scene_row_valid(bool listed, long long off, long long H, long long W, long long total_px) {
  return listed && H >= 1 && W >= 1 && H < (1 << 30) && W < (1 << 30) && off >= 0 && off <= total_px &&
         H * W <= total_px - off;
}

// a matrix / centre small enough that every warp coordinate stays far inside int64 and its
// integer part inside int: |A|, |Bm| <= 2^20, |cy|, |cx| < 2^46
constexpr long long kCoef = 1LL << 20, kCentre = 1LL << 46;
DDLPC_HDI bool warp_row_valid(long long A, long long Bm, long long cy, long long cx) {
  return A >= -kCoef && A <= kCoef && Bm >= -kCoef && Bm <= kCoef && cy > -kCentre && cy < kCentre &&
         cx > -kCentre && cx < kCentre;
}

// py = cy + ((Bm * u2 + A * v2) >> 1),  px = cx + ((A * u2 - Bm * v2) >> 1) with v2 = 2 a -
// (tile - 1), u2 = 2 b - (tile - 1) (32 x 32 -> 64-bit products).  For a valid row |py|, |px| <
// 2^46 + 2^36: the integer part (+ 1) fits an int.  -> (py, px)
DDLPC_HDI Index2<long long> warp_coord(long long cy, long long cx, int A, int Bm, int tile, int a, int b) {
  const int v2 = 2 * a - (tile - 1), u2 = 2 * b - (tile - 1);
  return {cy + (((long long)Bm * u2 + (long long)A * v2) >> 1),
          cx + (((long long)A * u2 - (long long)Bm * v2) >> 1)};
}

// iy = py >> 16 (the upper-left tap),  wy = float(py & 65535) * 2^-16 (exact),  the nearest
// pixel (py + 32768) >> 16
DDLPC_HDI int warp_tap(long long p) { return (int)(p >> 16); }
DDLPC_HDI float warp_weight(long long p) { return (float)(int)(p & 65535) * (1.0f / 65536.0f); }
DDLPC_HDI int warp_nearest(long long p) { return (int)((p + 32768) >> 16); }

// v = u8 / 255 (IEEE division)
DDLPC_HDI float u8_unit(uint32_t u8) { return div_rn((float)u8, 255.0f); }

// clamp(round(v * gain) + bias, 0, 1)
DDLPC_HDI float color_clamp(float v, float gain, float bias) {
  return fminf(fmaxf(add_rn(mul_rn(v, gain), bias), 0.f), 1.f);
}

// top = p00 + (p01 - p00) * wx,  bot = p10 + (p11 - p10) * wx,  val = top + (bot - top) * wy
DDLPC_HDI float bilinear(float p00, float p01, float p10, float p11, float wx, float wy) {
  const float top = add_rn(p00, mul_rn(sub_rn(p01, p00), wx));
  const float bot = add_rn(p10, mul_rn(sub_rn(p11, p10), wx));
  return add_rn(top, mul_rn(sub_rn(bot, top), wy));
}

}  // namespace ddlpc
