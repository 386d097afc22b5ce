// Elastic deformation of the device-cut training crops: a smooth random displacement field (cubic
// B-spline over a coarse per-sample control lattice) in front of warp_gather's coordinate.
//
//   * elastic_field_kernel: the control lattice of every sample of a batch, one thread per value
//   * elastic_gather_kernel: warp_gather with the displaced coordinate (elastic_coord)
//
// The bit-exact recipe is written in data_math.h (spline table, control lattice, the two rounded
// spline stages, the coordinate); the CPU twins (cpu_ref.cpp) call the same functions.
#include "common.h"
#include "data_math.h"
#include "ops.h"

namespace ddlpc {

namespace {

constexpr int kBS = 32;                          // output pixels per workgroup: kBS^2 (= data.hip)
constexpr int kG3 = kElasticMaxGrid + 3;         // lattice points per side, at most

__global__ __launch_bounds__(256) void elastic_field_kernel(const int64_t* __restrict__ idx, int total,
                                                            uint32_t seed, int amp, int per,
                                                            int* __restrict__ ctrl) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int b = e / per, r = e - b * per;        // per = 2 (grid + 3)^2 values per sample
  ctrl[e] = elastic_control(sample_key(seed, (uint64_t)idx[b]), r >> 1, r & 1, amp);
}

// warp_gather's work split: one workgroup (256 threads) per kBS^2 block of one sample's output
// pixels, lanes along ox, one 16-byte store per pixel, the sample's code and matrix uniform in a
// workgroup; the 4 taps and the label come straight from global memory.
//
// TWO_STAGE (the shipped form): the block's pixels span kBS values of a and kBS values of b, so the
// first spline stage (along b) is shared by all pixels of a column b and is done once per block:
//   1. the sample's lattice -> s_ctrl (clamped, one int2 (dy, dx) per point, <= 19 x 19); the
//      spline rows of the block's kBS a values -> s_ra, of its kBS b values -> s_rb (spline_row;
//      lanes 0..31 of wave 0 load s_ra and reduce the cell range [cmin, cmax] of the block by
//      shuffles, lanes 32..63 load s_rb).  Past the tile's edge the rows repeat the edge's.
//   2. s_T[r][bl] = spline_stage(w_b(bl), s_ctrl[cmin + r][cell_b(bl) + 0..3]) for the lattice
//      rows r = 0 .. cmax + 3 - cmin the block touches and its kBS columns bl, both axes per
//      thread: at most 19 x 32 int2 over 256 threads.
//   3. a pixel reads s_T[cell_a - cmin + 0..3][bl] and the row of a: 8 multiply-adds for the
//      two axes, against 40 for the direct tensor product.  The same sums with the same rounding
//      as elastic_displace, so the same bits.
// LDS banks (64 banks of 4 bytes; an 8-byte read is served per 32-lane half): s_T rows are
// padded to kBS + 1 int2 = 66 words.
//   * codes without bit 4 — bl = lx, one a per half-wave: lane lx reads words 66 r + 2 lx, + 1:
//     64 consecutive words, every bank once.  s_ra[ly] is one address (a broadcast).
//   * codes with bit 4 (transposing) — bl = ly is uniform in a half-wave and r = cell_a(lx) - cmin
//     + j takes one value per spline cell the 32 lanes cross: lanes of one r read one address,
//     different r are 66 (r' - r) words apart = banks 2 (r' - r) further, distinct for up to 32
//     rows (<= 19 exist).  Unpadded (64 words) every r would hit the same two banks.  s_ra[lx] is
//     read at a stride of 5 words: 5 lx mod 64 is distinct over 32 lanes.
//   * step 2's writes: a wave covers two r and all bl: words 66 r + 2 bl, + 1, consecutive.
// Without TWO_STAGE (knob ELASTIC_LDS = 0, kept for scripts/crop_micro.py's A/B) every pixel
// evaluates elastic_displace on the lattice and the table in global memory.
// No branch below diverges inside a wave beyond warp_gather's: valid, code and the row range are
// uniform in a workgroup.
template <bool TWO_STAGE>
__global__ __launch_bounds__(256) void elastic_gather_kernel(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ lab,
    const int64_t* __restrict__ table, int n, long long total_px, const int64_t* __restrict__ wparams,
    const float* __restrict__ color, const int* __restrict__ ctrl, int grid,
    const int* __restrict__ spline, int nb, int in_ch, int tile, int cpad, bf16_t* __restrict__ x,
    int64_t* __restrict__ y) {
  __shared__ int2 s_ctrl[kG3 * kG3];
  __shared__ int2 s_T[kG3][kBS + 1];
  __shared__ int s_ra[kBS][5], s_rb[kBS][5];
  __shared__ int s_range[2];
  const int blk = blockIdx.x;
  const int b = blk / (nb * nb);
  const int rem = blk - b * nb * nb;
  const int by = rem / nb, bx = rem - by * nb;
  const int tid = threadIdx.x;
  const int lx = tid & (kBS - 1), ly0 = tid / kBS;
  constexpr int kRows = 256 / kBS;
  const int64_t* wp = wparams + 6 * (long long)b;
  const long long sc = wp[0], cy = wp[1], cx = wp[2], Al = wp[4], Bl = wp[5];
  const int code = (int)wp[3] & 7;
  const bool listed = sc >= 0 && sc < n;
  const long long off = listed ? table[3 * sc] : 0;
  const long long Hl = listed ? table[3 * sc + 1] : 1, Wl = listed ? table[3 * sc + 2] : 1;
  // scene_row_valid && warp_row_valid and, below, d4_forward, spelled out as in warp_gather_kernel
  const bool valid = listed && Hl >= 1 && Wl >= 1 && Hl < (1 << 30) && Wl < (1 << 30) && off >= 0 &&
                     off <= total_px && Hl * Wl <= total_px - off && Al >= -kCoef && Al <= kCoef &&
                     Bl >= -kCoef && Bl <= kCoef && cy > -kCentre && cy < kCentre && cx > -kCentre &&
                     cx < kCentre;
  const int H = valid ? (int)Hl : 1, W = valid ? (int)Wl : 1;
  const int A = valid ? (int)Al : 0, Bm = valid ? (int)Bl : 0;
  const bool has_color = color != nullptr;
  const float gain = has_color ? color[2 * b] : 1.f, bias = has_color ? color[2 * b + 1] : 0.f;
  const int g3 = grid + 3;
  const int* lattice = ctrl + (long long)b * g3 * g3 * 2;
  const bool tr = (code & 4) != 0;
  int cmin = 0;
  if (TWO_STAGE && valid) {
    for (int i = tid; i < g3 * g3; i += 256) {
      const int2 v = reinterpret_cast<const int2*>(lattice)[i];
      s_ctrl[i] = make_int2(ctrl_clamp(v.x), ctrl_clamp(v.y));
    }
    if (tid < 2 * kBS) {                         // wave 0: lanes 0..31 the a rows, 32..63 the b rows
      const bool isb = tid >= kBS;
      // the output coordinate that local index lx stands for: a follows oy (ox when transposing)
      const int o = min(((isb != tr) ? bx : by) * kBS + lx, tile - 1);
      const int p = (code & (isb ? 1 : 2)) ? tile - 1 - o : o;
      const SplineRow r = spline_row(spline + 5 * p, grid);
      int* dst = isb ? s_rb[lx] : s_ra[lx];
      dst[0] = r.cell;
#pragma unroll
      for (int i = 0; i < 4; ++i) dst[1 + i] = r.w[i];
      int lo = r.cell, hi = r.cell;
#pragma unroll
      for (int m = 1; m < kBS; m <<= 1) {
        lo = min(lo, __shfl_xor(lo, m, kBS));
        hi = max(hi, __shfl_xor(hi, m, kBS));
      }
      if (tid == 0) { s_range[0] = lo; s_range[1] = hi; }
    }
    __syncthreads();
    cmin = s_range[0];
    const int items = (s_range[1] + 4 - cmin) * kBS;
    for (int e = tid; e < items; e += 256) {
      const int r = e / kBS, bl = e & (kBS - 1);
      const int* rb = s_rb[bl];
      const int2* c = s_ctrl + (cmin + r) * g3 + rb[0];
      const int2 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
      s_T[r][bl] = make_int2(spline_stage(rb + 1, c0.x, c1.x, c2.x, c3.x),
                             spline_stage(rb + 1, c0.y, c1.y, c2.y, c3.y));
    }
    __syncthreads();
  }
  for (int ly = ly0; ly < kBS; ly += kRows) {
    const int oy = by * kBS + ly, ox = bx * kBS + lx;
    if (oy >= tile || ox >= tile) continue;
    const long long e = ((long long)b * tile + oy) * tile + ox;
    float f[8];
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) f[ch] = 0.f;
    int64_t l = -100;
    if (valid) {
      int a = tr ? ox : oy, c = tr ? oy : ox;
      if (code & 2) a = tile - 1 - a;
      if (code & 1) c = tile - 1 - c;
      Index2<int> d;
      if (TWO_STAGE) {
        const int* ra = s_ra[tr ? lx : ly];
        const int2* t = &s_T[ra[0] - cmin][tr ? ly : lx];
        const int2 t0 = t[0], t1 = t[kBS + 1], t2 = t[2 * (kBS + 1)], t3 = t[3 * (kBS + 1)];
        d = {spline_stage(ra + 1, t0.x, t1.x, t2.x, t3.x), spline_stage(ra + 1, t0.y, t1.y, t2.y, t3.y)};
      } else {
        d = elastic_displace(lattice, grid, spline_row(spline + 5 * a, grid), spline_row(spline + 5 * c, grid));
      }
      const Index2<long long> p = elastic_coord(cy, cx, A, Bm, tile, a, c, d.a, d.b);
      const long long py = p.a, px = p.b;
      const int iy = warp_tap(py), ix = warp_tap(px);
      const float wy = warp_weight(py), wx = warp_weight(px);
      const long long r0 = off + (long long)reflect_fast(iy, H) * W;
      const long long r1 = off + (long long)reflect_fast(iy + 1, H) * W;
      const int c0 = reflect_fast(ix, W), c1 = reflect_fast(ix + 1, W);
      const uint8_t* q00 = src + (r0 + c0) * in_ch;
      const uint8_t* q01 = src + (r0 + c1) * in_ch;
      const uint8_t* q10 = src + (r1 + c0) * in_ch;
      const uint8_t* q11 = src + (r1 + c1) * in_ch;
#pragma unroll
      for (int ch = 0; ch < 8; ++ch)
        if (ch < in_ch) {
          const float p00 = (float)q00[ch], p01 = (float)q01[ch], p10 = (float)q10[ch], p11 = (float)q11[ch];
          float v = div_rn(bilinear(p00, p01, p10, p11, wx, wy), 255.0f);
          if (has_color) v = color_clamp(v, gain, bias);
          f[ch] = v;
        }
      const int ny = reflect_fast(warp_nearest(py), H), nx = reflect_fast(warp_nearest(px), W);
      l = (int64_t)lab[off + (long long)ny * W + nx];
    }
    y[e] = l;
    if (cpad == 8) {
      reinterpret_cast<uint4*>(x)[e] = pack8(f);
    } else {
#pragma unroll
      for (int ch = 0; ch < 8; ++ch)
        if (ch < cpad) x[e * cpad + ch] = f2bf(f[ch]);
    }
  }
}

}  // namespace

void elastic_field_launch(const int64_t* idx, int B, uint32_t seed, int amp, int grid, int* ctrl,
                          hipStream_t st) {
  const int per = 2 * (grid + 3) * (grid + 3), total = B * per;
  hipLaunchKernelGGL(elastic_field_kernel, dim3((total + 255) / 256), dim3(256), 0, st, idx, total, seed,
                     amp, per, ctrl);
}

void elastic_gather_launch(const uint8_t* src, const uint8_t* lab, const int64_t* table, int n,
                           long long total_px, const int64_t* wparams, const float* color,
                           const int* ctrl, int grid, const int* spline, int B, int in_ch, int tile,
                           int cpad, bool two_stage, bf16_t* x, int64_t* y, hipStream_t st) {
  const int nb = crop_gather_blocks(tile);
  const dim3 blocks((unsigned)((long long)B * nb * nb));
  if (two_stage)
    hipLaunchKernelGGL(elastic_gather_kernel<true>, blocks, dim3(256), 0, st, src, lab, table, n, total_px,
                       wparams, color, ctrl, grid, spline, nb, in_ch, tile, cpad, x, y);
  else
    hipLaunchKernelGGL(elastic_gather_kernel<false>, blocks, dim3(256), 0, st, src, lab, table, n, total_px,
                       wparams, color, ctrl, grid, spline, nb, in_ch, tile, cpad, x, y);
}

}  // namespace ddlpc
