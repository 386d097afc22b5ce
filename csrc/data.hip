// Device-side input pipeline — K20 of SURVEY.md §2.5 (input normalise + layout).
//
// Reference: every micro-batch is a host tensor `float32/255`, reshaped to NCHW and copied
// to the GPU (ref.py:737,741,754-755); the dataset is re-read from disk every epoch
// (ref.py:732).  Here the batch is produced directly in HBM, in the layout the first conv
// consumes (channel-last bf16, channels zero-padded to 8 = one 16-byte pixel for its
// LDS-DMA), by ONE kernel per batch:
//
//   * synth_tiles_kernel: the synthetic Vaihingen-shape generator (benchmark / no-data source)
//   * tile_gather_kernel: a real dataset uploaded ONCE to HBM as uint8 NHWC, gathered per batch
//   * crop_params_kernel + crop_gather_kernel: augmented random crops of whole scenes
//   * warp_params_kernel + warp_gather_kernel: the same crops under a random zoom and rotation
//
// Their bit-exact recipe is written in data_math.h, as the host+device functions that the
// kernels below and their CPU twins (cpu_ref.cpp) call.
#include "common.h"
#include "data_math.h"
#include "ops.h"

namespace ddlpc {

namespace {

// The kernel spells its recipe itself, over mix32 / u24 / add_rn / mul_rn (data_math.h, whose
// header says why), as does its CPU twin.
// One thread per pixel; spatial = tile^dims pixels per sample, row-major (d, h, w).
// POW2 (tile a power of two and B * tile^dims < 2^31, the benchmark shapes): the pixel
// geometry by 32-bit shifts and masks instead of 64-bit divisions (which made the kernel
// ALU-bound: 230 us for a 384 x 256^2 batch); the same integers, so the same bits
template <bool POW2>
__global__ __launch_bounds__(256) void synth_tiles_kernel(
    const int64_t* __restrict__ idx, int B, uint32_t seed, int classes, int in_ch, int tile,
    int dims, int grid, float k, const float* __restrict__ palette, int cpad,
    bf16_t* __restrict__ x, int64_t* __restrict__ y) {
  const long long S = dims == 3 ? (long long)tile * tile * tile : (long long)tile * tile;
  const long long total = (long long)B * S;
  const uint32_t skey = mix32(seed ^ 0x9E3779B9u);
  const int lt = POW2 ? __builtin_ctz((unsigned)tile) : 0;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    int b, w, h, d, cw, ch, cd;
    long long p;
    if constexpr (POW2) {
      const unsigned e32 = (unsigned)e, m = (unsigned)tile - 1u;
      b = (int)(e32 >> (lt * dims));
      p = (long long)(e32 & ((1u << (lt * dims)) - 1u));
      w = (int)(e32 & m);
      h = (int)((e32 >> lt) & m);
      d = dims == 3 ? (int)((e32 >> (2 * lt)) & m) : 0;
      cw = (w * grid) >> lt; ch = (h * grid) >> lt; cd = (d * grid) >> lt;
    } else {
      b = (int)(e / S);
      p = e - (long long)b * S;
      w = (int)(p % tile);
      const long long q = p / tile;
      h = (int)(q % tile);
      d = dims == 3 ? (int)(q / tile) : 0;
      cw = (w * grid) / tile; ch = (h * grid) / tile; cd = (d * grid) / tile;
    }
    const uint32_t key = mix32(skey ^ (uint32_t)idx[b]);
    const uint32_t cell = (uint32_t)((cd * grid + ch) * grid + cw);
    const int lab = (int)(mix32(key ^ mix32(cell + 0x632BE5ABu)) % (uint32_t)classes);
    y[e] = lab;
    float f[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float v = 0.f;
      if (c < in_ch) {
        const uint32_t base = key ^ mix32((uint32_t)(p * 8 + c) + 0x1B873593u);
        float s = u24(mix32(base));
        s = add_rn(s, u24(mix32(base + 0x9E3779B9u)));
        s = add_rn(s, u24(mix32(base + 2u * 0x9E3779B9u)));
        s = add_rn(s, u24(mix32(base + 3u * 0x9E3779B9u)));
        const float n = mul_rn(add_rn(s, -2.0f), k);
        v = fminf(fmaxf(add_rn(palette[lab * in_ch + c], n), 0.f), 1.f);
      }
      f[c] = v;
    }
    if (cpad == 8) {
      reinterpret_cast<uint4*>(x)[e] = pack8(f);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < cpad) x[e * cpad + c] = f2bf(f[c]);
    }
  }
}

__global__ __launch_bounds__(256) void tile_gather_kernel(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ lab, const int64_t* __restrict__ idx,
    int B, long long S, int in_ch, int cpad, long long N, bf16_t* __restrict__ x,
    int64_t* __restrict__ y) {
  const long long total = (long long)B * S;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(e / S);
    const long long p = e - (long long)b * S;
    const long long n = idx[b];
    // an out-of-range sample index reads nothing: zero image, label -100 (CrossEntropy's
    // ignore_index).  Host indices are range-checked by DeviceTileDataset.get first; device
    // indices cannot raise without a blocking read-back
    const bool in_range = n >= 0 && n < N;
    const long long sp = in_range ? n * S + p : 0;
    y[e] = in_range ? (int64_t)lab[sp] : (int64_t)-100;
    float f[8];
#pragma unroll
    for (int c = 0; c < 8; ++c)
      f[c] = (c < in_ch && in_range) ? u8_unit(src[sp * in_ch + c]) : 0.f;
    if (cpad == 8) {
      reinterpret_cast<uint4*>(x)[e] = pack8(f);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < cpad) x[e * cpad + c] = f2bf(f[c]);
    }
  }
}

int data_grid(long long total) {
  return (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, 16384));
}

// ---- augmented random crops -------------------------------------------------------------
// one thread per virtual sample number: the recipe of data_math.h
__global__ __launch_bounds__(256) void crop_params_kernel(
    const int64_t* __restrict__ idx, int B, const int64_t* __restrict__ cum,
    const int64_t* __restrict__ table, int n, uint32_t seed, int tile, int mode, float gj, float bj,
    int* __restrict__ params, float* __restrict__ color) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const uint32_t key = sample_key(seed, (uint64_t)idx[i]);
  const int lo = pick_scene(cum, n, draw(key, 0));
  const long long H = table[3 * lo + 1], W = table[3 * lo + 2];
  params[4 * i] = lo;
  params[4 * i + 1] = (int)scale_draw(draw(key, 1), origin_count(H, tile));
  params[4 * i + 2] = (int)scale_draw(draw(key, 2), origin_count(W, tile));
  params[4 * i + 3] = symmetry_code(draw(key, 3), mode);
  color_jitter(draw(key, 4), draw(key, 5), gj, bj, color + 2 * i);
}

__global__ __launch_bounds__(256) void warp_params_kernel(
    const int64_t* __restrict__ idx, int B, const int64_t* __restrict__ cum,
    const int64_t* __restrict__ table, int n, const int* __restrict__ steps, int S,
    const int* __restrict__ rot, int T, uint32_t seed, int tile, int mode, float gj, float bj,
    int64_t* __restrict__ wparams, float* __restrict__ color) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const uint32_t key = sample_key(seed, (uint64_t)idx[i]);
  const int lo = pick_scene(cum, n, draw(key, 0));
  const long long H = table[3 * lo + 1], W = table[3 * lo + 2];
  const long long step = steps[(int)scale_draw(draw(key, 6), (uint64_t)S)];
  const int k = (int)scale_draw(draw(key, 7), (uint64_t)T);
  const long long c = rot[2 * k], sn = rot[2 * k + 1];
  const long long F = footprint(tile, step);
  int64_t* w = wparams + 6 * (long long)i;
  w[0] = lo;
  w[1] = footprint_centre(draw(key, 1), H, F);
  w[2] = footprint_centre(draw(key, 2), W, F);
  w[3] = symmetry_code(draw(key, 3), mode);
  w[4] = matrix_entry(step, c);
  w[5] = matrix_entry(step, sn);
  color_jitter(draw(key, 4), draw(key, 5), gj, bj, color + 2 * i);
}

constexpr int kCropBS = 32;                  // output pixels per workgroup: kCropBS^2

// One workgroup (256 threads) per kCropBS^2 block of one sample's output pixels; lanes run
// along ox, so every output row segment is one 16-byte store per lane.
//   * codes without bit 4: a lane's source pixel moves by +-1 column with ox — the source row
//     is read forwards or backwards, coalesced; straight from HBM.
//   * codes with bit 4 (transposing): source COLUMN = f(oy), source ROW = f(ox).  With
//     LDS_T the block's source pixels are first read with lanes along the source row
//     (coalesced) into LDS as raw bytes, s[ox][oy], and the output phase reads s transposed;
//     rows padded to kCropBS + 1 entries: the transposed 8-byte read then touches 64 distinct
//     banks per 32-lane half, the 4-byte label read 32.  Without LDS_T adjacent lanes read
//     pixels W * in_ch bytes apart.
// The per-sample code is uniform in a workgroup, so no branch below diverges inside a wave.
template <bool LDS_T>
__global__ __launch_bounds__(256) void crop_gather_kernel(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ lab,
    const int64_t* __restrict__ table, int n, long long total_px, const int* __restrict__ params,
    const float* __restrict__ color, int nb, int in_ch, int tile, int cpad,
    bf16_t* __restrict__ x, int64_t* __restrict__ y) {
  __shared__ uint2 s_px[kCropBS][kCropBS + 1];
  __shared__ uint32_t s_lab[kCropBS][kCropBS + 1];
  const int blk = blockIdx.x;
  const int b = blk / (nb * nb);
  const int rem = blk - b * nb * nb;
  const int by = rem / nb, bx = rem - by * nb;
  const int lx = threadIdx.x & (kCropBS - 1), ly0 = threadIdx.x / kCropBS;
  constexpr int kRows = 256 / kCropBS;       // block rows covered per pass
  const int sc = params[4 * b];
  const bool listed = sc >= 0 && sc < n;
  const int oy0 = params[4 * b + 1], ox0 = params[4 * b + 2], code = params[4 * b + 3] & 7;
  const long long off = listed ? table[3 * sc] : 0;
  const long long Hl = listed ? table[3 * sc + 1] : 1, Wl = listed ? table[3 * sc + 2] : 1;
  const bool valid = listed && Hl >= 1 && Wl >= 1 && Hl < (1 << 30) && Wl < (1 << 30) && off >= 0 &&
                     off <= total_px && Hl * Wl <= total_px - off;     // scene_row_valid, spelled out
  const int H = valid ? (int)Hl : 1, W = valid ? (int)Wl : 1;
  const bool has_color = color != nullptr;
  const float gain = has_color ? color[2 * b] : 1.f, bias = has_color ? color[2 * b + 1] : 0.f;
  const bool staged = LDS_T && valid && (code & 4);
  if (staged) {
    // load role: r = ox - block origin (source row), lanes c = oy - block origin (source column)
    for (int r = ly0; r < kCropBS; r += kRows) {
      const int ox = bx * kCropBS + r, oy = by * kCropBS + lx;
      if (ox < tile && oy < tile) {
        const int a = (code & 2) ? tile - 1 - ox : ox;
        const int c = (code & 1) ? tile - 1 - oy : oy;
        const long long sp = off + (long long)reflect_fast(oy0 + a, H) * W + reflect_fast(ox0 + c, W);
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int ch = 0; ch < 8; ++ch)
          if (ch < in_ch) w[ch >> 2] |= (uint32_t)src[sp * in_ch + ch] << (8 * (ch & 3));
        s_px[r][lx] = make_uint2(w[0], w[1]);
        s_lab[r][lx] = lab[sp];
      }
    }
    __syncthreads();
  }
  for (int ly = ly0; ly < kCropBS; ly += kRows) {
    const int oy = by * kCropBS + ly, ox = bx * kCropBS + lx;
    if (oy >= tile || ox >= tile) continue;
    const long long e = ((long long)b * tile + oy) * tile + ox;
    uint32_t w[2] = {0u, 0u};
    int64_t l = -100;
    if (staged) {
      const uint2 v = s_px[lx][ly];
      w[0] = v.x; w[1] = v.y;
      l = (int64_t)s_lab[lx][ly];
    } else if (valid) {
      int a = (code & 4) ? ox : oy, c = (code & 4) ? oy : ox;
      if (code & 2) a = tile - 1 - a;
      if (code & 1) c = tile - 1 - c;
      const long long sp = off + (long long)reflect_fast(oy0 + a, H) * W + reflect_fast(ox0 + c, W);
#pragma unroll
      for (int ch = 0; ch < 8; ++ch)
        if (ch < in_ch) w[ch >> 2] |= (uint32_t)src[sp * in_ch + ch] << (8 * (ch & 3));
      l = (int64_t)lab[sp];
    }
    y[e] = l;
    float f[8];
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
      float v = 0.f;
      if (ch < in_ch && valid) {
        v = u8_unit((w[ch >> 2] >> (8 * (ch & 3))) & 0xffu);
        if (has_color) v = color_clamp(v, gain, bias);
      }
      f[ch] = v;
    }
    if (cpad == 8) {
      reinterpret_cast<uint4*>(x)[e] = pack8(f);
    } else {
#pragma unroll
      for (int ch = 0; ch < 8; ++ch)
        if (ch < cpad) x[e * cpad + ch] = f2bf(f[ch]);
    }
  }
}

// warp_gather: crop_gather's work split (one workgroup per kCropBS^2 output block of one sample,
// lanes along ox, one 16-byte store per pixel); the sample's code and matrix are uniform in a
// workgroup.  A lane's source coordinate moves by (Bm, A) per ox (or (A, -Bm) for the
// transposing codes): at zooms near 1 neighbouring lanes read neighbouring source pixels, so
// the 4 taps and the label come straight from global memory (L2 serves the re-reads).
__global__ __launch_bounds__(256) void warp_gather_kernel(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ lab,
    const int64_t* __restrict__ table, int n, long long total_px, const int64_t* __restrict__ wparams,
    const float* __restrict__ color, int nb, int in_ch, int tile, int cpad,
    bf16_t* __restrict__ x, int64_t* __restrict__ y) {
  const int blk = blockIdx.x;
  const int b = blk / (nb * nb);
  const int rem = blk - b * nb * nb;
  const int by = rem / nb, bx = rem - by * nb;
  const int lx = threadIdx.x & (kCropBS - 1), ly0 = threadIdx.x / kCropBS;
  constexpr int kRows = 256 / kCropBS;
  const int64_t* wp = wparams + 6 * (long long)b;
  const long long sc = wp[0], cy = wp[1], cx = wp[2], Al = wp[4], Bl = wp[5];
  const int code = (int)wp[3] & 7;
  const bool listed = sc >= 0 && sc < n;
  const long long off = listed ? table[3 * sc] : 0;
  const long long Hl = listed ? table[3 * sc + 1] : 1, Wl = listed ? table[3 * sc + 2] : 1;
  // scene_row_valid && warp_row_valid and, below, d4_forward, spelled out (data_math.h says why)
  const bool valid = listed && Hl >= 1 && Wl >= 1 && Hl < (1 << 30) && Wl < (1 << 30) && off >= 0 &&
                     off <= total_px && Hl * Wl <= total_px - off && Al >= -kCoef && Al <= kCoef &&
                     Bl >= -kCoef && Bl <= kCoef && cy > -kCentre && cy < kCentre && cx > -kCentre &&
                     cx < kCentre;
  const int H = valid ? (int)Hl : 1, W = valid ? (int)Wl : 1;
  const int A = valid ? (int)Al : 0, Bm = valid ? (int)Bl : 0;     // 32 x 32 -> 64-bit products
  const bool has_color = color != nullptr;
  const float gain = has_color ? color[2 * b] : 1.f, bias = has_color ? color[2 * b + 1] : 0.f;
  for (int ly = ly0; ly < kCropBS; ly += kRows) {
    const int oy = by * kCropBS + ly, ox = bx * kCropBS + lx;
    if (oy >= tile || ox >= tile) continue;
    const long long e = ((long long)b * tile + oy) * tile + ox;
    float f[8];
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) f[ch] = 0.f;
    int64_t l = -100;
    if (valid) {
      int a = (code & 4) ? ox : oy, c = (code & 4) ? oy : ox;
      if (code & 2) a = tile - 1 - a;
      if (code & 1) c = tile - 1 - c;
      const Index2<long long> p = warp_coord(cy, cx, A, Bm, tile, a, c);
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

void crop_params_launch(const int64_t* idx, int B, const int64_t* cum, const int64_t* table, int n,
                        uint32_t seed, int tile, int mode, float gain_jitter, float bias_jitter,
                        int* params, float* color, hipStream_t st) {
  hipLaunchKernelGGL(crop_params_kernel, dim3((B + 255) / 256), dim3(256), 0, st, idx, B, cum, table,
                     n, seed, tile, mode, gain_jitter, bias_jitter, params, color);
}

int crop_gather_blocks(int tile) { return (tile + kCropBS - 1) / kCropBS; }

void warp_params_launch(const int64_t* idx, int B, const int64_t* cum, const int64_t* table, int n,
                        const int* steps, int S, const int* rot, int T, uint32_t seed, int tile,
                        int mode, float gain_jitter, float bias_jitter, int64_t* wparams, float* color,
                        hipStream_t st) {
  hipLaunchKernelGGL(warp_params_kernel, dim3((B + 255) / 256), dim3(256), 0, st, idx, B, cum, table,
                     n, steps, S, rot, T, seed, tile, mode, gain_jitter, bias_jitter, wparams, color);
}

void warp_gather_launch(const uint8_t* src, const uint8_t* lab, const int64_t* table, int n,
                        long long total_px, const int64_t* wparams, const float* color, int B,
                        int in_ch, int tile, int cpad, bf16_t* x, int64_t* y, hipStream_t st) {
  const int nb = crop_gather_blocks(tile);
  hipLaunchKernelGGL(warp_gather_kernel, dim3((unsigned)((long long)B * nb * nb)), dim3(256), 0, st, src,
                     lab, table, n, total_px, wparams, color, nb, in_ch, tile, cpad, x, y);
}

void crop_gather_launch(const uint8_t* src, const uint8_t* lab, const int64_t* table, int n,
                        long long total_px, const int* params, const float* color, int B, int in_ch,
                        int tile, int cpad, bool lds_transpose, bf16_t* x, int64_t* y, hipStream_t st) {
  const int nb = crop_gather_blocks(tile);
  const dim3 grid((unsigned)((long long)B * nb * nb));
  if (lds_transpose)
    hipLaunchKernelGGL(crop_gather_kernel<true>, grid, dim3(256), 0, st, src, lab, table, n, total_px,
                       params, color, nb, in_ch, tile, cpad, x, y);
  else
    hipLaunchKernelGGL(crop_gather_kernel<false>, grid, dim3(256), 0, st, src, lab, table, n, total_px,
                       params, color, nb, in_ch, tile, cpad, x, y);
}

void synth_tiles_launch(const int64_t* idx, int B, uint32_t seed, int classes, int in_ch, int tile,
                        int dims, int grid, float k, const float* palette, int cpad, bf16_t* x,
                        int64_t* y, hipStream_t st) {
  const long long S = dims == 3 ? (long long)tile * tile * tile : (long long)tile * tile;
  const bool pow2 = tile > 0 && (tile & (tile - 1)) == 0 && (long long)B * S < (1LL << 31);
  if (pow2)
    hipLaunchKernelGGL(synth_tiles_kernel<true>, dim3(data_grid(B * S)), dim3(256), 0, st, idx, B, seed,
                       classes, in_ch, tile, dims, grid, k, palette, cpad, x, y);
  else
    hipLaunchKernelGGL(synth_tiles_kernel<false>, dim3(data_grid(B * S)), dim3(256), 0, st, idx, B, seed,
                       classes, in_ch, tile, dims, grid, k, palette, cpad, x, y);
}

void tile_gather_launch(const uint8_t* src, const uint8_t* lab, const int64_t* idx, int B,
                        long long S, int in_ch, int cpad, long long N, bf16_t* x, int64_t* y,
                        hipStream_t st) {
  hipLaunchKernelGGL(tile_gather_kernel, dim3(data_grid(B * S)), dim3(256), 0, st, src, lab, idx, B,
                     S, in_ch, cpad, N, x, y);
}

}  // namespace ddlpc
