// Device-side input pipeline — K20 of SURVEY.md §2.5 (input normalise + layout).
//
// Reference: every micro-batch is a host tensor `float32/255`, reshaped to NCHW and copied
// to the GPU (ref.py:737,741,754-755); the dataset is re-read from disk every epoch
// (ref.py:732).  Here the batch is produced directly in HBM, in the layout the first conv
// consumes (channel-last bf16, channels zero-padded to 8 = one 16-byte pixel for its
// LDS-DMA), by ONE kernel per batch:
//
//   * synth_tiles_kernel: the synthetic Vaihingen-shape generator (benchmark / no-data
//     source).  Sample i depends only on (seed, i): a counter-based hash (no RNG state),
//     so a batch is the same whichever rank, batch position or resume point renders it.
//     Recipe (the CPU twin in data/datasets.py computes the identical bits):
//       key     = mix(mix(seed ^ 0x9E3779B9) ^ i)
//       coarse  = mix(key ^ mix(cell + 0x632BE5AB)) % classes   on a grid^dims lattice
//       label   = coarse[(h*grid)/tile][(w*grid)/tile]           (nearest up-sampling)
//       u_j     = (mix(key ^ mix(p*8 + ch + 0x1B873593) + j*0x9E3779B9) >> 8) * 2^-24
//       x       = clamp(palette[label][ch] + (((u0+u1)+u2)+u3 - 2) * k, 0, 1)   -> bf16
//     (Irwin-Hall noise: k = noise*sqrt(3) gives std `noise`; every float op rounds on its
//     own — no FMA contraction — so the host twin matches bit for bit.)
//   * tile_gather_kernel: a real dataset uploaded ONCE to HBM as uint8 NHWC (+ uint8 label
//     maps): gather the batch's sample indices, /255 (IEEE division, as the reference's
//     numpy op), pad, bf16; labels widen to int64.
//   * crop_params_kernel + crop_gather_kernel: training on whole scenes.  The scenes are
//     uploaded ONCE, packed: uint8 pixels [total_pixels, in_ch], uint8 labels [total_pixels]
//     and an int64 table [n, 3] of (pixel offset, H, W) rows (a contiguous tile stack is
//     this packing with offset = n H W).  A batch is tile x tile random crops, augmented by
//     one of the 8 symmetries of the square and a per-sample gain / bias, cut in one pass.
//     Virtual sample s depends only on (seed, s), as the synthetic recipe (twin:
//     data/scenes.py crop_params_reference):
//       key   = mix(mix(mix(seed ^ 0xC2B2AE35) ^ lo32(s)) ^ mix(hi32(s) + 0x85EBCA6B))
//       r_j   = mix(key + (j + 1) * 0x9E3779B9)                       j = 0..5
//       scene = the k with cum[k] <= (r0 * cum[n]) >> 32 < cum[k + 1], cum = prefix sum of
//               the scenes' valid-origin counts ny * nx, ny = max(H - tile, 0) + 1 (crops are
//               uniform over all valid crops; cum[n] < 2^32)
//       y0    = (r1 * ny) >> 32,  x0 = (r2 * nx) >> 32
//       code  = 0 | r3 & 3 | r3 & 7                                   (none | flip | d4)
//       gain  = 1 + gain_jitter * (2 u24(r4) - 1),  bias = bias_jitter * (2 u24(r5) - 1)
//     crop_gather: output pixel (oy, ox) reads source pixel (y0 + a, x0 + b), mirrored into
//     the scene (reflect_index): (a, b) = (oy, ox); code & 4: swap a, b; code & 2: a = tile -
//     1 - a; code & 1: b = tile - 1 - b.  Value: v = u8 / 255, with colour clamp(round(v *
//     gain) + bias, 0, 1), every op rounded on its own, then bf16.
//   * warp_params_kernel + warp_gather_kernel: the same crops under a random zoom and a
//     rotation by an arbitrary angle — a resampling, where crop_gather is a permutation.
//     Coordinates are 16.16 fixed point in int64 (ONE = 65536; >> is arithmetic = floor).  The
//     zoom and the angle reach the kernels as two int32 tables the host builds in float64
//     (data/scenes.py): steps[S] = rint(ONE / z_k), z_k = zoom_min (zoom_max / zoom_min)^((k +
//     .5) / S) (log-uniform zoom; step = source pixels per output pixel) and rot[T] = (rint(cos
//     t_k ONE), rint(sin t_k ONE)), t_k = -rotate_deg + (k + .5) 2 rotate_deg / T — integers
//     only on the device, no pow / cos to match.  Twins: warp_params_reference /
//     warp_gather_reference.
//     warp_params: key, r_0..r_5, scene, code, gain, bias exactly as crop_params (the scene
//     choice keeps the unit-scale cum table: with zoom an approximation of "uniform over all
//     valid crops"), r_6, r_7 by the same rule, and
//       step  = steps[(r6 * S) >> 32],  (c, sn) = rot[(r7 * T) >> 32]
//       A     = (step * c + 32768) >> 16,  Bm = (step * sn + 32768) >> 16
//       F     = (tile * step + 65535) >> 16                 (the un-rotated source footprint)
//       ny    = max(H - F, 0) + 1,  y0 = (r1 * ny) >> 32,  cy = (2 y0 + F - 1) * 32768
//     and cx likewise from r2 and W: the un-rotated footprint lies inside a scene that is
//     large enough; whatever overhangs (small scenes, rotated corners) is mirrored.  Output:
//     wparams int64 [B, 6] = (scene, cy, cx, code, A, Bm), color fp32 [B, 2].
//     warp_gather: (a, b) from (oy, ox) and code as crop_gather;
//       v2 = 2 a - (tile - 1),  u2 = 2 b - (tile - 1)
//       py = cy + ((Bm * u2 + A * v2) >> 1),  px = cx + ((A * u2 - Bm * v2) >> 1)
//       iy = py >> 16,  wy = float(py & 65535) * 2^-16       (ix, wx likewise from px)
//     taps p00, p01, p10, p11 at rows reflect(iy), reflect(iy + 1), columns reflect(ix),
//     reflect(ix + 1); per channel, the u8 taps as fp32, every op rounded on its own:
//       top = p00 + (p01 - p00) * wx,  bot = p10 + (p11 - p10) * wx,  val = top + (bot - top) * wy
//     v = val / 255 (IEEE), the colour clamp of crop_gather, bf16.  Label: nearest,
//     lab[reflect((py + 32768) >> 16)][reflect((px + 32768) >> 16)].  A row whose scene is
//     not listed, whose table row fails crop_gather's checks, with |A| or |Bm| > 2^20 or |cy|
//     or |cx| >= 2^46 reads nothing (zero image, labels -100).  (A, Bm) = (ONE, 0) and cy = (2
//     y0 + tile - 1) * 32768 is crop_gather's (y0, x0) crop, bit for bit.
#include "common.h"
#include "ops.h"

namespace ddlpc {

namespace {

DDLPC_DEVICE uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

DDLPC_DEVICE float u24(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

// a separately rounded fp32 multiply: HIP's __fmul_rn is a plain operator that the default
// -ffp-contract=fast still fuses into the following add (the PyTorch twin rounds twice)
DDLPC_DEVICE float mul_rn(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// one thread per pixel; spatial = tile^dims pixels per sample, row-major (d, h, w).
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
        s = __fadd_rn(s, u24(mix32(base + 0x9E3779B9u)));
        s = __fadd_rn(s, u24(mix32(base + 2u * 0x9E3779B9u)));
        s = __fadd_rn(s, u24(mix32(base + 3u * 0x9E3779B9u)));
        const float n = mul_rn(__fadd_rn(s, -2.0f), k);
        v = fminf(fmaxf(__fadd_rn(palette[lab * in_ch + c], n), 0.f), 1.f);
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
      f[c] = (c < in_ch && in_range) ? __fdiv_rn((float)src[sp * in_ch + c], 255.0f) : 0.f;
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
// the draws of virtual sample s (the recipe in the header), shared by crop_params and warp_params
DDLPC_DEVICE uint32_t sample_key(uint32_t seed, uint64_t s) {
  const uint32_t skey = mix32(seed ^ 0xC2B2AE35u);
  return mix32(mix32(skey ^ (uint32_t)s) ^ mix32((uint32_t)(s >> 32) + 0x85EBCA6Bu));
}

DDLPC_DEVICE uint32_t draw(uint32_t key, int j) { return mix32(key + (uint32_t)(j + 1) * 0x9E3779B9u); }

// the scene with cum[lo] <= (r0 * cum[n]) >> 32 < cum[lo + 1]
DDLPC_DEVICE int pick_scene(const int64_t* __restrict__ cum, int n, uint32_t r0) {
  const uint64_t t = ((uint64_t)r0 * (uint64_t)cum[n]) >> 32;
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((uint64_t)cum[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

DDLPC_DEVICE int symmetry_code(uint32_t r3, int mode) {
  return mode == 0 ? 0 : (int)(r3 & (mode == 1 ? 3u : 7u));
}

DDLPC_DEVICE void color_jitter(uint32_t r4, uint32_t r5, float gj, float bj, float* __restrict__ color) {
  color[0] = __fadd_rn(1.0f, mul_rn(gj, __fadd_rn(mul_rn(2.0f, u24(r4)), -1.0f)));
  color[1] = mul_rn(bj, __fadd_rn(mul_rn(2.0f, u24(r5)), -1.0f));
}

// one thread per virtual sample number: see the recipe in the header
__global__ __launch_bounds__(256) void crop_params_kernel(
    const int64_t* __restrict__ idx, int B, const int64_t* __restrict__ cum,
    const int64_t* __restrict__ table, int n, uint32_t seed, int tile, int mode, float gj, float bj,
    int* __restrict__ params, float* __restrict__ color) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const uint32_t key = sample_key(seed, (uint64_t)idx[i]);
  const int lo = pick_scene(cum, n, draw(key, 0));
  const long long H = table[3 * lo + 1], W = table[3 * lo + 2];
  const uint64_t ny = (uint64_t)(H > tile ? H - tile : 0) + 1u;
  const uint64_t nx = (uint64_t)(W > tile ? W - tile : 0) + 1u;
  params[4 * i] = lo;
  params[4 * i + 1] = (int)(((uint64_t)draw(key, 1) * ny) >> 32);
  params[4 * i + 2] = (int)(((uint64_t)draw(key, 2) * nx) >> 32);
  params[4 * i + 3] = symmetry_code(draw(key, 3), mode);
  color_jitter(draw(key, 4), draw(key, 5), gj, bj, color + 2 * i);
}

// 16.16 centre of an F-pixel footprint whose origin is drawn from max(size - F, 0) + 1
// positions.  Unsigned arithmetic: a wild table entry wraps (warp_gather then rejects the row)
DDLPC_DEVICE long long footprint_centre(uint32_t r, long long size, long long F) {
  const uint64_t cnt = (size > F ? (uint64_t)size - (uint64_t)F : 0u) + 1u;
  const uint64_t o = ((uint64_t)r * cnt) >> 32;
  return (long long)((2u * o + (uint64_t)F - 1u) * 32768u);
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
  const long long step = steps[(int)(((uint64_t)draw(key, 6) * (uint64_t)S) >> 32)];
  const int k = (int)(((uint64_t)draw(key, 7) * (uint64_t)T) >> 32);
  const long long c = rot[2 * k], sn = rot[2 * k + 1];
  const long long F = ((long long)tile * step + 65535) >> 16;
  int64_t* w = wparams + 6 * (long long)i;
  w[0] = lo;
  w[1] = footprint_centre(draw(key, 1), H, F);
  w[2] = footprint_centre(draw(key, 2), W, F);
  w[3] = symmetry_code(draw(key, 3), mode);
  w[4] = (step * c + 32768) >> 16;
  w[5] = (step * sn + 32768) >> 16;
  color_jitter(draw(key, 4), draw(key, 5), gj, bj, color + 2 * i);
}

// reflect_index without the division for a coordinate already inside the scene (all of them,
// for a crop that does not overhang)
DDLPC_DEVICE int reflect_fast(int i, int n) {
  return (unsigned)i < (unsigned)n ? i : reflect_index(i, n);
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
  // a scene outside [0, n) reads nothing, nor does a table row that does not lie inside the
  // pixel buffer (the table is device data: the host cannot check it without a read-back)
  const bool valid = listed && Hl >= 1 && Wl >= 1 && Hl < (1 << 30) && Wl < (1 << 30) && off >= 0 &&
                     off <= total_px && Hl * Wl <= total_px - off;
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
        v = __fdiv_rn((float)((w[ch >> 2] >> (8 * (ch & 3))) & 0xffu), 255.0f);
        if (has_color) v = fminf(fmaxf(__fadd_rn(mul_rn(v, gain), bias), 0.f), 1.f);
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
  constexpr long long kCoef = 1LL << 20, kCentre = 1LL << 46;
  // crop_gather's checks, and a matrix / centre small enough that every coordinate below
  // stays far inside int64 and its integer part inside int
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
      const int v2 = 2 * a - (tile - 1), u2 = 2 * c - (tile - 1);
      const long long py = cy + (((long long)Bm * u2 + (long long)A * v2) >> 1);
      const long long px = cx + (((long long)A * u2 - (long long)Bm * v2) >> 1);
      // |py|, |px| < 2^46 + 2^36: the integer part (+ 1) fits an int; H, W < 2^30
      const int iy = (int)(py >> 16), ix = (int)(px >> 16);
      const float wy = (float)(int)(py & 65535) * (1.0f / 65536.0f);       // exact
      const float wx = (float)(int)(px & 65535) * (1.0f / 65536.0f);
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
          const float top = __fadd_rn(p00, mul_rn(__fsub_rn(p01, p00), wx));
          const float bot = __fadd_rn(p10, mul_rn(__fsub_rn(p11, p10), wx));
          float v = __fdiv_rn(__fadd_rn(top, mul_rn(__fsub_rn(bot, top), wy)), 255.0f);
          if (has_color) v = fminf(fmaxf(__fadd_rn(mul_rn(v, gain), bias), 0.f), 1.f);
          f[ch] = v;
        }
      const int ny = reflect_fast((int)((py + 32768) >> 16), H), nx = reflect_fast((int)((px + 32768) >> 16), W);
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
