// Argument checks of the input / prediction pipeline operators, one function per operator, called
// by both registrations (bindings.cpp, cpu_ref.cpp): dtype, rank, shape relations, ranges,
// same-device, symmetry-code values.  What depends on the backend stays with it: is_cuda,
// contiguity (the CPU twins call .contiguous()), grid limits, alignment, the GPU's code-list cache.
#pragma once

#include <ATen/ATen.h>

#include <cstdint>

namespace ddlpc {
namespace checks {

using T = const at::Tensor&;
using OptT = const c10::optional<at::Tensor>&;

inline bool has(OptT t) { return t.has_value() && t->defined(); }

inline void channels(int64_t in_ch, int64_t cpad) {
  TORCH_CHECK(in_ch >= 1 && in_ch <= 8 && cpad >= in_ch && cpad <= 8, "1 <= in_ch <= cpad <= 8");
}

inline void tile_range(int64_t tile) { TORCH_CHECK(tile >= 1 && tile <= 32768, "tile out of range"); }

inline void synth_tiles(T idx, int64_t classes, int64_t in_ch, int64_t tile, int64_t dims, int64_t grid,
                        T palette, int64_t cpad) {
  TORCH_CHECK(idx.scalar_type() == at::kLong, "idx must be int64");
  TORCH_CHECK(palette.scalar_type() == at::kFloat, "palette must be fp32");
  TORCH_CHECK(palette.device() == idx.device(), "synth_tiles: tensors on different devices");
  TORCH_CHECK(dims == 2 || dims == 3, "dims must be 2 or 3");
  channels(in_ch, cpad);
  TORCH_CHECK(classes >= 1 && palette.numel() == classes * in_ch, "palette must be [classes][in_ch]");
  TORCH_CHECK(grid >= 1 && grid <= tile && tile >= 1, "1 <= grid <= tile");
  TORCH_CHECK(tile <= 32768 && tile * tile * (dims == 3 ? tile : 1) * 8 < (int64_t)UINT32_MAX,
              "tile too large for the 32-bit per-pixel hash counter");
}

inline void tile_gather(T src, T lab, T idx, int64_t cpad) {
  TORCH_CHECK(src.scalar_type() == at::kByte && lab.scalar_type() == at::kByte, "uint8 dataset");
  TORCH_CHECK(idx.scalar_type() == at::kLong, "idx must be int64");
  TORCH_CHECK(lab.dim() >= 1 && src.dim() == lab.dim() + 1 && src.size(0) == lab.size(0),
              "images [N,...,C] / labels [N,...]");
  channels(src.size(-1), cpad);
  for (int64_t i = 1; i < lab.dim(); ++i) TORCH_CHECK(src.size(i) == lab.size(i), "spatial mismatch");
  TORCH_CHECK(lab.device() == src.device() && idx.device() == src.device(),
              "tile_gather: tensors on different devices");
}

// crop_gather and warp_gather: packed scenes (uint8 pixels [P, Cin], uint8 labels [P], int64 table
// [n, 3]), the op's rows `params` [B, k] (layout checked by the caller), optional (gain, bias)
inline void gather_args(const char* op, T scenes, T labels, T table, T params, OptT color, int64_t tile) {
  TORCH_CHECK(scenes.scalar_type() == at::kByte && scenes.dim() == 2, "scenes must be uint8 [pixels, Cin]");
  TORCH_CHECK(labels.scalar_type() == at::kByte && labels.dim() == 1 && labels.size(0) == scenes.size(0),
              "labels must be uint8 [pixels]");
  TORCH_CHECK(table.scalar_type() == at::kLong && table.dim() == 2 && table.size(1) == 3,
              "table must be int64 [n, 3] (pixel offset, H, W)");
  tile_range(tile);
  TORCH_CHECK(table.size(0) < (1LL << 31), "too many scenes");
  TORCH_CHECK(labels.device() == scenes.device() && table.device() == scenes.device() &&
              params.device() == scenes.device(), op, ": tensors on different devices");
  if (has(color))
    TORCH_CHECK(color->scalar_type() == at::kFloat && color->dim() == 2 && color->size(0) == params.size(0) &&
                color->size(1) == 2 && color->device() == scenes.device(),
                "color must be fp32 [B, 2] (gain, bias)");
}

inline void crop_gather(T scenes, T labels, T table, T params, OptT color, int64_t tile, int64_t cpad) {
  TORCH_CHECK(params.scalar_type() == at::kInt && params.dim() == 2 && params.size(1) == 4,
              "params must be int32 [B, 4] (scene, y0, x0, code)");
  gather_args("crop_gather", scenes, labels, table, params, color, tile);
  channels(scenes.size(1), cpad);
}

inline void warp_gather(T scenes, T labels, T table, T wparams, OptT color, int64_t tile, int64_t cpad) {
  TORCH_CHECK(wparams.scalar_type() == at::kLong && wparams.dim() == 2 && wparams.size(1) == 6,
              "wparams must be int64 [B, 6] (scene, cy, cx, code, A, Bm)");
  gather_args("warp_gather", scenes, labels, table, wparams, color, tile);
  TORCH_CHECK(cpad == 4 || cpad == 8, "cpad must be 4 or 8");
  TORCH_CHECK(scenes.size(1) >= 1 && scenes.size(1) <= cpad, "1 <= in_ch <= cpad");
}

// crop_params and warp_params: virtual sample numbers idx, cumulative counts cum [n + 1], table
inline void params_args(const char* op, T idx, T cum, T table, int64_t tile, int64_t mode) {
  TORCH_CHECK(idx.scalar_type() == at::kLong, "idx must be int64");
  TORCH_CHECK(table.scalar_type() == at::kLong && table.dim() == 2 && table.size(1) == 3 && table.size(0) >= 1,
              "table must be int64 [n >= 1, 3] (pixel offset, H, W)");
  TORCH_CHECK(cum.scalar_type() == at::kLong && cum.dim() == 1 && cum.size(0) == table.size(0) + 1,
              "cum must be int64 [n + 1]");
  TORCH_CHECK(cum.device() == idx.device() && table.device() == idx.device(), op,
              ": tensors on different devices");
  TORCH_CHECK(table.size(0) < (1LL << 31), "too many scenes");
  tile_range(tile);
  TORCH_CHECK(mode >= 0 && mode <= 2, "mode must be 0 (none), 1 (flip) or 2 (d4)");
  TORCH_CHECK(idx.numel() < (1LL << 31), "too many samples");
}

inline void warp_params(T idx, T cum, T table, T steps, T rot, int64_t tile, int64_t mode) {
  TORCH_CHECK(steps.scalar_type() == at::kInt && steps.dim() == 1 && steps.size(0) >= 1 &&
              steps.size(0) <= 65536, "steps must be int32 [S], 1 <= S <= 65536");
  TORCH_CHECK(rot.scalar_type() == at::kInt && rot.dim() == 2 && rot.size(1) == 2 && rot.size(0) >= 1 &&
              rot.size(0) <= 65536, "rot must be int32 [T, 2] (cos, sin), 1 <= T <= 65536");
  TORCH_CHECK(steps.device() == idx.device() && rot.device() == idx.device(),
              "warp_params: tensors on different devices");
  params_args("warp_params", idx, cum, table, tile, mode);
}

inline void origins(T o, T like) {
  TORCH_CHECK(o.scalar_type() == at::kInt && o.dim() == 2 && o.size(1) == 2,
              "origins must be int32 [B, 2] (y0, x0)");
  TORCH_CHECK(o.device() == like.device(), "origins must be on the scene's device");
}

// the symmetry codes of a call (int32 [S], 1 <= S <= 8) -> S; without codes S = 1 (the list {0})
inline int64_t codes(OptT c, T like) {
  if (!has(c)) return 1;
  TORCH_CHECK(c->scalar_type() == at::kInt && c->dim() == 1, "codes must be int32 [S]");
  TORCH_CHECK(c->device() == like.device(), "codes must be on the device of the other tensors");
  TORCH_CHECK(c->size(0) >= 1 && c->size(0) <= 8, "codes: 1 <= S <= 8");
  return c->size(0);
}

// a code list's values on the host: distinct, in 0..7 -> packed 3 bits each, code j at bits 3 j
inline uint32_t pack_code_values(const int* c, int64_t S) {
  uint32_t seen = 0u, packed = 0u;
  for (int64_t j = 0; j < S; ++j) {
    TORCH_CHECK(c[j] >= 0 && c[j] <= 7, "codes: values must lie in 0..7");
    TORCH_CHECK(!(seen & (1u << c[j])), "codes: values must be distinct");
    seen |= 1u << c[j];
    packed |= (uint32_t)c[j] << (3 * j);
  }
  return packed;
}

inline void window_gather(T scene, T o, int64_t tile, int64_t cpad) {
  TORCH_CHECK(scene.scalar_type() == at::kByte && scene.dim() == 3, "scene must be uint8 [H, W, Cin]");
  origins(o, scene);
  const int64_t H = scene.size(0), W = scene.size(1);
  TORCH_CHECK(H >= 1 && W >= 1 && H < (1 << 30) && W < (1 << 30), "scene size out of range");
  channels(scene.size(2), cpad);
  tile_range(tile);
  TORCH_CHECK(o.size(0) < (1 << 30), "too many windows");
}

// the window side of head_predict_accum (the (C, K) support test stays with each backend's head)
inline void head_predict_accum(T a, T Wh, T bh, T o, T win, T acc, int64_t S) {
  TORCH_CHECK(a.dim() == 4 && a.size(1) == a.size(2) && a.scalar_type() == at::kBFloat16,
              "a must be bf16 [B, tile, tile, C]");
  TORCH_CHECK(a.size(0) % S == 0, "a must hold S views per window: [B * S, ..]");
  TORCH_CHECK(Wh.dim() == 2 && Wh.size(1) == a.size(3) && bh.numel() == Wh.size(0), "Wh [K, C] / bh [K]");
  const int64_t B = a.size(0) / S, tile = a.size(1), K = Wh.size(0);
  origins(o, a);
  TORCH_CHECK(o.size(0) == B, "one origin per window");
  TORCH_CHECK(win.scalar_type() == at::kFloat && win.dim() == 1 && win.size(0) == tile, "win must be fp32 [tile]");
  TORCH_CHECK(acc.scalar_type() == at::kFloat && acc.dim() == 3 &&
              acc.size(2) == 4 * ((K + 4) / 4), "acc must be fp32 [H, W, 4 * ceil((K + 1) / 4)]");
  TORCH_CHECK(acc.size(0) < (1 << 30) && acc.size(1) < (1 << 30) && tile <= 32768 && a.size(0) < (1 << 30),
              "scene / window size out of range");
  TORCH_CHECK(Wh.device() == a.device() && bh.device() == a.device() && win.device() == a.device() &&
              acc.device() == a.device(), "device mismatch");
}

inline void scene_finalize(T acc, int64_t K, OptT labels) {
  TORCH_CHECK(acc.scalar_type() == at::kFloat && acc.dim() == 3 && acc.size(2) % 4 == 0,
              "acc must be fp32 [H, W, KA], KA % 4 == 0");
  TORCH_CHECK(K >= 1 && K <= 16 && K <= acc.size(2), "1 <= K <= min(16, KA)");
  if (has(labels))
    TORCH_CHECK(labels->scalar_type() == at::kByte && labels->dim() == 2 && labels->size(0) == acc.size(0) &&
                labels->size(1) == acc.size(1) && labels->device() == acc.device(), "labels must be uint8 [H, W]");
}

}  // namespace checks
}  // namespace ddlpc
